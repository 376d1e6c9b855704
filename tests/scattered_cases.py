"""The reference's own expectations of ScatteredArcsASCIIGraph, restated as data: (text, symmetrize, no_loops, arcs, ids).  From the class
documentation (example.arcs) and from ScatteredArcsASCIIGraphTest.testConstructor; shared by the model's test and the GPU tests."""

COMPLETE3 = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]


def _sym(arcs):
    return sorted(set(arcs) | {(t, s) for s, t in arcs})


EXAMPLE_ARCS = (b"# My graph\n-1 15\n15 2\n2 -1 This will cause a warning to be logged\nOOPS! (This will cause an error to be logged)\n-1 2\n")

_PLAIN = [
    (b"0 1\n0 2\n1 0\n1 2\n2 0\n2 1", COMPLETE3, [0, 1, 2]),
    (b"-1 15\n15 2\n2 -1\nOOPS!\n-1 2", [(0, 1), (0, 2), (1, 2), (2, 0)], [-1, 15, 2]),
    (b"0 1\n0 2\n1  0\n1 \t 2\n2 0\n2 1", COMPLETE3, [0, 1, 2]),                    # multiple blanks, TAB
    (b"2 0\n2 1", [(0, 1), (0, 2)], [2, 0, 1]),
    (b"1 2", [(0, 1)], [1, 2]),
    (b"2 1", [(0, 1)], [2, 1]),
    (b"0 1\n2 1", [(0, 1), (2, 1)], [0, 1, 2]),
    (b"\n0 1\n\n2 1", [(0, 1), (2, 1)], [0, 1, 2]),
    (b"\n0 1\n# comment\n2\n2 1\n2 X", [(0, 1), (2, 1)], [0, 1, 2]),
]

REFERENCE_CASES = ([(EXAMPLE_ARCS, False, False, [(0, 1), (0, 2), (1, 2), (2, 0)], [-1, 15, 2])]
                   + [(t, False, False, a, i) for t, a, i in _PLAIN]
                   + [(t, True, False, _sym(a), i) for t, a, i in _PLAIN]
                   + [(b"0 0\n0 1\n0 2\n2 2\n1 0\n1 2\n2 0\n2 1", True, True, COMPLETE3, [0, 1, 2])])
