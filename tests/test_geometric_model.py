"""CPU: the numpy model of the exact geometric centralities (tests/geometric_model.py) on hand graphs whose answers are written here, and
its two ways of counting distances against each other."""
import math

import numpy as np

import geometric_model as M


def test_path_of_four_nodes():
    off, adj = M.csr_of(4, [(0, 1), (1, 2), (2, 3)])
    counts = M.distance_counts(off, adj, range(4))
    assert [c.tolist() for c in counts] == [[1, 1, 1, 1], [1, 1, 1], [1, 1], [1]]
    assert M.reachable(counts).tolist() == [4, 3, 2, 1]
    h = M.exact(counts, M.coefficient("harmonic"))
    assert h.dtype == np.float32 and h[0] == np.float32(1 + 1 / 2 + 1 / 3) and h.tolist()[1:] == [1.5, 1.0, 0.0]
    assert M.exact(counts, M.coefficient(("power", 1))).tolist() == [6.0, 3.0, 1.0, 0.0]          # the sums of the distances
    assert M.exact(counts, M.coefficient(("exp", 0.5))).tolist() == [1.875, 1.75, 1.5, 1.0]       # coefficient 0 is 1: the source counts
    assert M.exact(counts, M.coefficient([0, 1, 1])).tolist() == [2.0, 2.0, 1.0, 0.0]             # the nodes within two hops
    assert np.isinf(M.exact(counts, M.coefficient(("power", -1)))).all()                          # 0 ** -1
    assert M.histogram(counts).tolist() == [4, 3, 2, 1]
    c, r = M.reference_order(off, adj, 0, M.coefficient("harmonic"))
    assert r == 4 and c == np.float32(np.float32(np.float32(1.0) + 0.5) + 1 / 3)


def test_self_loop_counts_for_nothing():
    off, adj = M.csr_of(2, [(0, 0), (0, 1), (1, 0)])                                              # a 2-cycle, node 0 with a self-loop
    counts = M.distance_counts(off, adj, range(2))
    assert [c.tolist() for c in counts] == [[1, 1], [1, 1]]
    assert M.exact(counts, M.coefficient("harmonic")).tolist() == [1.0, 1.0] and M.reachable(counts).tolist() == [2, 2]
    assert [M.reference_order(off, adj, s, M.coefficient("harmonic")) for s in range(2)] == [(np.float32(1), 2), (np.float32(1), 2)]
    off, adj = M.csr_of(1, [(0, 0)])
    assert [c.tolist() for c in M.distance_counts(off, adj, [0])] == [[1]]


def test_coefficients():
    assert [M.coefficient("harmonic")(d) for d in range(3)] == [0.0, 1.0, 0.5]
    assert [M.coefficient(("power", 2))(d) for d in range(3)] == [0.0, 1.0, 4.0] and M.coefficient(("power", 0))(0) == 1.0
    assert M.coefficient(("power", -0.5))(0) == math.inf and M.coefficient(("power", -0.5))(4) == 0.5
    assert [M.coefficient(("exp", 3))(d) for d in range(3)] == [1.0, 3.0, 9.0]
    assert [M.coefficient([5, 7])(d) for d in range(4)] == [5.0, 7.0, 0.0, 0.0]


def test_the_two_counts_agree():
    rng = np.random.RandomState(5)
    n = 300
    arcs = [(int(x), int(y)) for x in range(n) for y in rng.randint(0, n, rng.poisson(1.5))]
    off, adj = M.csr_of(n, arcs)
    sources = list(range(40, 190))                                                                # three words, the last one partial
    a, b = M.distance_counts(off, adj, sources), M.distance_counts_pull(off, adj, sources)
    assert len(a) == len(b) == 150 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert max(len(x) for x in a) > 4 and len(set(M.reachable(a).tolist())) > 3                   # not a trivial graph
    for name, (k, hand) in M.HAND.items():
        off, adj = M.csr_of(k, hand)
        a, b = M.distance_counts(off, adj, range(k)), M.distance_counts_pull(off, adj, range(k))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    assert M.distance_counts_pull(off, adj, []) == []


def test_one_spacing():
    e = np.array([1.0, 3.0, np.inf], dtype=np.float32)
    up = np.nextafter(e, np.float32(np.inf))
    assert M.within_one_spacing(e, e) and M.within_one_spacing(up, e)
    assert not M.within_one_spacing(np.nextafter(up, np.float32(np.inf)), e)
    assert not M.within_one_spacing(np.array([1.0, 3.0, 3.0], dtype=np.float32), e)


def test_reference_order_bound_on_the_hand_graphs():
    """The reference's value is within reach * 2^-24 * value of the exact one: half an ulp per float addition of a growing positive sum."""
    for name, (k, hand) in M.HAND.items():
        off, adj = M.csr_of(k, hand)
        counts = M.distance_counts(off, adj, range(k))
        for cname, spec in M.COEFFS.items():
            coeff = M.coefficient(spec)
            value = M.exact_double(counts, coeff)
            for s in range(0, k, 7):
                c, r = M.reference_order(off, adj, s, coeff)
                assert r == int(counts[s].sum())
                if math.isinf(value[s]):
                    assert math.isinf(float(c)), (name, cname, s)
                else:
                    assert abs(float(c) - value[s]) <= r * 2.0 ** -24 * value[s], (name, cname, s)
