"""GPU: randomised parity of the text graph entry points with the model (tests/textgraph_model.py), both formats, both directions.
200 small cases by default; BVG_TEXT_FUZZ=<n> sets the count.  Each case draws a graph, the separators and line breaks of its text, a
chunking for the formatter and, one time in three, a defect; the seed of a failing case is in the assertion message."""
import os

import numpy as np
import pytest

import textgraph_model as M
from test_gpu_text import lib_record, model_record

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("BVG_TEXT_FUZZ", "200"))
SEPARATORS = [b" ", b"\t", b"  ", b" \t", b"\x0b", b"\x01 ", b"\x1f"]
BREAKS = [b"\n", b"\r\n", b"\r"]
JUNK = [b"-", b".", b"/", b"#", b"x", b"\xff", b"\"", b"+", b" ", b"\n", b"\r", b"7", b"99999999999999999999", b"00"]


def join(pieces):
    """The text of the pieces; a lone '\\r' break in front of a '\\n' would read as one "\\r\\n", so such a '\\r' becomes "\\r\\n" itself."""
    out = []
    for p in pieces:
        if p.startswith(b"\n") and out and out[-1].endswith(b"\r"):
            out.append(b"\n")
        if p:
            out.append(p)
    return b"".join(out)


def random_lists(rng):
    n = int(rng.choice([0, 1, 2, 5, 17, 64, 65, 130]))
    dens = rng.choice([0.0, 0.05, 0.3, 0.6])
    return [np.flatnonzero(rng.random(n) < dens).tolist() for _ in range(n)]


def ascii_text(rng, lists):
    out = [b"%d" % len(lists), BREAKS[rng.integers(3)]]
    for l in lists:
        if rng.random() < 0.3:
            out.append(SEPARATORS[rng.integers(len(SEPARATORS))])
        for v in l:
            out += [b"0" * int(rng.integers(0, 3) if rng.random() < 0.2 else 0), b"%d" % v, SEPARATORS[rng.integers(len(SEPARATORS))]]
        out.append(BREAKS[rng.integers(3)])
    if rng.random() < 0.3:
        out.append(b"never read - . /")
    return join(out)


def arcs_text(rng, lists, shift):
    pairs = [(x, t) for x, l in enumerate(lists) for t in l]
    pairs += [pairs[i] for i in rng.integers(0, len(pairs), size=len(pairs) // 4)] if pairs else []
    order = rng.permutation(len(pairs))
    base = max(0, -shift)                             # ids in the text: a negative shift brings them back to the nodes
    out = []
    for i in order:
        s, t = pairs[i]
        r = rng.random()
        if r < 0.1:
            out += [b"# a comment ", JUNK[rng.integers(len(JUNK) - 5)], BREAKS[rng.integers(3)]]
        elif r < 0.2:
            out += [SEPARATORS[rng.integers(len(SEPARATORS))] if r < 0.15 else b"", BREAKS[rng.integers(3)]]
        out += [b"%d" % (s + base), SEPARATORS[rng.integers(len(SEPARATORS))], b"%d" % (t + base), SEPARATORS[rng.integers(len(SEPARATORS))] if rng.random() < 0.3 else b"",
                BREAKS[rng.integers(3)]]
    text = join(out)
    return text[:-1] if text and rng.random() < 0.2 and not text.endswith(b"\r\n") else text


def damage(rng, text):
    kind = rng.integers(4)
    at = int(rng.integers(0, len(text) + 1))
    if kind == 0:
        return text[:at] + JUNK[rng.integers(len(JUNK))] + text[at:]
    if kind == 1:
        return text[:at]
    if kind == 2 and at < len(text):
        return text[:at] + text[at + 1:]
    return text[:at] + JUNK[rng.integers(len(JUNK))] + text[at + int(rng.integers(1, 4)):]


def test_fuzz_parse_and_format(W):
    for case in range(CASES):
        seed = 77000 + case
        rng = np.random.default_rng(seed)
        lists = random_lists(rng)
        n = len(lists)
        # parse, ASCIIGraph
        text = ascii_text(rng, lists)
        if rng.random() < 1 / 3:
            text = damage(rng, text)
        got, want = lib_record(W.parse_ascii_graph, text), model_record(M.parse_ascii, text)
        assert got == want, ("seed %d ascii" % seed, text, got, want)
        # parse, arc list
        shift = int(rng.choice([0, 0, 1, -3, -7]))       # (small: a defect that glues two ids together must not ask for a graph of 10^9 nodes)
        kw = dict(shift=shift, symmetrize=bool(rng.integers(2)), no_loops=bool(rng.integers(2)), min_nodes=int(rng.choice([0, 0, n, n + 3])))
        text = arcs_text(rng, lists, shift)
        if rng.random() < 1 / 3:
            text = damage(rng, text)
        got, want = lib_record(W.parse_arc_list, text, **kw), model_record(M.parse_arcs, text, **kw)
        assert got == want, ("seed %d arcs %r" % (seed, kw), text, got, want)
        # format, from a stored BVGraph in random node ranges and from the CSR
        off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
        adj = np.array([v for l in lists for v in l], dtype=np.int64)
        assert W.format_csr(W.TEXT_ASCII, 0, off, adj) == M.format_ascii(lists), "seed %d format_csr" % seed
        shift = abs(shift)                            # (written ids stay at or above 0)
        assert W.format_csr(W.TEXT_ARCS, 4, off, adj, shift) == M.format_arcs(lists, 4, shift), "seed %d format_csr arcs" % seed
        if n and case % 4 == 0:
            p = W.default_params(window_size=int(rng.integers(0, 8)), min_interval_length=int(rng.choice([0, 2, 4])))
            graph, offsets = W.store((off, adj), p)
            p.nodes, p.arcs = n, len(adj)
            g = W.BVGraph.from_memory(p, graph, offsets)
            cuts = sorted(set([0, n] + rng.integers(0, n + 1, size=int(rng.integers(0, 5))).tolist()))
            assert b"".join(g.format_ascii(a, b) for a, b in zip(cuts, cuts[1:])) == M.format_ascii(lists), "seed %d format_ascii %r" % (seed, cuts)
            assert b"".join(g.format_arcs(a, b, shift) for a, b in zip(cuts, cuts[1:])) == M.format_arcs(lists, 0, shift), "seed %d format_arcs %r" % (seed, cuts)
            g.close()
