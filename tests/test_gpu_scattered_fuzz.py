"""GPU: randomised scattered arc lists against the model (tests/scattered_model.py).  BVG_SCATTERED_FUZZ=<n> sets the number of texts
(default 48, of at most 20 KB each).  The texts mix every kind of token, of break and of switch; the identifier pools are small, so that
repeats are the rule; every third text is read in a given numbering, and every text twice (nothing may depend on the lanes' order)."""
import os

import numpy as np
import pytest

import scattered_model as M

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("BVG_SCATTERED_FUZZ", "48"))
BAD = [b"x", b"+1", b"--1", b"1-", b"1x", b"\xff\xfe", b"#", b"1#2", b"9223372036854775808", b"-9223372036854775809", b"123456789012345678901234", b"1.5", b"0x10"]
BREAKS = [b"\n", b"\n", b"\n", b"\r", b"\r\n", b"\n\n", b"\r\r\n"]
BLANKS = [b" ", b" ", b"\t", b"  ", b" \t ", b"\x00", b"\x0b", b"\x1f "]


def random_text(rng):
    pool = np.concatenate([rng.integers(-(1 << 63), (1 << 63) - 1, rng.integers(1, 40), dtype=np.int64, endpoint=True), rng.integers(-3, 4, 8),
                           np.array([-1, 0, M.INT64_MIN, M.INT64_MAX])])
    pool = pool[:rng.integers(1, len(pool) + 1)]
    limit = int(rng.choice([200, 4000, 20000]))
    hub = int(pool[rng.integers(len(pool))])
    parts, size = [], 0

    def ident():
        if rng.random() < 0.3:
            return b"%d" % hub
        v = int(pool[rng.integers(len(pool))])
        s = b"%d" % v
        if rng.random() < 0.1:
            s = (b"-" if v < 0 else b"") + b"0" * int(rng.integers(1, 25)) + s.lstrip(b"-")
        return b"-" if v == 0 and rng.random() < 0.2 else s

    while size < limit:
        k = rng.random()
        blank = lambda: BLANKS[rng.integers(len(BLANKS))]
        if k < 0.05:
            line = b"#" + bytes(rng.integers(32, 127, rng.integers(0, 40)).astype(np.uint8))
        elif k < 0.10:
            line = b"".join(blank() for _ in range(rng.integers(0, 4)))
        elif k < 0.13:
            line = b"#" + b"c 1 2 " * int(rng.integers(100, 1700))                   # a comment across tiles
        else:
            toks = [ident(), ident()]
            if k < 0.30:
                toks[rng.integers(2)] = BAD[rng.integers(len(BAD))]
            if k > 0.9:
                toks = toks[:1]
            if rng.random() < 0.1:
                toks += [ident() if rng.random() < 0.5 else b"etc"]
            line = (blank() if rng.random() < 0.2 else b"") + blank().join(toks) + (blank() if rng.random() < 0.2 else b"")
        line += BREAKS[rng.integers(len(BREAKS))]
        parts.append(line); size += len(line)
    text = b"".join(parts)[:20000]
    return text.rstrip(b"\r\n") if rng.random() < 0.3 else text, pool


@pytest.mark.parametrize("seed", range(CASES))
def test_random_texts(W, seed):
    rng = np.random.default_rng(0x5CA7 + seed)
    text, pool = random_text(rng)
    sym, nol = bool(seed & 1), bool(seed & 2)
    known = None
    if seed % 3 == 2:
        known = np.unique(pool)
        known = known[rng.permutation(len(known))][:max(1, len(known) * 2 // 3)].tolist()
    want = M.parse(text, sym, nol, known)
    woff, wadj = M.csr(want["nodes"], want["arcs"])
    for _ in range(2):
        with W.parse_scattered_arcs(text, symmetrize=sym, no_loops=nol, ids=known) as g:
            off, adj = g.csr()
            assert g.ids.tolist() == want["ids"] and np.array_equal(off, woff) and np.array_equal(adj, wadj) and g.report == want["report"]
    rep = want["report"]
    try:
        W.parse_scattered_arcs(text, symmetrize=sym, no_loops=nol, ids=known, strict=True).close()
        assert rep["first_reason"] is None
    except W.IOException as e:
        assert (e.line, e.byte, e.reason) == (rep["first_line"], rep["first_byte"], rep["first_reason"])
