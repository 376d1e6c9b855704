"""GPU: the labelled graph product on random pairs of small labelled graphs against the model (tests/lcompose_model.py), refusals included: node
counts of 0-300 drawn independently for the two sides, skewed degrees (a few heavy rows on the left, a few popular targets on the right, so that
some rows pile their products onto few keys), a random semiring, label class, width of the sources and of the result, a forced tier or none
and a workspace of one table or the default.  A refused case counts as checked: the device must refuse it with the model's count and first
arc.  BVG_LCOMPOSE_FUZZ=<n> sets the number of cases (default 60); every assertion message carries the seed that rebuilds its case."""
import os

import numpy as np
import pytest

import lcompose_model as LC

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("BVG_LCOMPOSE_FUZZ", "60"))
SEED0 = 20261000


def skewed(rng, n, targets, density, heavy, popular, lab_max):
    """n rows over [0, targets): every arc with probability `density`, `heavy` rows that hold most targets, `popular` targets most rows hold."""
    if not n or not targets:
        return LC.from_rows([[] for _ in range(n)])
    m = rng.random((n, targets)) < density
    for x in rng.integers(0, n, size=heavy):
        m[x] |= rng.random(targets) < 0.8
    for z in rng.integers(0, targets, size=popular):
        m[:, z] |= rng.random(n) < 0.8
    return LC.from_rows([[(int(z), int(rng.integers(0, lab_max + 1))) for z in np.flatnonzero(row)] for row in m])


def case(seed):
    rng = np.random.default_rng(seed)
    n0, n1 = int(rng.integers(0, 301)), int(rng.integers(0, 301))
    kind = int(rng.choice([LC.GAMMA, LC.FIXED]))
    width = int(rng.choice([1, 4, 8, 16, 31])) if kind == LC.FIXED else 0
    # a third of the gamma cases draw labels from all of [0, 2^31): their sums and products leave the class
    lab_max = (1 << width) - 1 if kind == LC.FIXED else int(rng.choice([3, 1000, (1 << 31) - 1]))
    out_width = None if kind == LC.GAMMA else [None, max(0, width - 1), min(31, width + 1), min(31, 2 * width), 31][int(rng.integers(0, 5))]
    a = skewed(rng, n0, n0, float(rng.choice([0.0, 0.02, 0.2])), int(rng.integers(0, 3)), 0, lab_max)
    b = skewed(rng, n1, n1, float(rng.choice([0.0, 0.02, 0.2])), 0, int(rng.integers(0, 3)), lab_max)
    semiring = int(rng.integers(0, 5))
    tier = [None, 0, 1, 2][int(rng.integers(0, 4))]
    ws = [None, 1][int(rng.integers(0, 2))]
    return a, b, semiring, kind, width, out_width, tier, ws


def test_random_pairs(W, monkeypatch):
    refused = 0
    for seed in range(SEED0, SEED0 + CASES):
        a, b, semiring, kind, width, out_width, tier, ws = case(seed)
        what = "seed %d (n0 %d, n1 %d, semiring %d, kind %d, width %d -> %s, tier %s, ws %s)" % (seed, len(a[0]) - 1, len(b[0]) - 1, semiring, kind, width, out_width, tier, ws)
        for name, v in (("BVG_COMPOSE_TIER", tier), ("BVG_COMPOSE_WS", ws)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
        want = LC.compose(a, b, semiring, kind, width if out_width is None else out_width)
        with W.LabelledGraph.from_csr(a[0], a[1], a[2], kind, width) as ga, W.LabelledGraph.from_csr(b[0], b[1], b[2], kind, width) as gb:
            if want[0] == "range":
                refused += 1
                with pytest.raises(W.IllegalArgumentException) as e:
                    W.compose_labelled(ga, gb, semiring, out_width=out_width)
                assert getattr(e.value, "out_of_range", None) == want[1] and e.value.first_arc == want[2], what
                continue
            g, rep = W.compose_labelled(ga, gb, semiring, out_width=out_width, report=True)
            with g:
                off, adj, lab = g.csr()
                assert (g.kind, g.width) == (kind, (width if out_width is None else out_width) if kind == LC.FIXED else 0), what
        assert np.array_equal(off.astype(np.int64), want[1][0]), what + ": offsets differ"
        assert np.array_equal(adj, want[1][1]), what + ": successors differ"
        assert np.array_equal(lab.astype(np.int64), want[1][2]), what + ": labels differ"
        assert rep["arcs"] == len(adj) and rep["out_of_range"] == 0, what + ": report %r" % (rep,)
        if tier == 2:
            assert rep["rows"][:2] == [0, 0], what
            assert rep["batches"] == (rep["rows"][2] if ws == 1 else min(1, rep["rows"][2])), what
    if CASES >= 60:
        assert 5 <= refused <= CASES - 20                                      # both kinds of case are well represented
