"""GPU: the graph product on random pairs of graphs against the model (tests/compose_model.py): node counts of 0-400 drawn independently
for the two sides, four densities, a forced tier or none.  BVG_COMPOSE_FUZZ=<n> sets the number of cases (default 60); every assertion
message carries the seed that rebuilds its case."""
import os

import numpy as np
import pytest

import compose_model as CM
import transform_model as M

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("BVG_COMPOSE_FUZZ", "60"))
SEED0 = 20260000


def case(seed):
    rng = np.random.default_rng(seed)
    n0, n1 = int(rng.integers(0, 401)), int(rng.integers(0, 401))
    d0, d1 = (float(rng.choice([0.0, 0.02, 0.2, 0.6])) for _ in range(2))
    la = [np.flatnonzero(rng.random(n0) < d0) for _ in range(n0)]
    lb = [np.flatnonzero(rng.random(n1) < d1) for _ in range(n1)]
    tier = [None, 0, 1, 2][int(rng.integers(0, 4))]
    return M.csr(la), M.csr(lb), tier


def test_random_pairs(W, monkeypatch):
    for seed in range(SEED0, SEED0 + CASES):
        a, b, tier = case(seed)
        what = "seed %d (n0 %d, n1 %d, tier %s)" % (seed, len(a[0]) - 1, len(b[0]) - 1, tier)
        if tier is None:
            monkeypatch.delenv("BVG_COMPOSE_TIER", raising=False)
        else:
            monkeypatch.setenv("BVG_COMPOSE_TIER", str(tier))
        want = CM.compose(a, b)
        ub = CM.bounds(a, b)
        with W.ParsedGraph.from_csr(*a) as ga, W.ParsedGraph.from_csr(*b) as gb:
            g, rep = W.compose(ga, gb, report=True)
            with g:
                off, adj = g.csr()
        assert np.array_equal(off.astype(np.int64), want[0]), what + ": offsets differ"
        assert np.array_equal(adj, want[1]), what + ": successors differ"
        assert rep["products"] == int(ub.sum()) and rep["arcs"] == len(want[1]) and sum(rep["rows"]) == int(np.sum(ub > 0)), what + ": report %r" % (rep,)
        if tier == 2:
            assert rep["rows"][:2] == [0, 0], what
