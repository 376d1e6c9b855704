"""GPU: seeded random graphs and parameters through every EFGraph entry point against the model (tests/efgraph_model.py).
A short default set; BVG_EF_FUZZ=<n> runs n cases."""
import os

import numpy as np
import pytest

import efgraph_model as M

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("BVG_EF_FUZZ", "12"))


def _case(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([1, 2, 5, 64, 100, 300, 1000]))
    U = int(rng.choice([n, n + int(rng.integers(1, 100)), n * n + 1, 1 << int(rng.integers(20, 50))]))
    q = int(rng.integers(0, 9))
    mean = float(rng.choice([0.2, 3, 30]))
    forced = tuple(int(min(n, d)) for d in rng.choice([0, 1, 63, 64, 65, 200, n], size=min(n, 4)))
    return n, U, q, M.random_lists(n, int(mean * n), seed=seed, degrees=forced), str(rng.choice(["LITTLE_ENDIAN", "BIG_ENDIAN"]))


@pytest.mark.parametrize("seed", range(CASES))
def test_fuzz(W, seed, monkeypatch):
    n, U, q, lists, order = _case(seed)
    data, off, info = M.store(lists, U, q, order)
    graph, offsets = W.store_efgraph(lists, U, q, order)
    assert np.array_equal(offsets, off) and graph.tobytes() == data
    p = W.EFParams(nodes=n, arcs=info["arcs"], upper_bound=U, log2_quantum=q, big_endian=int(order == "BIG_ENDIAN"))
    flat = np.concatenate([np.asarray(l, np.int64) for l in lists]) if info["arcs"] else np.empty(0, np.int64)
    rng = np.random.default_rng(seed)
    batch = rng.integers(0, n, size=200)
    qn = rng.integers(0, n, size=2000); qb = rng.integers(0, n + 1, size=2000)
    want = np.array([(lambda a, i: int(a[i]) if i < len(a) else -1)(lists[x], int(np.searchsorted(lists[x], b))) for x, b in zip(qn, qb)])
    for given in (off, None):
        g = W.EFGraph.from_memory(p, data, given)
        for path in ("0", "1", "2"):
            monkeypatch.setenv("BVG_EF_PATH", path)
            deg, succ = g.decode_range(0, n)
            assert np.array_equal(deg, [len(l) for l in lists]) and np.array_equal(succ, flat)
            r = g.scan()
            assert (r["nodes"], r["arcs"], r["chk"]) == (n, info["arcs"], M.scan_checksum(lists))
            bdeg, bsucc = g.successors_batch(batch)
            assert np.array_equal(bsucc, np.concatenate([np.asarray(lists[x], np.int64) for x in batch]))
        for noptr in ("0", "1"):
            monkeypatch.setenv("BVG_EF_NOPTR", noptr)
            assert np.array_equal(g.skip_to(qn, qb), want)
        g.close()
