"""Test helper of tests/test_gpu_components.py, tests/test_gpu_bfs.py and tests/test_gpu_hyperball.py: the graph on which the arc-bounded sweep
the three share (csrc/bvg_plan.hip: SweepPlan) meets node ranges that its batch plan leaves out.  plan_batches cuts at lower bounds in the
outdegree prefix sums, so a run of nodes without successors is attached to a neighbouring batch or belongs to none; under a budget of a few
arcs the runs at the start, in the middle and at the end of this graph fall on every such side."""
import numpy as np

NODES = 1000
EMPTY = ((0, 200), (400, 600), (800, 1000))     # node ranges [lo, hi) whose lists are empty (they are still targets)
LONG_NODE, LONG_ARCS = 300, 150                 # one list longer than any budget the tests set


def empty_runs_graph(seed=2026):
    """(off uint64[n + 1], succ int64[arcs]): Poisson(3) lists with targets anywhere in [0, n) outside EMPTY, one list of LONG_ARCS arcs."""
    n = NODES
    rng = np.random.RandomState(seed)
    lists = [sorted(set(int(y) for y in rng.randint(0, n, rng.poisson(3.0)))) for _ in range(n)]
    lists[LONG_NODE] = sorted(int(y) for y in rng.choice(n, LONG_ARCS, replace=False))
    for lo, hi in EMPTY:
        for x in range(lo, hi):
            lists[x] = []
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    succ = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    deg = np.diff(off.astype(np.int64))
    assert deg.max() == LONG_ARCS and all(not deg[lo:hi].any() for lo, hi in EMPTY)
    assert all(np.any((succ >= lo) & (succ < hi)) for lo, hi in EMPTY)             # the empty nodes are reached
    return off, succ
