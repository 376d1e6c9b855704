"""Test helper of the tests of the analytics that share the arc-bounded sweep (csrc/bvg_plan.hip: SweepPlan; csrc/bvg_arcwalk.h).

empty_runs_graph: the graph on which the sweep meets node ranges that its batch plan leaves out.  plan_batches cuts at lower bounds in the
outdegree prefix sums, so a run of nodes without successors is attached to a neighbouring batch or belongs to none; under a budget of a few
arcs the runs at the start, in the middle and at the end of this graph fall on every such side.

chunk_edges_graph: the graph whose lists end on, just past and across the edges of the chunks of 64 arcs in which a wavefront walks the
arcs of 64 consecutive lists (csrc/bvg_arcwalk.h)."""
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


CHUNK_NODES = 200
CHUNK_LISTS = (0, 1, 127, 128, 199)             # the nodes that have successors


def chunk_edges_graph():
    """(off uint64[n + 1], succ int64[arcs]), no randomness.  In one batch that starts at node 0, the groups of 64 lists are nodes [0, 64), [64, 128),
    [128, 192) and the tail [192, 200); what each holds is asserted below.  Every node with a list is a successor of node 0 and has node 0 as
    a successor: reachable from 0 and on a cycle, so the kernels that filter lists (BFS levels, SCC propagation, frontiers) take them too."""
    n = CHUNK_NODES
    lists = [[] for _ in range(n)]
    lists[0] = [1] + list(range(2, 61)) + [127, 128, 199]                       # 63 arcs: the next list starts at arc 63 of the group
    lists[1] = [0, 127]                                                         # arcs 63 and 64: across the first chunk edge; the group totals 65
    lists[127] = [0] + list(range(136, 199))                                    # list 63 of its group, alone in it: 64 arcs, the group totals 64
    lists[128] = [0] + list(range(61, 188))                                     # list 0 of its group, alone in it: 128 arcs, two full chunks
    lists[199] = [0]                                                            # the last node of the tail group
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    succ = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    deg = np.diff(off.astype(np.int64))
    assert n <= 200 and all(l == sorted(set(l)) for l in lists) and np.flatnonzero(deg).tolist() == list(CHUNK_LISTS)
    assert deg[127] == 64 and deg[128] == 128                                   # lists of exactly one and exactly two chunks
    assert deg[0:64].sum() == 65 and deg[64:128].sum() == 64                    # groups of one chunk plus one arc, and of exactly one chunk
    assert np.flatnonzero(deg[64:128]).tolist() == [63]                         # a group whose only list is its last
    assert np.flatnonzero(deg[128:192]).tolist() == [0]                         # a group whose only list is its first
    assert int(off[1] - off[0]) == 63 and deg[1] == 2                           # a list over arcs 63 and 64 of its group
    assert len(set(succ.tolist())) == n                                         # every node is a successor
    assert all(x == 0 or x in lists[0] for x in CHUNK_LISTS) and all(0 in lists[x] for x in CHUNK_LISTS if x != 0)   # reachable from 0, on a cycle
    return off, succ
