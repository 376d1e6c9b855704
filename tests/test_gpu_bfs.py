"""GPU: breadth-first visits on the device (bvg_bfs_*; algo/ParallelBreadthFirstVisit.java).

Every expected answer comes from a level-synchronous breadth-first search on the CPU (numpy) over the adjacency the test built itself or
the reference's golden cnr-2000 lists, restating the library's determinism: inside a level the queue is in increasing id, and a node's
parent is the smallest node of the previous level that has it as a successor.  Everything is compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import sweep_cases

GOLDEN_CNR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cnr-2000")

pytestmark = pytest.mark.gpu


# ---- the CPU side ----
def cpu_bfs(off, adj, start, seen=None):
    """(queue, cuts, dist, parent) of visit(start); `seen` (bool per node, updated) = the nodes marked by earlier visits."""
    off = np.asarray(off, dtype=np.int64); adj = np.asarray(adj, dtype=np.int64)
    n = len(off) - 1
    if seen is None:
        seen = np.zeros(n, dtype=bool)
    assert not seen[start]
    dist = np.full(n, -1, dtype=np.int32); parent = np.full(n, -1, dtype=np.int64)
    seen[start] = True; dist[start] = 0; parent[start] = start
    frontier = np.array([start], dtype=np.int64)
    levels, cuts, d = [frontier], [0, 1], 0
    while True:
        starts = off[frontier]; lens = off[frontier + 1] - starts
        total = int(lens.sum())
        if total == 0:
            break
        idx = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(total, dtype=np.int64)
        src = np.repeat(frontier, lens); tgt = adj[idx]
        new = ~seen[tgt]
        tgt, src = tgt[new], src[new]
        if len(tgt) == 0:
            break
        order = np.argsort(tgt, kind="stable")                                # (src is non-decreasing: the first of a run is the smallest parent)
        tgt, src = tgt[order], src[order]
        first = np.ones(len(tgt), dtype=bool); first[1:] = tgt[1:] != tgt[:-1]
        frontier = tgt[first]
        seen[frontier] = True; dist[frontier] = d + 1; parent[frontier] = src[first]
        levels.append(frontier); cuts.append(cuts[-1] + len(frontier)); d += 1
    return np.concatenate(levels), np.array(cuts, dtype=np.int64), dist, parent


def cpu_visit_all(off, adj, parent_mode):
    """visitAll() (ParallelBreadthFirstVisit.java:272-339): (marker, round, queue, cuts, dist) afterwards."""
    off = np.asarray(off, dtype=np.int64); adj = np.asarray(adj, dtype=np.int64)
    n = len(off) - 1
    marker = np.full(n, -1, dtype=np.int64); seen = np.zeros(n, dtype=bool)
    rnd, queue, cuts, dist = -1, np.empty(0, np.int64), np.empty(0, np.int64), np.full(n, -1, dtype=np.int32)
    for curr in np.arange(n):
        if seen[curr]:
            continue
        rnd += 1
        d = off[curr + 1] - off[curr]
        if d == 0 or (d == 1 and adj[off[curr]] == curr):                     # no expansion: queue and cut points stay (:309-317)
            seen[curr] = True; marker[curr] = curr if parent_mode else rnd
            continue
        queue, cuts, dist, par = cpu_bfs(off, adj, int(curr), seen)
        marker[queue] = par[queue] if parent_mode else rnd
    return marker, rnd, queue, cuts, dist


def csr_of_lists(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if len(lists):
        off[1:] = np.cumsum([len(l) for l in lists])
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) and off[-1] else np.empty(0, np.int64)
    return off, adj


def open_graph(W, tools, off, adj, params=None, **tuning):
    st = tools.store((off, adj), params, threads=2)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    if tuning:
        g.set_tuning(**tuning)
    return g


def check_state(v, queue, cuts, dist):
    assert np.array_equal(v.queue, queue)
    assert np.array_equal(v.cut_points, cuts)
    assert np.array_equal(v.dist, dist)
    assert v.max_distance() == len(cuts) - 2
    if len(queue):
        assert v.node_at_max_distance() == queue[-1]


def check_visit(g, off, adj, start, both_modes=True):
    """visit(start) on fresh objects (round and parent mode) against the CPU; returns what the CPU found and the round object's counters."""
    queue, cuts, dist, parent = cpu_bfs(off, adj, start)
    counters = None
    for pm in ((False, True) if both_modes else (False,)):
        with g.breadth_first_visit(parent=pm) as v:
            assert v.round == -1 and len(v.queue) == 0
            assert v.visit(start) == len(queue)
            assert v.round == 0
            check_state(v, queue, cuts, dist)
            m = v.marker
            if pm:
                assert np.array_equal(m, parent)
                assert m[start] == start
            else:
                assert np.array_equal(m, np.where(dist >= 0, 0, -1))
                counters = v.counters()
    return queue, cuts, dist, parent, counters


@pytest.fixture(scope="module")
def cnr(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.int64); off[1:] = np.cumsum(deg)
    return off, np.asarray(succ, dtype=np.int64)


# 1. the golden graph, with answers computed on the CPU when the feature was specified
CNR_KNOWN = {                       # start: (visited, max_distance, widest level, last queue element)
    0: (325557, 38, 48640, 69105),
    100000: (610, 19, 141, 99730),
    325556: (2, 1, 1, 122557),
    3: (1, 0, 1, 3),
}


@pytest.mark.parametrize("start", sorted(CNR_KNOWN))
def test_cnr2000_visits(W, cnr, start):
    off, adj = cnr
    g = W.BVGraph.load(GOLDEN_CNR)
    queue, cuts, dist, parent, _ = check_visit(g, off, adj, start)
    visited, maxd, widest, last = CNR_KNOWN[start]
    assert (len(queue), len(cuts) - 2, int(np.diff(cuts).max()), int(queue[-1])) == (visited, maxd, widest, last)
    if start == 3:
        assert off[4] == off[3]                                                # no successors
    if start == 325556:
        assert sorted(queue.tolist()) == [122557, 325556]
    # parents: in the previous level, with the node as a successor, and the smallest such (re-derived here, not taken from cpu_bfs)
    reached = np.flatnonzero((dist > 0))
    assert np.all(dist[parent[reached]] == dist[reached] - 1)
    for y in reached[:: max(1, len(reached) // 500)].tolist():
        p = int(parent[y])
        assert y in adj[off[p]:off[p + 1]]
        prev = queue[cuts[dist[y] - 1]:cuts[dist[y]]]
        smaller = prev[prev < p]
        assert not any(y in adj[off[u]:off[u + 1]] for u in smaller[-50:].tolist())


# 2. both routes, the arc budget, and the switch between the routes
@pytest.mark.parametrize("route,budget,small", [("frontier", None, None), ("sweep", None, None), ("frontier", "9973", None), ("sweep", "99991", "0"), (None, None, "0"),
                                                ("frontier", None, "7")])
def test_cnr2000_routes_give_the_same_visit(W, cnr, monkeypatch, route, budget, small):
    off, adj = cnr
    for k, val in (("BVG_BFS_ROUTE", route), ("BVG_BFS_BATCH_ARCS", budget), ("BVG_BFS_SMALL", small)):
        if val is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, val)
    g = W.BVGraph.load(GOLDEN_CNR)
    for start in (0, 100000):
        queue, cuts, dist, parent, c = check_visit(g, off, adj, start, both_modes=(start != 0 or route is None))
        levels = len(cuts) - 1
        assert c["frontier_levels"] + c["sweep_levels"] == levels
        if route == "frontier":
            assert c["sweep_levels"] == 0 and c["frontier_batches"] >= 1
            if budget and start == 0:
                assert c["frontier_batches"] > levels                          # levels cut into several batches
        elif route == "sweep":
            assert c["frontier_levels"] == 0 and c["sweep_batches"] >= levels
            if budget:
                assert c["sweep_batches"] >= levels * (3216152 // int(budget))
        else:                                                                  # the default: the switch must separate these
            assert c["first_level_route"] == 1
            if start == 0:
                assert c["sweep_levels"] >= 1 and c["frontier_levels"] >= 1
            else:
                assert c["sweep_levels"] == 0
        if small == "0":
            assert c["sorted_levels"] == 0 and c["compacted_levels"] == levels - 1
        elif small is None and start == 100000:
            assert c["compacted_levels"] == 0


@pytest.mark.parametrize("route", ["frontier", "sweep"])
@pytest.mark.parametrize("budget", ["1", "97"])
def test_tiny_budgets(W, tools, cnr, monkeypatch, route, budget):
    monkeypatch.setenv("BVG_BFS_ROUTE", route); monkeypatch.setenv("BVG_BFS_BATCH_ARCS", budget)
    n = 300 if budget == "1" else 1500                                         # (one arc per batch: thousands of batches per sweep)
    off, adj = tools.synth_adjacency(n, seed=5, synth=tools.web_like(p_empty=0.3, mean_deg=6.0, max_deg=200, local_gap=100.0))
    assert np.diff(off.astype(np.int64)).max() > int(budget)                   # some lists exceed the budget
    g = open_graph(W, tools, off, adj)
    deg = np.diff(off.astype(np.int64))
    for start in (int(np.argmax(deg)), 0, n - 1):
        check_visit(g, off, adj, start)
    if route == "frontier":                                                    # small visits of the golden graph with one arc per batch
        coff, cadj = cnr
        gc = W.BVGraph.load(GOLDEN_CNR)
        for start in (100000, 325556):
            check_visit(gc, coff, cadj, start, both_modes=False)


# 3. every decode route
ROUTES = {
    "default": {},
    "force_slow": dict(force_slow=True),
    "no_index": dict(no_index=1),
    "marks_only": dict(no_index=2),
    "force_wide": dict(force_wide=True),                                       # 64-bit markers on a small graph
}


@pytest.mark.parametrize("bfs_route", [None, "frontier", "sweep"])
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape,seed", [("web", 1), ("eu", 3)])
def test_synthetic_graphs_every_route(W, tools, monkeypatch, route, shape, seed, bfs_route):
    if bfs_route:
        monkeypatch.setenv("BVG_BFS_ROUTE", bfs_route)
    else:
        monkeypatch.delenv("BVG_BFS_ROUTE", raising=False)
    n = 6000 if shape == "eu" else 20000
    synth = tools.web_like(p_empty=0.3, mean_deg=4.0, local_gap=40.0, p_far=0.2) if shape == "web" else tools.eu_like(p_empty=0.3, mean_deg=30.0)
    off, adj = tools.synth_adjacency(n, seed=seed, synth=synth)
    g = open_graph(W, tools, off, adj, **ROUTES[route])
    deg = np.diff(off.astype(np.int64))
    sizes = []
    for start in (0, int(np.argmax(deg)), n // 2, n - 1):
        queue = check_visit(g, off, adj, start)[0]
        sizes.append(len(queue))
    assert max(sizes) > 100
    marker, rnd, queue, cuts, dist = cpu_visit_all(off, adj, False)
    with g.breadth_first_visit() as v:
        v.visit_all()
        assert v.round == rnd and np.array_equal(v.marker, marker)
        check_state(v, queue, cuts, dist)


@pytest.mark.parametrize("window,n", [(70, 8400), (20, 600)])
def test_unbounded_reference_chains_take_the_deep_fallback(W, tools, monkeypatch, window, n):
    """Identical lists three nodes apart and maxrefcount = -1: reference chains as long as the graph.  A request block holds a chain that
    reaches up to 64 nodes back (8192 with a window above 64, which runs on the global-memory kernel); longer ones go through the block
    plan.  The visits stay small (a request near the end decodes its whole chain, whichever way it goes)."""
    monkeypatch.setenv("BVG_BFS_ROUTE", "frontier")
    shared = [n - 19, n - 15, n - 14, n - 13, n - 10, n - 5, n - 1]
    lists = [sorted(set(shared + [n - 400 + x % 3])) for x in range(n)]
    off, adj = csr_of_lists(lists)
    g = open_graph(W, tools, off, adj, W.default_params(window_size=window, max_ref_count=-1))
    deep = 0
    for start in (0, n - 1):
        queue, _, _, _, c = check_visit(g, off, adj, start, both_modes=start == 0)
        deep += c["deep_requests"]
        assert len(queue) >= 10
    assert deep > 0                                                            # some request's chain did not fit a request block


# 5. state across visits
def test_state_across_visits(W, tools):
    n = 4000
    off, adj = tools.synth_adjacency(n, seed=21, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    g = open_graph(W, tools, off, adj)
    h = g.copy()
    v = h.breadth_first_visit()
    h.close()                                                                  # the object holds its own flyweight
    seen = np.zeros(n, dtype=bool)
    q0, c0, d0, _ = cpu_bfs(off, adj, 0, seen)
    assert v.visit(0) == len(q0) and v.round == 0
    inside = int(q0[-1])
    assert v.visit(inside) == 0 and v.round == 0                               # marked already: nothing changes
    check_state(v, q0, c0, d0)
    other = int(np.flatnonzero(~seen)[0])
    first_seen = seen.copy()
    q1, c1, d1, _ = cpu_bfs(off, adj, other, seen)
    assert v.visit(other) == len(q1) and v.round == 1
    check_state(v, q1, c1, d1)
    m = v.marker
    assert np.all(m[first_seen] == 0) and np.all(m[q1] == 1) and np.all(m[~seen] == -1)
    v.clear()
    assert v.round == -1 and np.all(v.marker == -1) and len(v.queue) == 0 and np.all(v.dist == -1)
    assert v.visit(inside) == len(cpu_bfs(off, adj, inside)[0]) and v.round == 0
    v.close()
    v.close()


# 6. visit_all
def _symmetrise(off, adj):
    n = len(off) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(off, dtype=np.int64)))
    pairs = np.unique(np.stack([np.concatenate([src, adj]), np.concatenate([adj, src])]), axis=1)
    soff = np.zeros(n + 1, dtype=np.uint64); soff[1:] = np.cumsum(np.bincount(pairs[0], minlength=n))
    return soff, pairs[1].astype(np.int64)


@pytest.mark.parametrize("parent_mode", [False, True])
def test_visit_all_symmetric_equals_components(W, tools, parent_mode):
    n = 20000
    off, adj = tools.synth_adjacency(n, seed=11, synth=tools.web_like(p_empty=0.6, mean_deg=2.0, local_gap=10.0))
    adj = adj.copy(); off = off.copy()
    soff, sadj = _symmetrise(off, adj)
    lists = [sadj[soff[x]:soff[x + 1]] for x in range(n)]
    lists = [l[l < n - 5] if x < n - 5 else l[:0] for x, l in enumerate(lists)]   # the last five nodes isolated
    isolated = [x for x in range(n) if len(lists[x]) == 0]
    assert len(isolated) > 10
    lists[isolated[3]] = np.array([isolated[3]])                                # lone self-loops
    lists[isolated[7]] = np.array([isolated[7]])
    soff, sadj = csr_of_lists(lists)
    g = open_graph(W, tools, soff, sadj)
    cc = g.connected_components()
    marker, rnd, queue, cuts, dist = cpu_visit_all(soff, sadj, parent_mode)
    with g.breadth_first_visit(parent=parent_mode) as v:
        v.visit_all()
        assert v.round == rnd and v.round + 1 == cc.count
        assert np.array_equal(v.marker, marker)
        if not parent_mode:
            assert np.array_equal(v.marker, cc.component)
        check_state(v, queue, cuts, dist)                                      # those of the last expanding visit
        assert len(queue) and any(x > queue[0] for x in isolated)              # (isolated nodes after it did not replace them)


@pytest.mark.parametrize("parent_mode", [False, True])
def test_visit_all_directed(W, tools, cnr, parent_mode):
    n = 30000
    coff, cadj = cnr
    a, b = 100000, 100000 + n                                                  # a slice of cnr-2000, arcs inside blocks of 500 nodes
    src = np.repeat(np.arange(a, b), np.diff(coff[a:b + 1])); dst = cadj[coff[a]:coff[b]]
    keep = (dst >= a) & (dst < b) & ((src - a) // 500 == (dst - a) // 500)
    s, d = src[keep] - a, dst[keep] - a
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(np.bincount(s, minlength=n))
    lists = [d[int(off[x]):int(off[x + 1])] for x in range(n)]
    empty = [x for x in range(n) if len(lists[x]) == 0]
    assert len(empty) > 10
    lists[empty[2]] = np.array([empty[2]]); lists[empty[-2]] = np.array([empty[-2]])   # lone self-loops
    for x in range(n - 10, n):                                                 # out-arc-less nodes after the last expanding visit
        lists[x] = np.empty(0, np.int64)
    empty = [x for x in range(n) if len(lists[x]) == 0]
    off, d = csr_of_lists(lists)
    deg = np.diff(off.astype(np.int64))
    marker, rnd, queue, cuts, dist = cpu_visit_all(off, d, parent_mode)
    rounds = cpu_visit_all(off, d, False)[0]
    firsts = np.unique(rounds, return_index=True)[1]                           # the node every visit started from
    assert (deg[firsts] == 0).any() and (np.bincount(rounds) > 1).any()        # out-arc-less starts (isolated, or reached by nobody before), real visits
    assert any(x > queue[0] for x in empty)                                    # non-expanding visits after the last expanding one
    g = open_graph(W, tools, off, d, W.default_params(min_interval_length=3))
    with g.breadth_first_visit(parent=parent_mode) as v:
        v.visit_all()
        assert v.round == rnd and np.array_equal(v.marker, marker)
        check_state(v, queue, cuts, dist)
        v.visit_all()                                                          # clears first: the same again
        assert v.round == rnd and np.array_equal(v.marker, marker)


def test_visit_all_of_isolated_nodes(W, tools):
    n = 200000
    off = np.zeros(n + 1, dtype=np.uint64)
    g = open_graph(W, tools, off, np.empty(0, np.int64))
    with g.breadth_first_visit() as v:
        v.visit_all()
        assert v.round == n - 1 and np.array_equal(v.marker, np.arange(n)) and len(v.queue) == 0 and len(v.cut_points) == 0
        assert np.all(v.dist == -1)
    with g.breadth_first_visit(parent=True) as v:
        v.visit_all()
        assert v.round == n - 1 and np.array_equal(v.marker, np.arange(n))


# 7. shapes that break visits
@pytest.mark.parametrize("small", [None, "0"])
def test_path(W, tools, monkeypatch, small):
    if small is None:
        monkeypatch.delenv("BVG_BFS_SMALL", raising=False)
    else:
        monkeypatch.setenv("BVG_BFS_SMALL", small)
    n = 3000
    off, adj = csr_of_lists([[x + 1] if x + 1 < n else [] for x in range(n)])
    g = open_graph(W, tools, off, adj)
    queue, cuts, dist, parent, c = check_visit(g, off, adj, 0, both_modes=small is None)
    assert len(cuts) - 2 == n - 1 and np.array_equal(queue, np.arange(n))
    assert c["sweep_levels"] == 0
    check_visit(g, off, adj, n - 5, both_modes=False)


@pytest.mark.parametrize("route", [None, "frontier", "sweep"])
def test_star_longer_than_the_budget(W, tools, monkeypatch, route):
    monkeypatch.setenv("BVG_BFS_BATCH_ARCS", "1000")
    if route:
        monkeypatch.setenv("BVG_BFS_ROUTE", route)
    else:
        monkeypatch.delenv("BVG_BFS_ROUTE", raising=False)
    n = 50000
    lists = [[] for _ in range(n)]
    lists[7] = [x for x in range(n) if x != 7 and x % 3]
    lists[100] = [7]
    off, adj = csr_of_lists(lists)
    g = open_graph(W, tools, off, adj)
    for start in (7, 100, 3):
        check_visit(g, off, adj, start)


# long runs of nodes without successors at the start, in the middle and at the end: node ranges the sweep's batch plan leaves out
@pytest.mark.parametrize("budget", ["1", "97"])
def test_empty_runs_under_tiny_budgets(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_BFS_ROUTE", "sweep"); monkeypatch.setenv("BVG_BFS_BATCH_ARCS", budget)
    off, adj = sweep_cases.empty_runs_graph()
    assert np.diff(off.astype(np.int64)).max() > int(budget)                   # the longest list exceeds the budget
    g = open_graph(W, tools, off, adj)
    _, _, dist, _, c = check_visit(g, off, adj, sweep_cases.LONG_NODE)
    assert c["frontier_levels"] == 0 and c["sweep_batches"] > c["sweep_levels"] > 2
    assert all((dist[lo:hi] > 0).any() for lo, hi in sweep_cases.EMPTY)         # nodes of every empty run are reached
    check_visit(g, off, adj, sweep_cases.NODES - 1, both_modes=False)          # from a node without successors


# lists and groups of 64 lists that end on, just past and across the edges of the mark kernel's chunks of 64 arcs (sweep route, both modes)
@pytest.mark.parametrize("budget", [None, "61"])
def test_chunk_edges_under_budgets(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_BFS_ROUTE", "sweep")
    if budget is None:
        monkeypatch.delenv("BVG_BFS_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_BFS_BATCH_ARCS", budget)
    off, adj = sweep_cases.chunk_edges_graph()
    g = open_graph(W, tools, off, adj)
    for start in (0, 128):                                                     # level 1 expands every other list at once; from 128: node 0 alone
        queue, _, dist, _, c = check_visit(g, off, adj, start)
        assert len(queue) == sweep_cases.CHUNK_NODES and c["frontier_levels"] == 0 and c["sweep_levels"] >= 3
        assert all(dist[x] <= 2 for x in sweep_cases.CHUNK_LISTS)


@pytest.mark.parametrize("depth", [1, 5, 12])
def test_complete_binary_trees(W, tools, depth):
    n = (1 << (depth + 1)) - 1
    out = [[2 * x + 1, 2 * x + 2] if 2 * x + 2 < n else [] for x in range(n)]
    inn = [[(x - 1) // 2] if x else [] for x in range(n)]
    for lists, start, reach in ((out, 0, n), (inn, n - 1, depth + 1), (out, n - 1, 1), (inn, 0, 1)):
        off, adj = csr_of_lists(lists)
        g = open_graph(W, tools, off, adj)
        queue, cuts, _, _, _ = check_visit(g, off, adj, start)
        assert len(queue) == reach
    assert np.array_equal(np.diff(cpu_bfs(*csr_of_lists(out), 0)[1]), 1 << np.arange(depth + 1))


def test_empty_and_one_node_graphs(W, tools):
    st = tools.store([])
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    with g.breadth_first_visit() as v:
        v.visit_all()
        assert v.round == -1 and len(v.queue) == 0 and len(v.marker) == 0 and len(v.dist) == 0
        with pytest.raises(W.IllegalArgumentException):
            v.visit(0)
    for lists in ([[]], [[0]]):
        off, adj = csr_of_lists(lists)
        g = open_graph(W, tools, off, adj)
        check_visit(g, off, adj, 0)
        with g.breadth_first_visit() as v:
            v.visit_all()
            assert v.round == 0 and v.marker.tolist() == [0] and len(v.queue) == 0   # no expansion: the queue stays empty


# 8. errors
def test_errors(W, tools):
    off, adj = tools.synth_adjacency(1000, seed=1)
    g = open_graph(W, tools, off, adj)
    L = W.bvgraph._bfs_fns()
    with g.breadth_first_visit() as v:
        for bad in (-1, 1000, 1 << 40):
            with pytest.raises(W.IllegalArgumentException):
                v.visit(bad)
        assert v.round == -1
        k = v.visit(0)
        q = np.zeros(max(k, 1), dtype=np.int64); cp = np.zeros(64, dtype=np.uint64)
        if k > 1:
            assert L.bvg_bfs_get(v._v, None, q.ctypes.data, k - 1, None, 0, None) == W.E_CAPACITY
        assert L.bvg_bfs_get(v._v, None, None, 0, cp.ctypes.data, 1, None) == W.E_CAPACITY
        assert L.bvg_bfs_get(v._v, None, q.ctypes.data, k, None, 0, None) == 0 and q[0] == 0
    h = C.c_void_p()
    assert L.bvg_bfs_create(g._h, 2, C.byref(h)) == W.E_ARG                     # unknown flag bits
    g.set_node_base(1000)
    with pytest.raises(W.IllegalArgumentException):
        g.breadth_first_visit()


@pytest.mark.parametrize("route", ["frontier", "sweep"])
def test_successor_outside_the_graph_is_eof(W, monkeypatch, route):
    from bvrecords import Record, assemble
    monkeypatch.setenv("BVG_BFS_ROUTE", route)
    recs = [Record(d=1, residuals=[1]), Record(d=1, residuals=[0]), Record(d=1, residuals=[9])]   # 0 <-> 1, and node 2 -> 9 in a 3-node graph
    gbytes, offs, _ = assemble(recs)
    p = W.default_params().clone(nodes=3, arcs=3)
    g = W.BVGraph.from_memory(p, np.frombuffer(gbytes, dtype=np.uint8), offs)
    with g.breadth_first_visit() as v:
        assert v.visit(1) == 2
        with pytest.raises(W.EOFException):
            v.visit(2)
        assert v.round == -1 and np.all(v.marker == -1) and len(v.queue) == 0   # cleared, and usable
        assert v.visit(1) == 2 and v.queue.tolist() == [1, 0] and v.round == 0
        with pytest.raises(W.EOFException):
            v.visit_all()
        assert v.round == -1 and np.all(v.marker == -1)


# 9. randomised parity
def test_random_graphs_random_starts(W, tools, monkeypatch):
    cases = max(1, int(os.environ.get("BVG_FUZZ", "12")))
    rng = np.random.default_rng(20261016)
    for case in range(cases):
        n = int(rng.integers(1, 3000))
        m = int(rng.integers(0, 6 * n))
        src = rng.integers(0, n, m); dst = (src + rng.integers(-50, 50, m)) % n if rng.random() < 0.5 else rng.integers(0, n, m)
        pairs = np.unique(np.stack([src, dst]), axis=1)
        off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(np.bincount(pairs[0], minlength=n))
        adj = pairs[1].astype(np.int64)
        params = W.default_params(window_size=int(rng.integers(0, 12)), max_ref_count=int(rng.integers(1, 6)), min_interval_length=int(rng.choice([0, 2, 3, 4])),
                                  zeta_k=int(rng.integers(1, 6)))
        for k, choices in (("BVG_BFS_ROUTE", [None, "frontier", "sweep"]), ("BVG_BFS_BATCH_ARCS", [None, "61", "1009"]), ("BVG_BFS_SMALL", [None, "0", "5"])):
            val = choices[int(rng.integers(0, len(choices)))]
            if val is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, val)
        g = open_graph(W, tools, off, adj, params)
        for start in rng.integers(0, n, 3).tolist():
            check_visit(g, off, adj, int(start))
        pm = bool(rng.integers(0, 2))
        marker, rnd, queue, cuts, dist = cpu_visit_all(off, adj, pm)
        with g.breadth_first_visit(parent=pm) as v:
            v.visit_all()
            assert v.round == rnd and np.array_equal(v.marker, marker), "case %d" % case
            check_state(v, queue, cuts, dist)
