"""GPU: weakly connected components on the device (bvg_components; algo/ConnectedComponents.java).

Every expected answer comes from the CPU: scipy's connected_components(connection="weak") when it is importable, a plain union-find
otherwise, over the adjacency the test built itself (or the reference's golden cnr-2000 lists), canonicalised to the reference's
numbering -- component c is the one whose smallest node is the c-th smallest among the components' smallest nodes
(ParallelBreadthFirstVisit.visitAll, ParallelBreadthFirstVisit.java:272-337)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sweep_cases

GOLDEN_CNR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cnr-2000")

pytestmark = pytest.mark.gpu


# ---- the CPU side ----
def _uf_labels(n, src, dst):
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for u, v in zip(src.tolist(), dst.tolist()):
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def cpu_components(n, src, dst):
    """(count, comp[n], sizes[count]) in the reference's numbering."""
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    if n == 0:
        return 0, np.empty(0, np.int64), np.empty(0, np.int64)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        m = coo_matrix((np.ones(len(src), dtype=np.int8), (src, dst)), shape=(n, n)).tocsr()
        k, lab = connected_components(m, directed=True, connection="weak")
        lab = lab.astype(np.int64)
    except ImportError:
        lab = _uf_labels(n, src, dst)
        _, lab = np.unique(lab, return_inverse=True)
        k = int(lab.max()) + 1
    first = np.full(k, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n, dtype=np.int64))
    rank = np.empty(k, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(k, dtype=np.int64)
    comp = rank[lab]
    return int(k), comp, np.bincount(comp, minlength=k).astype(np.int64)


def sorted_by_size(comp, sizes):
    """sortBySize with ties by increasing old index (= smallest node)."""
    k = len(sizes)
    order = np.lexsort((np.arange(k), -sizes))
    newidx = np.empty(k, dtype=np.int64); newidx[order] = np.arange(k, dtype=np.int64)
    return newidx[comp], sizes[order]


def arcs_of(off, adj):
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)), np.asarray(adj, dtype=np.int64)


def check(g, n, src, dst, sort=True):
    k, comp, sizes = cpu_components(n, src, dst)
    r = g.connected_components(sizes=True)
    assert r.count == k
    assert np.array_equal(r.component, comp)
    assert np.array_equal(r.sizes, sizes)
    if sort:
        rs = g.connected_components(sizes=True, sort_by_size=True)
        c2, s2 = sorted_by_size(comp, sizes)
        assert rs.count == k and np.array_equal(rs.component, c2) and np.array_equal(rs.sizes, s2)
    return k, comp, sizes


@pytest.fixture(scope="module")
def cnr_arcs(cnr_csr):
    deg, succ = cnr_csr
    return np.repeat(np.arange(len(deg), dtype=np.int64), deg), succ


def _cut(src, dst, n, B):
    keep = (src // B) == (dst // B)
    s, d = src[keep], dst[keep]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(s, minlength=n)).astype(np.uint64)
    return off, d, s


# 1. the golden graph: weakly connected
def test_cnr2000_is_one_component(W, cnr_arcs):
    g = W.BVGraph.load(GOLDEN_CNR)
    n = g.num_nodes()
    src, dst = cnr_arcs
    k, comp, sizes = cpu_components(n, src, dst)
    assert (k, sizes.tolist()) == (1, [325557])                                # (the issue's known answer, scipy)
    for h in (g, g.copy()):
        r = h.connected_components(sizes=True)
        assert r.count == 1 and not r.component.any() and r.sizes.tolist() == [325557]
        rs = h.connected_components(sizes=True, sort_by_size=True)
        assert rs.count == 1 and not rs.component.any() and rs.sizes.tolist() == [325557]


# 2. cnr-2000 cut into many components: isolated nodes, self-loops, components whose smallest node has no out-arcs
@pytest.mark.parametrize("B", [1024, 4096, 300])
def test_cnr2000_cut_into_blocks(W, tools, cnr_arcs, B):
    src, dst = cnr_arcs
    n = 325557
    off, adj, s = _cut(src, dst, n, B)
    st = tools.store((off, adj), W.default_params(min_interval_length=3), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    k, comp, sizes = check(g, n, s, adj)
    assert k > n // B                                                          # many components
    outdeg = np.diff(off.astype(np.int64))
    firsts = np.unique(comp, return_index=True)[1]                             # the smallest node of every component
    assert (outdeg[firsts] == 0).any() and (sizes > 1)[comp[firsts]].any()      # some smallest nodes are reached only as targets
    assert (s == adj).any()                                                    # self-loops in the cut


# 3. synthetic graphs under every decode route
ROUTES = {
    "default": {},
    "force_slow": dict(force_slow=True),
    "no_index": dict(no_index=1),
    "marks_only": dict(no_index=2),
    "force_wide": dict(force_wide=True),                                       # the 64-bit parent array on a small graph
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape,seed", [("web", 1), ("web", 2), ("eu", 3)])
def test_synthetic_graphs_every_route(W, tools, route, shape, seed):
    n = 6000 if shape == "eu" else 20000
    synth = tools.web_like(p_empty=0.5, mean_deg=4.0, local_gap=40.0) if shape == "web" else tools.eu_like(p_empty=0.3, mean_deg=30.0)
    off, adj = tools.synth_adjacency(n, seed=seed, synth=synth)
    if shape == "eu":                                                          # (one giant component otherwise: cut it into blocks of 700 nodes)
        off, adj, _ = _cut(*arcs_of(off, adj), n, 700)
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    if ROUTES[route]:
        g.set_tuning(**ROUTES[route])
    src, dst = arcs_of(off, adj)
    k, _, _ = check(g, n, src, dst, sort=route == "default")
    assert k > 1


def test_window_above_64_takes_the_slow_kernel(W, tools):
    n = 5000
    off, adj = tools.synth_adjacency(n, seed=9, synth=tools.web_like(p_empty=0.5, mean_deg=4.0))
    st = tools.store((off, adj), W.default_params(window_size=70, max_ref_count=-1), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    src, dst = arcs_of(off, adj)
    check(g, n, src, dst)


# 4. batch boundaries: tiny batches, a prime, unlimited -- components span batches, lists longer than the budget
@pytest.mark.parametrize("budget", ["1", "97", None])
def test_batch_boundaries_do_not_change_the_result(W, tools, monkeypatch, budget):
    n = 3000
    off, adj = tools.synth_adjacency(n, seed=5, synth=tools.web_like(p_empty=0.4, mean_deg=6.0, max_deg=400, local_gap=200.0))
    deg = np.diff(off.astype(np.int64))
    assert deg.max() > 97                                                      # some lists exceed the small budget
    st = tools.store((off, adj), threads=2)
    if budget is None:
        monkeypatch.delenv("BVG_CC_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_CC_BATCH_ARCS", budget)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    src, dst = arcs_of(off, adj)
    k, comp, sizes = check(g, n, src, dst)
    assert sizes.max() > 97                                                    # a component that spans several batches of 97 arcs


# 4b. long runs of nodes without successors at the start, in the middle and at the end: node ranges the batch plan leaves out
@pytest.mark.parametrize("budget", ["1", "97"])
def test_empty_runs_under_tiny_budgets(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_CC_BATCH_ARCS", budget)
    off, adj = sweep_cases.empty_runs_graph()
    assert np.diff(off.astype(np.int64)).max() > int(budget)                   # the longest list exceeds the budget
    st = tools.store((off, adj), threads=2)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    check(g, len(off) - 1, *arcs_of(off, adj))


# 4c. lists and groups of 64 lists that end on, just past and across the edges of the hook kernel's chunks of 64 arcs
@pytest.mark.parametrize("budget", [None, "61"])
def test_chunk_edges_under_budgets(W, tools, monkeypatch, budget):
    if budget is None:
        monkeypatch.delenv("BVG_CC_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_CC_BATCH_ARCS", budget)
    off, adj = sweep_cases.chunk_edges_graph()
    st = tools.store((off, adj), threads=2)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    k, _, sizes = check(g, len(off) - 1, *arcs_of(off, adj))
    assert k == 1 and sizes[0] == sweep_cases.CHUNK_NODES                      # every node is a successor of a node with a list


# 5. sortBySize and a sizes buffer that is too small
def test_sort_by_size_and_capacity(W, tools):
    n = 20000
    off, adj = tools.synth_adjacency(n, seed=11, synth=tools.web_like(p_empty=0.6, mean_deg=2.0, local_gap=10.0))
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    src, dst = arcs_of(off, adj)
    k, comp, sizes = cpu_components(n, src, dst)
    rs = g.connected_components(sizes=True, sort_by_size=True)
    assert np.all(np.diff(rs.sizes) <= 0) and rs.sizes.sum() == n
    ties = np.flatnonzero(np.diff(rs.sizes) == 0)
    firsts = np.full(k, n, dtype=np.int64); np.minimum.at(firsts, rs.component, np.arange(n))
    assert np.all(firsts[ties] < firsts[ties + 1])                             # ties: increasing smallest node
    assert len(ties) > 10
    # the same partition as unsorted
    r = g.connected_components()
    assert r.sizes is None and r.count == k
    pairs = np.unique(np.stack([r.component, rs.component]), axis=1)
    assert pairs.shape[1] == k
    # sizes_cap too small: BVG_E_CAPACITY, the count reported, comp written
    L = W.lib(); W.bvgraph._components_fns()
    comp_buf = np.full(n, -7, dtype=np.int64); sz = np.zeros(4, dtype=np.int64); cnt = C.c_uint64()
    st_ = L.bvg_components(g._h, 0, comp_buf.ctypes.data, sz.ctypes.data, 4, C.byref(cnt))
    assert st_ == W.E_CAPACITY and cnt.value == k and np.array_equal(comp_buf, comp)
    assert L.bvg_components(g._h, 2, comp_buf.ctypes.data, None, 0, C.byref(cnt)) == W.E_ARG   # unknown flag bits


# 6. tiled graphs: copy j is the base shifted by j * n0
def test_tiled_graph(W, tools):
    n0, K = 4000, 7
    off, adj = tools.synth_adjacency(n0, seed=21, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    st = tools.store((off, adj), threads=2)
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    c0, comp0, sizes0 = cpu_components(n0, *arcs_of(off, adj))
    g = base.tile(K)
    r = g.connected_components(sizes=True)
    assert r.count == K * c0
    expect = (np.arange(K, dtype=np.int64)[:, None] * c0 + comp0[None, :]).ravel()
    assert np.array_equal(r.component, expect) and np.array_equal(r.sizes, np.tile(sizes0, K))


def _body_past_2_to_32(W, tools, torch):
    n0 = 1 << 19
    off, adj = tools.synth_adjacency(n0, seed=77, synth=tools.web_like(mean_deg=3.0, p_empty=0.5, max_deg=200))
    st = tools.store((off, adj), threads=4)
    c0, comp0, _ = cpu_components(n0, *arcs_of(off, adj))
    tiles = (1 << 32) // n0 + 3
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    try:
        g = base.tile(tiles)
        n = g.num_nodes()
        comp = torch.empty(n, dtype=torch.int64, device="cuda")
        k = g.connected_components_dev(comp)
    except (MemoryError, torch.cuda.OutOfMemoryError):
        print("SKIP needs ~150 GB of HBM")
        return
    assert n > (1 << 32) and k == tiles * c0, (n, k, tiles, c0)
    t0 = torch.from_numpy(comp0).cuda()
    step = 256
    for j in range(0, tiles, step):                                            # tile by tile on the device: copy j = base labels + j * C0
        m = min(step, tiles - j)
        got = comp[j * n0:(j + m) * n0].view(m, n0)
        want = t0[None, :] + (torch.arange(j, j + m, device="cuda", dtype=torch.int64)[:, None] * c0)
        assert torch.equal(got, want), "tiles %d..%d" % (j, j + m - 1)


def _run_child(name):
    """torch-tensor tests run in a fresh child process that imports torch before the product library (torch's HIP runtime and the
    library's must be the same one: tests/test_gpu_device_buffers.py)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=560)
    if r.returncode == 0 and "SKIP" in r.stdout:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_tiled_past_2_to_32_nodes_on_the_64_bit_path():
    _run_child("past_2_to_32")


# 7. what is refused
def test_shard_handle_is_refused(W, tools):
    off, adj = tools.synth_adjacency(1000, seed=1)
    st = tools.store((off, adj))
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    g.set_node_base(1000)
    with pytest.raises(W.IllegalArgumentException):
        g.connected_components()


def test_successor_outside_the_graph_is_eof(W):
    from bvrecords import Record, assemble
    recs = [Record(d=2, residuals=[1, 2]), Record(d=1, residuals=[0]), Record(d=1, residuals=[9])]   # node 2 -> 9 in a 3-node graph
    gbytes, offs, _ = assemble(recs)
    p = W.default_params().clone(nodes=3, arcs=4)
    g = W.BVGraph.from_memory(p, np.frombuffer(gbytes, dtype=np.uint8), offs)
    with pytest.raises(W.EOFException):
        g.connected_components()


def test_empty_graph(W, tools):
    st = tools.store([])
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    r = g.connected_components(sizes=True)
    assert r.count == 0 and len(r.component) == 0 and len(r.sizes) == 0


# 8. the CAS interleaving does not leak into the result
def test_two_runs_are_identical(W, tools):
    n = 200000
    off, adj = tools.synth_adjacency(n, seed=13, synth=tools.web_like(p_empty=0.3, mean_deg=3.0, local_gap=50.0, p_far=0.2))
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    a = g.connected_components(sizes=True, sort_by_size=True)
    b = g.copy().connected_components(sizes=True, sort_by_size=True)
    assert a.count == b.count and np.array_equal(a.component, b.component) and np.array_equal(a.sizes, b.sizes)
    k, comp, sizes = cpu_components(n, *arcs_of(off, adj))
    c2, s2 = sorted_by_size(comp, sizes)
    assert np.array_equal(a.component, c2) and np.array_equal(a.sizes, s2)


def _body_device_buffers(W, tools, torch):
    n = 30000
    off, adj = tools.synth_adjacency(n, seed=17, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    k, comp, sizes = cpu_components(n, *arcs_of(off, adj))
    dc = torch.empty(n, dtype=torch.int64, device="cuda"); ds = torch.empty(k, dtype=torch.int64, device="cuda")
    assert g.connected_components_dev(dc, ds) == k
    assert np.array_equal(dc.cpu().numpy(), comp) and np.array_equal(ds.cpu().numpy(), sizes)
    dc.fill_(-1)
    try:
        g.connected_components_dev(dc, torch.empty(k - 1, dtype=torch.int64, device="cuda"))
        raise AssertionError("no IllegalArgumentException for a short sizes buffer")
    except W.IllegalArgumentException:
        pass
    assert np.array_equal(dc.cpu().numpy(), comp)                             # comp written all the same
    c2, s2 = sorted_by_size(comp, sizes)
    assert g.connected_components_dev(dc, ds, sort_by_size=True) == k
    assert np.array_equal(dc.cpu().numpy(), c2) and np.array_equal(ds.cpu().numpy(), s2)


def test_device_buffers_match_host():
    _run_child("device_buffers")


if __name__ == "__main__":
    import torch                                                              # (before the product library)
    torch.cuda.init()
    _HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_HERE), _HERE]
    import tooling
    import webgraph_big_amd
    tooling.lib()
    globals()["_body_" + sys.argv[1]](webgraph_big_amd, tooling, torch)
    print("CHILD OK")
