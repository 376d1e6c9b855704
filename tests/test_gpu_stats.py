"""GPU: graph statistics on the device (bvg_stats_*; Stats.java).  Every expected answer comes from tests/stats_model.py, a plain
restatement of Stats.run over the adjacency the test built itself (or the reference's golden cnr-2000 lists)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stats_model as SM
import sweep_cases

GOLDEN_CNR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cnr-2000")

pytestmark = pytest.mark.gpu


def graph_of(W, tools, off, adj, params=None, threads=2):
    st = tools.store((off, adj), params, threads=threads) if params is not None else tools.store((off, adj), threads=threads)
    return W.BVGraph.from_memory(st.params, st.graph, st.offsets)


def check(W, tools, off, adj, params=None, tuning=None, what=""):
    g = graph_of(W, tools, off, adj, params)
    if tuning:
        g.set_tuning(**tuning)
    m = SM.model(off, adj)
    SM.assert_same(g.stats(indegrees=True), m, what=what)
    return g, m


@pytest.fixture(scope="module")
def cnr_model(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.uint64); off[1:] = np.cumsum(deg, dtype=np.uint64)
    return SM.model(off, succ)


# 1. the golden graph from disk
def test_cnr2000_from_disk(W, cnr_model):
    g = W.BVGraph.load(GOLDEN_CNR)
    for h in (g, g.copy()):
        r = h.stats(indegrees=True)
        SM.assert_same(r, cnr_model)
        assert (r.max_indegree, r.max_indegree_node) == (18235, 205307)        # five nodes tie: the largest of them
    r = g.stats()
    assert r.indegrees is None
    SM.assert_same(r, cnr_model, indegrees=False)


# 2. node ranges the batch plan leaves out, lists longer than the budget
@pytest.mark.parametrize("budget", [None, "7", "61", "1009"])
def test_empty_runs_under_every_budget(W, tools, monkeypatch, budget):
    if budget is None:
        monkeypatch.delenv("BVG_STATS_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_STATS_BATCH_ARCS", budget)
    off, adj = sweep_cases.empty_runs_graph()
    deg = np.diff(off.astype(np.int64))
    _, m = check(W, tools, off, adj)
    zeros = int(np.count_nonzero(deg == 0))
    assert m["dangling"] == zeros and zeros > 600                              # the 600 nodes of the empty runs and the Poisson zeros
    assert zeros - 600 == int(np.count_nonzero(deg[200:400] == 0) + np.count_nonzero(deg[600:800] == 0))


# 2b. lists and groups of 64 lists that end on, just past and across the edges of the sweep kernel's chunks of 64 arcs
@pytest.mark.parametrize("budget", [None, "61"])
def test_chunk_edges_under_budgets(W, tools, monkeypatch, budget):
    if budget is None:
        monkeypatch.delenv("BVG_STATS_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_STATS_BATCH_ARCS", budget)
    off, adj = sweep_cases.chunk_edges_graph()
    _, m = check(W, tools, off, adj)
    assert m["dangling"] == sweep_cases.CHUNK_NODES - len(sweep_cases.CHUNK_LISTS)


# 3. sizes around a wavefront and a workgroup
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_a_wavefront_and_a_workgroup(W, tools, n):
    off, adj = tools.synth_adjacency(n, seed=n, synth=tools.web_like(p_empty=0.5))
    check(W, tools, off, adj, what="web")
    off, adj = tools.synth_adjacency(n, seed=n + 1, synth=tools.eu_like(p_empty=0.0, mean_deg=min(90.0, n / 2)))
    check(W, tools, off, adj, what="dense")


# 4. hubs: one address, two addresses, one address per wavefront's worth of lists; ties everywhere
@pytest.mark.parametrize("shape", ["one", "two", "per64", "complete"])
def test_hubs(W, tools, monkeypatch, shape):
    n = 300 if shape == "complete" else 5000
    x = np.arange(n, dtype=np.int64)
    if shape == "one":
        lists = [[0]] * n
    elif shape == "two":
        lists = [[0, 1]] * n
    elif shape == "per64":
        lists = [[int(v)] for v in x // 64 * 64]
    else:
        lists = [list(range(n))] * n
    off, adj = SM.csr(lists)
    g, m = check(W, tools, off, adj, what=shape)
    if shape == "one":
        assert (m["max_indegree"], m["max_indegree_node"], m["loops"], m["terminal"]) == (n, 0, 1, 1)
    if shape == "complete":
        assert (m["min_outdegree"], m["max_outdegree"], m["min_outdegree_node"], m["max_outdegree_node"]) == (n, n, 0, 0)
        assert (m["min_indegree"], m["max_indegree"], m["min_indegree_node"], m["max_indegree_node"]) == (n, n, n - 1, n - 1)
    # the combining form of the scatter gives the same
    monkeypatch.setenv("BVG_STATS_SCATTER", "elect")
    SM.assert_same(g.stats(indegrees=True), m, what=shape + " elect")


# 5. carries of the 128-bit sums
def test_sum_seed_carries_into_the_high_word(W, tools, monkeypatch):
    seed = (1 << 64) - 1000
    monkeypatch.setenv("BVG_STATS_SUM_SEED", str(seed))
    off, adj = tools.synth_adjacency(1000, seed=3, synth=tools.web_like(p_empty=0.3, mean_deg=8.0, local_gap=30.0))
    g = graph_of(W, tools, off, adj)
    m = SM.model(off, adj)
    assert m["tot_gap"] > 1000 and m["tot_loc"] > 1000
    r = g.stats()
    assert r.tot_gap == seed + m["tot_gap"] and r.tot_loc == seed + m["tot_loc"]
    assert r.tot_gap >> 64 == 1 and r.tot_loc >> 64 == 1
    monkeypatch.delenv("BVG_STATS_SUM_SEED")
    SM.assert_same(g.stats(), m, indegrees=False)


# 6. the 64-bit path, windows, codings
def test_force_wide_is_identical(W, tools):
    off, adj = tools.synth_adjacency(3000, seed=5, synth=tools.web_like(p_empty=0.4, mean_deg=6.0, max_deg=400, local_gap=200.0))
    check(W, tools, off, adj, tuning=dict(force_wide=True))


PARAMS = [dict(window_size=0, max_ref_count=0), dict(window_size=70, max_ref_count=-1), dict(residual_coding=1), dict(residual_coding=2),
          dict(residual_coding=3, zeta_k=2), dict(residual_coding=6, zeta_k=1), dict(residual_coding=7)]


@pytest.mark.parametrize("kw", PARAMS, ids=lambda kw: "-".join("%s%s" % (k[0], v) for k, v in kw.items()))
def test_windows_and_codings(W, tools, kw):
    off, adj = tools.synth_adjacency(2000, seed=9, synth=tools.web_like(p_empty=0.5, mean_deg=4.0))
    check(W, tools, off, adj, params=W.default_params(**kw))


# 7. tiled graphs: copy j is the base shifted by j * n0
def test_tiled_graph(W, tools):
    n0, K = 4000, 7
    off, adj = tools.synth_adjacency(n0, seed=21, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    base = graph_of(W, tools, off, adj)
    m = SM.model(off, adj)
    r = base.tile(K).stats(indegrees=True)
    for k in ("nodes", "arcs", "loops", "dangling", "terminal", "num_gaps", "tot_gap", "tot_loc"):
        assert getattr(r, k) == K * m[k], k
    assert r.log_delta == [K * v for v in m["log_delta"]]
    assert np.array_equal(r.outdegree_distribution, K * m["outdegree_distribution"]) and np.array_equal(r.indegree_distribution, K * m["indegree_distribution"])
    assert np.array_equal(r.indegrees, np.tile(m["indegrees"], K))
    for k in ("min_outdegree", "max_outdegree", "min_indegree", "max_indegree"):
        assert getattr(r, k) == m[k], k
    assert (r.min_outdegree_node, r.max_outdegree_node) == (m["min_outdegree_node"], m["max_outdegree_node"])                  # tile 0
    assert (r.min_indegree_node, r.max_indegree_node) == (m["min_indegree_node"] + (K - 1) * n0, m["max_indegree_node"] + (K - 1) * n0)   # tile K - 1


# 8. what is refused, states
def test_shard_handle_is_refused(W, tools):
    off, adj = tools.synth_adjacency(1000, seed=1)
    g = graph_of(W, tools, off, adj)
    g.set_node_base(1000)
    with pytest.raises(W.IllegalArgumentException):
        g.stats()


def test_successor_outside_the_graph_is_eof(W):
    from bvrecords import Record, assemble
    recs = [Record(d=2, residuals=[1, 2]), Record(d=1, residuals=[0]), Record(d=1, residuals=[9])]   # node 2 -> 9 in a 3-node graph
    gbytes, offs, _ = assemble(recs)
    p = W.default_params().clone(nodes=3, arcs=4)
    g = W.BVGraph.from_memory(p, np.frombuffer(gbytes, dtype=np.uint8), offs)
    with pytest.raises(W.EOFException):
        g.stats()


def test_capacity_ranges_and_states(W, tools):
    n = 3000
    off, adj = tools.synth_adjacency(n, seed=11, synth=tools.web_like(p_empty=0.4, mean_deg=5.0))
    g = graph_of(W, tools, off, adj)
    m = SM.model(off, adj)
    L = W.bvgraph._stats_fns()
    h = C.c_void_p()
    assert L.bvg_stats_compute(g._h, 2, C.byref(h)) == W.E_ARG and not h.value   # unknown flag bits
    assert L.bvg_stats_compute(g._h, W._abi.STATS_KEEP_INDEGREES_FLAG, C.byref(h)) == 0
    try:
        for which, key in ((W._abi.STATS_OUT, "outdegree_distribution"), (W._abi.STATS_IN, "indegree_distribution")):
            want = m[key]; ln = C.c_uint64(0)
            buf = np.full(len(want) + 1, 77, dtype=np.uint64)
            assert L.bvg_stats_distribution(h, which, buf.ctypes.data, len(want) - 1, C.byref(ln)) == W.E_CAPACITY
            assert ln.value == len(want) and (buf == 77).all()
            assert L.bvg_stats_distribution(h, which, buf.ctypes.data, len(want), C.byref(ln)) == 0
            assert ln.value == len(want) and np.array_equal(buf[:-1], want) and buf[-1] == 77
        assert L.bvg_stats_distribution(h, 2, None, 0, C.byref(ln)) == W.E_ARG
        for frm, to in ((0, n), (0, 0), (n, n), (17, 18), (63, 257), (n - 5, n)):
            out = np.full(to - frm + 1, -7, dtype=np.int64)
            assert L.bvg_stats_indegrees(h, frm, to, out.ctypes.data) == 0, (frm, to)
            assert np.array_equal(out[:-1], m["indegrees"][frm:to]) and out[-1] == -7, (frm, to)
        out = np.full(4, -7, dtype=np.int64)
        for frm, to in ((-1, 2), (2, 1), (0, n + 1), (n + 1, n + 1)):
            assert L.bvg_stats_indegrees(h, frm, to, out.ctypes.data) == W.E_ARG, (frm, to)
        assert (out == -7).all()
    finally:
        L.bvg_stats_close(h)
    assert L.bvg_stats_compute(g._h, 0, C.byref(h)) == 0                       # without KEEP_INDEGREES: no per-node array
    try:
        assert L.bvg_stats_indegrees(h, 0, n, out.ctypes.data) == W.E_UNSUPPORTED and (out == -7).all()
        sm = W.StatsSummary()
        assert L.bvg_stats_get(h, C.byref(sm)) == 0 and sm.arcs == m["arcs"] and sm.max_indegree_node == m["max_indegree_node"]
    finally:
        L.bvg_stats_close(h)


def test_two_runs_are_identical(W, tools):
    n = 100000
    off, adj = tools.synth_adjacency(n, seed=13, synth=tools.web_like(p_empty=0.3, mean_deg=3.0, local_gap=50.0, p_far=0.2))
    g = graph_of(W, tools, off, adj, threads=4)
    a, b = g.stats(indegrees=True), g.copy().stats(indegrees=True)
    for k in SM.SCALARS:
        assert getattr(a, k) == getattr(b, k), k
    assert a.log_delta == b.log_delta and np.array_equal(a.indegrees, b.indegrees)
    SM.assert_same(a, SM.model(off, adj))


def test_empty_graph(W, tools):
    st = tools.store([])
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    r = g.stats(indegrees=True)
    SM.assert_same(r, SM.model(*SM.csr([])))
    assert (r.nodes, r.min_outdegree, r.min_indegree) == (0, SM.INT64_MAX, SM.INT64_MAX)
    assert list(r.outdegree_distribution) == [0] and list(r.indegree_distribution) == [0] and len(r.indegrees) == 0


# 9. device buffers
def _body_device_buffers(W, tools, torch):
    n = 30000
    off, adj = tools.synth_adjacency(n, seed=17, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    want = np.bincount(adj, minlength=n).astype(np.int64)
    L = W.bvgraph._stats_fns()
    h = C.c_void_p()
    assert L.bvg_stats_compute(g._h, 1, C.byref(h)) == 0
    try:
        t = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        assert L.bvg_stats_indegrees_dev(h, 0, n, t.data_ptr()) == 0
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert np.array_equal(got[:n], want) and got[n] == -7
        t.fill_(-7)
        assert L.bvg_stats_indegrees_dev(h, 100, 357, t.data_ptr()) == 0
        torch.cuda.synchronize()
        got = t.cpu().numpy()
        assert np.array_equal(got[:257], want[100:357]) and (got[257:] == -7).all()
        assert L.bvg_stats_indegrees_dev(h, 0, n + 1, t.data_ptr()) == W.E_ARG
    finally:
        L.bvg_stats_close(h)


def _run_child(name):
    """torch-tensor tests run in a fresh child process that imports torch before the product library (torch's HIP runtime and the
    library's must be the same one: tests/test_gpu_device_buffers.py)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=560)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_device_buffers_match_host():
    _run_child("device_buffers")


# 10. the command line
def test_stats_main_on_cnr2000(W, cnr_model, tmp_path):
    base = str(tmp_path / "cnr")
    r = W.stats_main([GOLDEN_CNR, base])
    SM.assert_same(r, cnr_model, indegrees=False)
    assert open(base + ".stats", "rb").read() == SM.properties(cnr_model).encode()
    assert open(base + ".outdegree").read().split("\n") == [str(int(v)) for v in cnr_model["outdegree_distribution"]] + [""]
    assert open(base + ".indegree").read().split("\n") == [str(int(v)) for v in cnr_model["indegree_distribution"]] + [""]
    assert not os.path.exists(base + ".sccdistr") and not os.path.exists(base + ".indegrees")


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
