"""GPU: exact geometric centralities on the device (bvg_geometric; algo/LinearGeometricCentrality.java).

Every expected answer comes from the numpy model (tests/geometric_model.py).  reachable, the histogram and a table of integer coefficients
are compared exactly.  A float centrality must lie within one float32 spacing of exact(): the device sums at most n positive terms in
double, which is off by at most n 2^-52 relative, far below half a float ulp, so only the final rounding to float can differ, by at most
one ulp.  Against the reference's own order of additions (reference_order) the bound is reach 2^-24 value: half an ulp per float addition
of a growing positive sum."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import geometric_model as M
import sweep_cases
from test_gpu_components import ROUTES

GOLDEN_CNR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cnr-2000")

pytestmark = pytest.mark.gpu


def graph_of(W, tools, off, adj, params=None, threads=2):
    st = tools.store((off, adj), params, threads=threads) if params is not None else tools.store((off, adj), threads=threads)
    return W.BVGraph.from_memory(st.params, st.graph, st.offsets)


def is_integer_table(spec):
    return not isinstance(spec, (str, tuple)) and all(float(v) == int(v) for v in spec)


def check(g, counts, spec, sources=None, r=None):
    """One run against the model's counts of the same sources; returns the result."""
    if r is None:
        r = g.linear_geometric_centrality(spec, sources=sources, histogram=True)
    assert r.centrality.dtype == np.float32 and r.reachable.dtype == np.int64 and len(r.centrality) == len(r.reachable) == len(counts)
    assert np.array_equal(r.reachable, M.reachable(counts))
    assert np.array_equal(r.histogram, M.histogram(counts))
    expected = M.exact(counts, M.coefficient(spec))
    with np.errstate(all="ignore"):
        off_by = np.where(np.isinf(expected), 0, np.abs(r.centrality.astype(np.float64) - expected) / np.spacing(np.abs(expected)))
    print("largest difference from exact(), in float32 spacings:", float(np.max(off_by, initial=0.0)))
    if is_integer_table(spec):
        assert np.array_equal(r.centrality, expected)
    else:
        assert M.within_one_spacing(r.centrality, expected)
    return r


# 1. hand graphs, all sources, each kind of coefficients  /  2. the reference's order of additions
@pytest.mark.parametrize("name", sorted(M.HAND))
def test_hand_graphs(W, tools, name):
    n, arcs = M.HAND[name]
    off, adj = M.csr_of(n, arcs)
    g = graph_of(W, tools, off, adj)
    counts = M.distance_counts(off, adj, range(n))
    for cname, spec in sorted(M.COEFFS.items()):
        r = check(g, counts, spec)
        c = r.counters
        assert c["words_per_node"] == min(8, 1 << int(math.log2((n + 63) // 64))) and c["passes"] == -(-n // (64 * c["words_per_node"]))
        assert c["deepest_pass_levels"] == max(len(k) for k in counts) - 1 and c["sweeps"] >= c["deepest_pass_levels"] + 1
        assert c["single_resident_batch"] == (1 if len(adj) else 0) and c["batch_decodes"] == (1 if len(adj) else 0)
        coeff = M.coefficient(spec)
        value = M.exact_double(counts, coeff)
        for s in range(n):
            ref, reach = M.reference_order(off, adj, s, coeff)
            assert reach == r.reachable[s]
            if math.isinf(value[s]):
                assert math.isinf(float(ref)) and math.isinf(float(r.centrality[s])), (cname, s)
            else:
                assert abs(float(r.centrality[s]) - float(ref)) <= reach * 2.0 ** -24 * value[s], (cname, s, float(r.centrality[s]), float(ref))
    if name == "path_70":
        assert r.counters["deepest_pass_levels"] == 69 and r.counters["words_per_node"] == 2 and r.counters["passes"] == 1
    sod = g.linear_geometric_centrality(("power", 1))                          # closeness and Lin from the sums of the distances
    d = np.array([sum(i * int(k) for i, k in enumerate(c)) for c in counts], dtype=np.float64)
    assert sod.histogram is None and np.array_equal(sod.centrality, d.astype(np.float32))
    reach = M.reachable(counts).astype(np.float64)
    assert np.array_equal(sod.closeness(), np.where(d == 0, 0, 1 / np.where(d == 0, 1, d)).astype(np.float32))
    assert np.array_equal(sod.lin(), np.where(d == 0, 1, reach * reach / np.where(d == 0, 1, d)).astype(np.float32))


def test_empty_graph(W, tools):
    st = tools.store([])
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    for spec in M.COEFFS.values():
        r = g.linear_geometric_centrality(spec, histogram=True)
        assert len(r.centrality) == 0 and len(r.reachable) == 0 and len(r.histogram) == 0 and r.counters["passes"] == 0


def test_empty_range_writes_nothing(W, tools):
    off, adj = M.csr_of(*M.HAND["star"])
    g = graph_of(W, tools, off, adj)
    L = W.bvgraph._geometric_fns()
    cen = np.full(4, 7, dtype=np.float32); rea = np.full(4, 7, dtype=np.int64); hist = np.full(4, 7, dtype=np.uint64); hl = C.c_uint64(5)
    for at in (0, 4, 9):
        assert L.bvg_geometric(g._h, W.GEO_HARMONIC, 0.0, None, 0, at, at, cen.ctypes.data, rea.ctypes.data, hist.ctypes.data, 4, C.byref(hl), None) == 0
        assert (cen == 7).all() and (rea == 7).all() and (hist == 7).all() and hl.value == 0


# 3. neither the words per node nor the batch budget reaches the result
def test_words_and_budget_do_not_change_a_bit(W, tools, monkeypatch):
    n = 600                                                                    # more than 512 sources: two passes of eight words, the second partial
    rng = np.random.RandomState(11)
    lists = [sorted(set(int(y) for y in rng.randint(0, n, rng.poisson(2.0)))) for _ in range(n)]
    lists[17] = sorted(int(y) for y in rng.choice(n, 130, replace=False))      # longer than the small budget
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    counts = M.distance_counts_pull(off, adj, range(n))
    assert max(len(c) for c in counts) > 5 and len(set(M.reachable(counts).tolist())) > 10
    g = graph_of(W, tools, off, adj)
    spec = ("exp", 0.7)
    first = None
    for words in (1, 2, 4, 8):
        for budget in (None, "97"):
            monkeypatch.setenv("BVG_GEO_WORDS", str(words))
            if budget is None:
                monkeypatch.delenv("BVG_GEO_BATCH_ARCS", raising=False)
            else:
                monkeypatch.setenv("BVG_GEO_BATCH_ARCS", budget)
            r = g.linear_geometric_centrality(spec, histogram=True)
            c = r.counters
            assert c["words_per_node"] == words and c["passes"] == -(-n // (64 * words))
            if budget is None:
                assert c["single_resident_batch"] == 1 and c["batch_decodes"] == 1
            else:
                assert c["single_resident_batch"] == 0 and c["batch_decodes"] > c["sweeps"]
            if first is None:
                first = check(g, counts, spec, r=r)
            else:
                assert r.centrality.tobytes() == first.centrality.tobytes() and r.reachable.tobytes() == first.reachable.tobytes()
                assert r.histogram.tobytes() == first.histogram.tobytes()
    monkeypatch.delenv("BVG_GEO_WORDS")
    monkeypatch.delenv("BVG_GEO_BATCH_ARCS")
    r = g.linear_geometric_centrality(spec, histogram=True)                    # the default: 600 sources fill eight words
    assert r.counters["words_per_node"] == 8 and r.centrality.tobytes() == first.centrality.tobytes()


# 4. long runs of nodes without successors: node ranges the batch plan leaves out; the longest list exceeds the budget
@pytest.mark.parametrize("budget", ["1", "97"])
def test_empty_runs_under_tiny_budgets(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_GEO_BATCH_ARCS", budget)
    off, adj = sweep_cases.empty_runs_graph()
    assert np.diff(off.astype(np.int64)).max() > int(budget)
    sources = (180, 260)                                                       # across the end of an empty run and the boundary of the two words
    counts = M.distance_counts(off, adj, range(*sources))
    assert M.reachable(counts)[:20].tolist() == [1] * 20 and M.reachable(counts)[20:].max() > 100   # the first twenty sources have no successors
    g = graph_of(W, tools, off, adj)
    for spec in ("harmonic", [0, 1, 1]):
        r = check(g, counts, spec, sources=sources)
        assert r.counters["words_per_node"] == 2 and r.counters["passes"] == 1 and r.counters["batch_decodes"] > r.counters["sweeps"]


# 4b. lists and groups of 64 lists that end on, just past and across the edges of the mark kernel's chunks of 64 arcs
@pytest.mark.parametrize("budget", [None, "61"])
def test_chunk_edges_under_budgets(W, tools, monkeypatch, budget):
    if budget is None:
        monkeypatch.delenv("BVG_GEO_BATCH_ARCS", raising=False)
    else:
        monkeypatch.setenv("BVG_GEO_BATCH_ARCS", budget)
    off, adj = sweep_cases.chunk_edges_graph()
    counts = M.distance_counts(off, adj, range(sweep_cases.CHUNK_NODES))
    assert all(M.reachable(counts)[x] == sweep_cases.CHUNK_NODES for x in sweep_cases.CHUNK_LISTS)
    g = graph_of(W, tools, off, adj)
    for spec in ("harmonic", [0, 1, 1]):
        r = check(g, counts, spec)
        assert r.counters["single_resident_batch"] == (1 if budget is None else 0)
        assert r.counters["batch_decodes"] == 1 if budget is None else r.counters["batch_decodes"] > r.counters["sweeps"]


# 5. the golden graph
@pytest.fixture(scope="module")
def cnr_counts(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.int64); off[1:] = np.cumsum(deg)
    return M.distance_counts_pull(off, succ, range(1000, 1100))


def test_cnr2000(W, cnr_counts):
    g = W.BVGraph.load(GOLDEN_CNR)
    sources = (1000, 1100)
    assert M.reachable(cnr_counts).max() > 1000
    for h in (g, g.copy()):
        for spec in ("harmonic", [0, 1, 1]):
            r = check(h, cnr_counts, spec, sources=sources)
            c = r.counters
            print("cnr-2000 counters:", c)
            assert c["single_resident_batch"] == 1 and c["batch_decodes"] == 1   # one resident batch, decoded once
            assert c["words_per_node"] == 2 and c["passes"] == 1 and c["sweeps"] == c["deepest_pass_levels"] + 1 == len(r.histogram)
        within_two = np.array([int(k[1:3].sum()) for k in cnr_counts])
        assert np.array_equal(r.centrality, within_two.astype(np.float32))      # the nodes within two hops: exact integers
    with g.breadth_first_visit() as v:                                         # the reachable counts against visits that know nothing of the model
        for s in (1000, 1021, 1042, 1063, 1099):
            v.clear()
            assert v.visit(s) == r.reachable[s - 1000]


# 6. every decode route
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_synthetic_graph_every_route(W, tools, route):
    n = 20000
    off, adj = tools.synth_adjacency(n, seed=1, synth=tools.web_like(p_empty=0.5, mean_deg=4.0, local_gap=40.0))
    g = graph_of(W, tools, off, adj, threads=4)
    if ROUTES[route]:
        g.set_tuning(**ROUTES[route])
    sources = (5000, 5128)
    counts = M.distance_counts_pull(off, adj, range(*sources))
    assert M.reachable(counts).max() > 100
    r = check(g, counts, "harmonic", sources=sources)
    assert r.counters["words_per_node"] == 2 and r.counters["passes"] == 1


# 7. the contract
def test_successor_outside_the_graph_is_eof(W):
    from bvrecords import Record, assemble
    recs = [Record(d=2, residuals=[1, 2]), Record(d=1, residuals=[0]), Record(d=1, residuals=[9])]   # node 2 -> 9 in a 3-node graph
    gbytes, offs, _ = assemble(recs)
    p = W.default_params().clone(nodes=3, arcs=4)
    g = W.BVGraph.from_memory(p, np.frombuffer(gbytes, dtype=np.uint8), offs)
    with pytest.raises(W.EOFException):
        g.linear_geometric_centrality("harmonic")
    with pytest.raises(W.EOFException):                                        # g is usable: the same answer again (from 1 the arc 2 -> 9 is met at level 3)
        g.linear_geometric_centrality([0, 1, 1], sources=(1, 2), histogram=True)
    assert g.outdegree(2) == 1 and g.outdegree(0) == 2


def test_capacity_and_arguments(W, tools):
    n, arcs = M.HAND["path_70"]
    off, adj = M.csr_of(n, arcs)
    g = graph_of(W, tools, off, adj)
    counts = M.distance_counts(off, adj, range(10, 30))
    L = W.bvgraph._geometric_fns()
    cen = np.full(20, 7, dtype=np.float32); rea = np.full(20, 7, dtype=np.int64); hist = np.full(8, 7, dtype=np.uint64); hl = C.c_uint64(0); ctr = np.zeros(8, dtype=np.uint64)
    args = (cen.ctypes.data, rea.ctypes.data, hist.ctypes.data, 8, C.byref(hl), ctr.ctypes.data)
    assert L.bvg_geometric(g._h, W.GEO_HARMONIC, 0.0, None, 0, 10, 30, *args) == W.E_CAPACITY
    full = M.histogram(counts)
    assert hl.value == len(full) == 60 and np.array_equal(hist, full[:8])      # the length, and what fits
    assert np.array_equal(rea, M.reachable(counts)) and M.within_one_spacing(cen, M.exact(counts, M.coefficient("harmonic")))   # the other outputs all the same
    assert ctr[0] == 1 and ctr[3] == 1
    table = np.array([0.0, 1.0])
    for bad in ((4, 0.0, None, 0, 0, 4), (W.GEO_TABLE, 0.0, None, 2, 0, 4), (W.GEO_TABLE, 0.0, table.ctypes.data, 0, 0, 4), (W.GEO_HARMONIC, 0.0, None, 0, 3, 2),
                (W.GEO_HARMONIC, 0.0, None, 0, -1, 2), (W.GEO_HARMONIC, 0.0, None, 0, 0, 71), (W.GEO_HARMONIC, 0.0, None, 0, 71, 71)):
        assert L.bvg_geometric(g._h, *bad, *args) == W.E_ARG, bad
    assert L.bvg_geometric(g._h, W.GEO_HARMONIC, 0.0, None, 0, 0, 4, cen.ctypes.data, rea.ctypes.data, hist.ctypes.data, 8, None, None) == W.E_ARG   # hist without hist_len
    only = np.zeros(70, dtype=np.int64)                                        # either output may be NULL; g is usable after every refusal
    assert L.bvg_geometric(g._h, W.GEO_HARMONIC, 0.0, None, 0, 0, 70, None, only.ctypes.data, None, 0, None, None) == 0
    assert only.tolist() == list(range(70, 0, -1))
    with pytest.raises(W.IllegalArgumentException):
        g.linear_geometric_centrality("harmonic", sources=(5, 71))
    g.set_node_base(1000)
    with pytest.raises(W.IllegalArgumentException):
        g.linear_geometric_centrality("harmonic")


def test_command_line_writes_the_reference_files(W, tools, tmp_path):
    n, arcs = M.HAND["two_disjoint_cycles"]
    off, adj = M.csr_of(n, arcs)
    tools.store((off, adj)).write(str(tmp_path / "g"))
    cp, rp = str(tmp_path / "c.bin"), str(tmp_path / "r.bin")
    W.geometric_main(["-m", "-T", "4", str(tmp_path / "g"), "it.unimi.dsi.big.webgraph.algo.LinearGeometricCentrality$ExponentialCoefficients(0.5)", cp, rp])
    c, r = W.load_geometric(cp, rp)
    counts = M.distance_counts(off, adj, range(n))
    assert np.array_equal(r, M.reachable(counts)) and np.array_equal(c, M.exact(counts, M.coefficient(("exp", 0.5))))   # (powers of two: exact in float)


# device buffers (a child process that imports torch before the product library: tests/test_gpu_device_buffers.py)
def _body_device_buffers(W, tools, torch):
    n = 3000
    off, adj = tools.synth_adjacency(n, seed=17, synth=tools.web_like(p_empty=0.5, mean_deg=3.0))
    st = tools.store((off, adj), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    sources = (100, 300)
    counts = M.distance_counts_pull(off, adj, range(*sources))
    dc = torch.full((200,), -1.0, dtype=torch.float32, device="cuda"); dr = torch.full((200,), -1, dtype=torch.int64, device="cuda")
    hist, counters = g.linear_geometric_centrality_dev("harmonic", dc, dr, sources=sources, histogram=True)
    assert counters["passes"] == 1 and counters["words_per_node"] == 4               # 200 sources: four words hold them
    assert np.array_equal(hist, M.histogram(counts)) and np.array_equal(dr.cpu().numpy(), M.reachable(counts))
    assert M.within_one_spacing(dc.cpu().numpy(), M.exact(counts, M.coefficient("harmonic")))
    host = g.linear_geometric_centrality("harmonic", sources=sources)
    assert host.centrality.tobytes() == dc.cpu().numpy().tobytes()
    dr.fill_(-1)
    assert g.linear_geometric_centrality_dev([0, 1, 1], None, dr, sources=sources)[0] is None          # either buffer may be left out
    assert np.array_equal(dr.cpu().numpy(), M.reachable(counts))
    try:
        g.linear_geometric_centrality_dev("harmonic", torch.empty(199, dtype=torch.float32, device="cuda"), None, sources=sources)
        raise AssertionError("no IllegalArgumentException for a short buffer")
    except W.IllegalArgumentException:
        pass


def test_device_buffers_match_host():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "device_buffers"], capture_output=True, text=True, timeout=560)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


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
