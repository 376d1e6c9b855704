"""GPU: HyperBall on the device (bvg_hyperball_*; algo/HyperBall.java, standard iterations).

Every expected answer comes from the numpy model (tests/hyperball_model.py), which restates the algorithm and the library's hash and is
itself checked against exact breadth-first search (tests/test_hyperball_model.py).  Registers and modified() are compared exactly;
counts to relative 2^-40 (the sum of 2^-register is exact to a few roundings of 2^-53 on both sides, the margin covers the device's log);
terms of the neighbourhood function to relative n 2^-52 (the bound on reordering a sum of n positive doubles); the float32 centralities to
relative iterations 2^-22 (one float rounding per iteration plus the count's error)."""
import ctypes as C
import os

import numpy as np
import pytest

import hyperball_model as M
import sweep_cases
from conftest import CNR

pytestmark = pytest.mark.gpu


def open_graph(W, tools, off, adj, params=None, **tuning):
    st = tools.store((off, adj), params, threads=2)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    if tuning:
        g.set_tuning(**tuning)
    return g


def close_rel(got, want, rel, what):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want)
    bound = rel * np.abs(want)
    worst = float(np.max(err / np.maximum(np.abs(want), 1e-300))) if len(want) else 0.0
    print("%s: worst relative error %.3g (bound %.3g)" % (what, worst, rel))
    assert np.all(err <= bound), "%s: worst relative error %g > %g" % (what, worst, rel)


def check_state(hb, model, n, its, centralities):
    assert np.array_equal(hb.registers(), model.regs)
    assert hb.modified() == model.modified and hb.iteration == model.iteration
    close_rel(hb.counts(), model.counts(), 2.0 ** -40, "counts")
    close_rel(hb.neighbourhood_function, model.nf, max(n, 1) * 2.0 ** -52, "neighbourhood function")
    if centralities:
        rel = max(its, 1) * 2.0 ** -22
        close_rel(hb.sum_of_distances(), model.sod, rel, "sum of distances")
        close_rel(hb.harmonic_centrality(), model.sid, rel, "harmonic")
        close_rel(hb.closeness(), model.closeness(), rel, "closeness")
        close_rel(hb.lin(), model.lin(), rel, "lin")
        close_rel(hb.nieminen(), model.nieminen(), rel, "nieminen")
        close_rel(hb.reachable(), model.reachable(), rel, "reachable")


def lockstep(g, off, adj, log2m, seed=0, centralities=True, max_iterations=None):
    """init and every iteration up to stabilisation (or max_iterations) on the device and in the model, compared after each step."""
    n = len(off) - 1
    model = M.HyperBallModel(off, adj, log2m, seed=seed, sum_of_distances=centralities, harmonic=centralities)
    with g.hyperball(log2m, seed=seed, sum_of_distances=centralities, harmonic=centralities) as hb:
        hb.init(seed); model.init(seed)
        check_state(hb, model, n, 0, centralities)
        its = 0
        while max_iterations is None or its < max_iterations:
            hb.iterate(); model.iterate(); its += 1
            check_state(hb, model, n, its, centralities)
            if model.modified == 0:
                break
            assert its <= n + 1
    return model


SMALL = {
    "clique": lambda: M.clique(100),
    "cycle": lambda: M.cycle(120),
    "line": lambda: M.line(150),
    "out_tree": lambda: M.out_tree(255),
    "random": lambda: M.random_graph(300, 3.0, 2026),
}


# 1. the small graphs of the model's own test
@pytest.mark.parametrize("log2m", [4, 5, 6, 8])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_graphs_in_lockstep(W, tools, name, log2m):
    off, adj = M.adjacency(SMALL[name]())
    g = open_graph(W, tools, off, adj)
    lockstep(g, off, adj, log2m, seed=log2m)


# 2. every counter size (a counter on 1 .. 64 lanes, 1 .. 4 pieces per lane), lists short and long
def awkward_graph(n=3000, seed=9):
    """Self-loops, isolated nodes, a lone self-loop, long duplicate-free lists (whole-wavefront walks), a long list that holds its own node."""
    rng = np.random.RandomState(seed)
    lists = [sorted(set(int(y) for y in rng.randint(0, n, rng.poisson(2.0)))) for _ in range(n)]
    for x in range(0, n, 7):
        lists[x] = sorted(set(lists[x] + [x]))                                # self-loops
    for x in range(3, n, 11):
        lists[x] = []                                                          # isolated (as sources)
    lists[5] = [5]
    lists[100] = [y for y in range(n) if y % 3 != 1]                           # two thirds of the nodes; 100 % 3 == 1: not its own
    lists[101] = [y for y in range(n) if y % 2]                                # half of the nodes, 101 among them
    a = 2 * n // 3
    lists[a] = list(range(n // 3, n // 3 + 300))                               # 300 arcs
    lists[a + 1] = list(range(0, 255))                                         # just below the whole-wavefront threshold
    lists[a + 2] = list(range(0, 256))                                         # just at it
    return lists


@pytest.mark.parametrize("log2m", range(4, 13))
def test_every_counter_size(W, tools, log2m):
    off, adj = M.adjacency(awkward_graph())
    g = open_graph(W, tools, off, adj)
    model = lockstep(g, off, adj, log2m, seed=1, max_iterations=None if log2m <= 8 else 4)
    assert model.iteration >= 2


# 3. every coding the encoder writes, tiny batches, 64-bit decode
PARAMS = [dict(), dict(window_size=0, max_ref_count=0), dict(min_interval_length=0), dict(outdegree_coding=1, block_coding=1, residual_coding=1, reference_coding=1, block_count_coding=1),
          dict(residual_coding=2, reference_coding=2, block_count_coding=5, block_coding=5), dict(residual_coding=7, window_size=20, min_interval_length=2),
          dict(residual_coding=3, zeta_k=2), dict(zeta_k=1, max_ref_count=-1)]


@pytest.mark.parametrize("params", PARAMS, ids=[",".join("%s=%s" % kv for kv in sorted(p.items())) or "default" for p in PARAMS])
def test_every_coding(W, tools, params):
    off, adj = tools.synth_adjacency(5000, seed=4, synth=tools.web_like(p_empty=0.2, mean_deg=5.0, local_gap=40.0, p_far=0.2))
    g = open_graph(W, tools, off, adj, W.default_params(**params))
    lockstep(g, off, adj, 5, seed=2, centralities=False, max_iterations=6)


@pytest.mark.parametrize("budget", ["1", "97"])
def test_tiny_batches(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_HB_BATCH_ARCS", budget)
    off, adj = M.adjacency(awkward_graph(600, seed=3) if budget == "1" else awkward_graph(2500, seed=4))
    assert np.diff(off.astype(np.int64)).max() > int(budget)                   # a list that is a batch of its own
    g = open_graph(W, tools, off, adj)
    lockstep(g, off, adj, 6, seed=5, max_iterations=5)


# long runs of nodes without successors at the start, in the middle and at the end: node ranges the batch plan leaves out, whose counters
# are carried over and counted all the same
@pytest.mark.parametrize("budget", ["1", "97"])
def test_empty_runs_under_tiny_batches(W, tools, monkeypatch, budget):
    monkeypatch.setenv("BVG_HB_BATCH_ARCS", budget)
    off, adj = sweep_cases.empty_runs_graph()
    assert np.diff(off.astype(np.int64)).max() > int(budget)                   # the longest list exceeds the budget
    g = open_graph(W, tools, off, adj)
    lockstep(g, off, adj, 5, max_iterations=4)


@pytest.mark.parametrize("tuning", [dict(force_wide=True), dict(force_slow=True), dict(no_index=1)], ids=["force_wide", "force_slow", "no_index"])
def test_decode_routes(W, tools, tuning):
    off, adj = tools.synth_adjacency(6000, seed=3, synth=tools.eu_like(p_empty=0.3, mean_deg=30.0))
    g = open_graph(W, tools, off, adj, **tuning)
    lockstep(g, off, adj, 4, seed=7, max_iterations=8)


# 4. the golden graph
@pytest.fixture(scope="module")
def cnr(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.uint64); off[1:] = np.cumsum(deg)
    return off, np.asarray(succ, dtype=np.int64)


@pytest.mark.parametrize("log2m,bound", [(4, None), (6, None), (8, 6)])
def test_cnr2000(W, cnr, log2m, bound):
    off, adj = cnr
    n = len(off) - 1
    g = W.BVGraph.load(CNR)
    model = M.HyperBallModel(off, adj, log2m, seed=0, sum_of_distances=True, harmonic=True)
    model.init()
    with g.hyperball(log2m, seed=0, sum_of_distances=True, harmonic=True) as hb:
        hb.init(0)
        assert np.array_equal(hb.registers(), model.regs)
        its = 0
        while bound is None or its < bound:
            hb.iterate(); model.iterate(); its += 1
            assert hb.modified() == model.modified, "iteration %d" % its
            for a in range(0, n, 1 << 16):                                      # (registers in slices: the from / to arguments)
                b = min(n, a + (1 << 16))
                assert np.array_equal(hb.registers(a, b), model.regs[a:b]), "iteration %d, nodes [%d, %d)" % (its, a, b)
            if model.modified == 0:
                break
        print("cnr-2000, log2m %d: %d iterations, neighbourhood function ends at %.6g" % (log2m, its, model.nf[-1]))
        check_state(hb, model, n, its, True)
        assert hb.count(12345) == hb.counts(12345, 12346)[0]
        r = g.scan()                                                           # the caller's handle stays usable while the object is open
        assert r["arcs"] == len(adj) and r["nodes"] == n


# 5. determinism and the stopping rules
def test_two_runs_are_bit_identical(W, tools):
    off, adj = tools.synth_adjacency(20000, seed=8, synth=tools.web_like(p_empty=0.2, mean_deg=6.0, local_gap=60.0, p_far=0.1))
    g = open_graph(W, tools, off, adj)
    got = []
    for _ in range(2):
        with g.hyperball(7, seed=11, sum_of_distances=True, harmonic=True) as hb:
            hb.run()
            got.append((hb.neighbourhood_function.tobytes(), hb.sum_of_distances().tobytes(), hb.harmonic_centrality().tobytes(), hb.counts().tobytes(), hb.registers().tobytes()))
    assert got[0] == got[1]
    with g.hyperball(7, seed=11, sum_of_distances=True, harmonic=True) as hb:   # and run() twice on one object
        hb.run(); a = hb.neighbourhood_function.tobytes()
        hb.run(); assert hb.neighbourhood_function.tobytes() == a
        hb.init(12); hb.iterate()
        assert hb.neighbourhood_function.tobytes() != a[:16]                    # another seed: other counters


@pytest.mark.parametrize("upper_bound,threshold", [(-1, -1.0), (-1, 0.001), (3, -1.0), (10 ** 9, 0.5)])
def test_run_stops_where_the_model_stops(W, tools, upper_bound, threshold):
    off, adj = tools.synth_adjacency(8000, seed=12, synth=tools.web_like(p_empty=0.2, mean_deg=5.0, local_gap=30.0, p_far=0.05))
    g = open_graph(W, tools, off, adj)
    model = M.HyperBallModel(off, adj, 6, seed=3)
    model.run(upper_bound, threshold)
    with g.hyperball(6, seed=3) as hb:
        hb.run(upper_bound, threshold)
        assert hb.iteration == model.iteration and hb.modified() == model.modified
        assert np.array_equal(hb.registers(), model.regs)
        close_rel(hb.neighbourhood_function, model.nf, 8000 * 2.0 ** -52, "neighbourhood function")
        close_rel([hb.relative_increment], [model.relative_increment], 8000 * 2.0 ** -51, "relative increment")
    if upper_bound == 3:
        assert model.iteration == 2 and model.modified > 0
    if threshold == 0.001:
        assert model.modified > 0 and model.iteration >= 4                      # stopped by the increment, not by stabilisation
    if (upper_bound, threshold) == (-1, -1.0):
        assert model.modified == 0


# 6. states and errors
def test_state_errors(W, tools):
    off, adj = tools.synth_adjacency(1000, seed=1)
    g = open_graph(W, tools, off, adj)
    L = W.bvgraph._hyperball_fns()
    with g.hyperball(5) as hb:
        with pytest.raises(W.IllegalStateException):
            hb.iterate()                                                       # before init
        with pytest.raises(W.IllegalStateException):
            hb.registers()
        hb.init(0)
        hb.iterate()
        for get in (hb.sum_of_distances, hb.harmonic_centrality, hb.closeness, hb.lin, hb.nieminen):
            with pytest.raises(W.IllegalStateException):
                get()                                                          # not enabled
        assert len(hb.reachable()) == 1000
        nf = np.zeros(1)
        assert L.bvg_hyperball_neighbourhood_function(hb._h, nf.ctypes.data, 1) == W.E_CAPACITY
        for frm, to in ((-1, 5), (5, 4), (0, 1001)):
            with pytest.raises(W.IllegalArgumentException):
                hb.registers(frm, to)
            with pytest.raises(W.IllegalArgumentException):
                hb.counts(frm, to)
        assert L.bvg_hyperball_centrality(hb._h, 6, nf.ctypes.data) == W.E_ARG
    with g.hyperball(5, harmonic=True) as hb:
        hb.run(2)
        assert len(hb.harmonic_centrality()) == 1000
        with pytest.raises(W.IllegalStateException):
            hb.closeness()
    for bad in (3, 0, -1):
        with pytest.raises(W.IllegalArgumentException):
            g.hyperball(bad)
    with pytest.raises(W.UnsupportedOperationException):
        g.hyperball(13)
    h = C.c_void_p()
    assert L.bvg_hyperball_create(g._h, 5, 4, 0, C.byref(h)) == W.E_ARG         # unknown flag bits
    g.set_node_base(1000)
    with pytest.raises(W.IllegalArgumentException):
        g.hyperball(5)


def test_empty_and_one_node_graphs(W, tools):
    st = tools.store([])
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    with g.hyperball(4) as hb:
        hb.run()
        assert hb.neighbourhood_function.tolist() == [0.0] and hb.modified() == 0 and hb.registers().shape == (0, 16)
    for lists in ([[]], [[0]]):
        off, adj = M.adjacency(lists)
        g = open_graph(W, tools, off, adj)
        lockstep(g, off, adj, 4)


def test_successor_outside_the_graph_is_eof(W):
    from bvrecords import Record, assemble
    recs = [Record(d=1, residuals=[1]), Record(d=1, residuals=[0]), Record(d=1, residuals=[9])]   # 0 <-> 1, and node 2 -> 9 in a 3-node graph
    gbytes, offs, _ = assemble(recs)
    p = W.default_params().clone(nodes=3, arcs=3)
    g = W.BVGraph.from_memory(p, np.frombuffer(gbytes, dtype=np.uint8), offs)
    with g.hyperball(4, seed=1) as hb:
        hb.init(1)
        before = hb.registers()
        with pytest.raises(W.EOFException):
            hb.iterate()
        with pytest.raises(W.IllegalStateException):
            hb.iterate()                                                       # half an iteration behind it: init first
        hb.init(1)                                                             # usable again
        assert np.array_equal(hb.registers(), before) and hb.iteration == -1 and hb.neighbourhood_function.tolist() == [3.0]
        with pytest.raises(W.EOFException):
            hb.run()


# 7. the command line
def test_cli_files_equal_the_api(W, tmp_path):
    out = {k: str(tmp_path / k) for k in ("nf", "sod", "harmonic", "closeness", "lin", "nieminen", "reachable")}
    nf = W.hyperball_main(["-l", "5", "-S", "4", "-u", "6", "-n", out["nf"], "-d", out["sod"], "-h", out["harmonic"], "-c", out["closeness"], "-L", out["lin"],
                           "-N", out["nieminen"], "-r", out["reachable"], CNR])
    g = W.BVGraph.load(CNR)
    with g.hyperball(5, seed=4, sum_of_distances=True, harmonic=True) as hb:
        hb.run(6)
        assert hb.iteration == 5
        assert np.array_equal(nf, hb.neighbourhood_function)
        lines = open(out["nf"]).read().split("\n")
        assert lines[-1] == "" and not any("e" in l.lower() for l in lines)     # plain decimals
        assert np.array_equal(np.array([float(l) for l in lines[:-1]]), hb.neighbourhood_function)
        for k, get in (("sod", hb.sum_of_distances), ("harmonic", hb.harmonic_centrality), ("closeness", hb.closeness), ("lin", hb.lin), ("nieminen", hb.nieminen),
                       ("reachable", hb.reachable)):
            assert os.path.getsize(out[k]) == 4 * g.num_nodes()
            assert np.array_equal(W.load_floats(out[k]), get()), k
        raw = np.fromfile(out["reachable"], dtype=np.uint8)[:4]
        assert np.array_equal(raw, np.frombuffer(np.array([hb.reachable()[0]], dtype=">f4").tobytes(), dtype=np.uint8))   # big-endian
