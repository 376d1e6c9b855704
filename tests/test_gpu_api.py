"""GPU: the host-side mirror of the reference API (ImmutableGraph / NodeIterator / LazyLongIterator)
and the auxiliary C-ABI entry points, checked against the oracle.  Follows WebGraphTestCase.assertGraph
(test/it/unimi/dsi/big/webgraph/WebGraphTestCase.java:106-199)."""
import numpy as np
import pytest

from conftest import CNR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(W, tools, oracle):
    st = tools.synth_store(5000, seed=2, chunk_nodes=1024, threads=2)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    deg, succ = og.decode_range(0, 5000)
    cum = np.concatenate([[0], np.cumsum(deg)])
    lists = [succ[cum[i]:cum[i + 1]] for i in range(5000)]
    return g, og, lists, st


def test_assert_graph_contract(W, small):
    g, og, lists, st = small
    n = g.num_nodes()
    it = g.node_iterator()
    with pytest.raises(W.IllegalStateException):
        it.outdegree()                                                      # BVGraph.java:1207
    arcs = 0
    for x in range(n):
        assert it.has_next()
        assert it.next_long() == x
        d = it.outdegree()
        assert d == len(lists[x])
        assert np.array_equal(it.successor_array(), lists[x])
        li = it.successors()
        assert [li.next_long() for _ in range(d)] == lists[x].tolist()
        assert li.next_long() == -1 and li.next_long() == -1               # WebGraphTestCase.java:125
        arcs += d
    assert not it.has_next()
    with pytest.raises(W.NoSuchElementException):
        it.next_long()                                                      # BVGraph.java:1165
    assert arcs == g.num_arcs()                                             # WebGraphTestCase.java:140


@pytest.mark.parametrize("start", [0, 1, 6, 7, 8, 63, 64, 65, 1023, 1024, 1025, 4999, 5000])
def test_node_iterator_from_every_kind_of_start(small, start):
    """WebGraphTestCase.java:151-180: nodeIterator(s) agrees with random access for all later nodes."""
    g, og, lists, st = small
    it = g.node_iterator(start)
    for x in range(start, min(start + 200, g.num_nodes())):
        assert it.next_long() == x
        assert np.array_equal(it.successor_array(), lists[x])
        assert g.outdegree(x) == len(lists[x])
    if start == g.num_nodes():
        assert not it.has_next()


def test_copy_and_split_node_iterators(small):
    g, og, lists, st = small
    it = g.node_iterator(10)
    it.next_long(); it.next_long()
    c = it.copy(40)                                                         # NodeIterator.copy(upperBound), BVGraph.java:1223-1229
    seen = [x for x in c]
    assert seen == list(range(12, 40))
    parts = g.split_node_iterators(3)                                       # ImmutableGraph.java:405-436
    got = []
    for p in parts:
        for x in p:
            got.append(x)
            assert np.array_equal(p.successor_array(), lists[x])
    assert got == list(range(g.num_nodes()))
    g2 = g.copy()                                                           # flyweight, BVGraph.java:553-578
    assert np.array_equal(g2.successor_array(77), lists[77])


def test_errors_map_to_reference_exceptions(W, small):
    g, og, lists, st = small
    n = g.num_nodes()
    for bad in (-1, n):
        with pytest.raises(W.IllegalArgumentException):
            g.outdegree(bad)                                                # BVGraph.java:823
        with pytest.raises(W.IllegalArgumentException):
            g.successors(bad)                                               # BVGraph.java:863
    with pytest.raises(W.IllegalArgumentException):
        g.node_iterator(n + 1)                                              # BVGraph.java:1128
    with pytest.raises(W.IllegalArgumentException):
        g.decode_range(5, 4)
    with pytest.raises(W.UnsupportedOperationException):
        W.BVGraph.from_memory(W.default_params(nodes=1, outdegree_coding=W.ZETA), b"\x80", np.array([0, 1], dtype=np.uint64))   # BVG:658
    with pytest.raises(W.EOFException):
        W.BVGraph.from_memory(W.default_params(nodes=3), b"\x80", None)    # offsets derived from the stream: it ends after 1 node


@pytest.mark.parametrize("wide", [False, True])
def test_offsets_index_packed_and_plain(W, tools, oracle, monkeypatch, wide):
    """The index lives in HBM packed (32-bit distance per node + a 64-bit base per 1 024 nodes); BVG_WIDE_OFFSETS=1 keeps the plain
    array (also the fall-back when a distance does not fit).  Both give back the offsets they were given and decode the same."""
    if wide: monkeypatch.setenv("BVG_WIDE_OFFSETS", "1")
    st = tools.synth_store(7000, seed=12, chunk_nodes=1024, threads=2)          # > 6 groups of 1 024 nodes, the last one partial
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    assert np.array_equal(g.offsets(), st.offsets)
    r, o = g.scan(), og.scan()
    assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"])
    for a, b in [(1023, 1025), (2047, 2049), (6999, 7000), (0, 7000)]:          # ranges across the group boundaries
        ra, oa = g.scan(a, b), og.scan(a, b)
        assert (ra["arcs"], ra["chk"], ra["graph_bytes"]) == (oa["arcs"], oa["chk"], (int(st.offsets[b]) + 7) // 8 - int(st.offsets[a]) // 8), (a, b)
    deg, succ = g.decode_range(1000, 3100)
    odeg, osucc = og.decode_range(1000, 3100)
    assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc)
    t = g.tile(3)                                                               # tiling writes the packed form directly
    assert np.array_equal(t.offsets(), np.concatenate([st.offsets[:-1] + k * st.offsets[-1] for k in range(3)] + [[3 * st.offsets[-1]]]).astype(np.uint64))
    assert t.scan()["arcs"] == 3 * o["arcs"]
    t.close(); g.close()


def test_offsets_and_outdegrees_by_products(small):
    g, og, lists, st = small
    assert np.array_equal(g.offsets(), st.offsets)
    assert np.array_equal(g.outdegrees(), np.array([len(l) for l in lists], dtype=np.int32))
    b = g.split_by_bits(4)
    assert b[0] == 0 and b[-1] == g.num_nodes() and all(b[i] <= b[i + 1] for i in range(4))
    bits = np.diff(st.offsets[b].astype(np.int64))
    assert bits.max() - bits.min() < int(st.offsets[-1]) // 4 // 4 + 20000     # roughly equal compressed size
    # arc-balanced split points: exactly the skipTo() targets over the cumulative outdegrees (HyperBall.java:748-768)
    cum = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    for k in (1, 3, 7):
        ba = g.split_by_arcs(k)
        per = (int(cum[-1]) + k - 1) // k
        want = [0] + [int(np.searchsorted(cum, j * per, side="left")) for j in range(1, k)] + [g.num_nodes()]
        want = [min(w, g.num_nodes()) for w in want]
        assert ba.tolist() == want, (k, ba.tolist(), want)


def test_tile_is_a_translated_concatenation(W, small, oracle):
    """bvg_tile: K copies of the stream are the graph shifted by j*n (translation invariance)."""
    g, og, lists, st = small
    n = g.num_nodes()
    t = g.tile(3)
    assert t.num_nodes() == 3 * n and t.num_arcs() == 3 * g.num_arcs()
    deg, succ = t.decode_range(n - 5, 2 * n + 5)
    exp = [lists[x] for x in range(n - 5, n)] + [l + n for l in lists] + [lists[x] + 2 * n for x in range(5)]
    assert deg.tolist() == [len(l) for l in exp]
    assert np.array_equal(succ, np.concatenate(exp))
    r = t.scan()
    want_chk = sum(og.scan(0, n, node_base=j * n)["chk"] for j in range(3)) % (1 << 64)
    assert r["arcs"] == 3 * g.num_arcs() and r["chk"] == want_chk
    # node_base: the shard semantics used by bench.py --gpus N
    g.set_node_base(7 * n)
    assert g.scan()["chk"] == og.scan(0, n, node_base=7 * n)["chk"]
    d2, s2 = g.decode_range(10, 20)
    assert np.array_equal(s2, np.concatenate([lists[x] for x in range(10, 20)]) + 7 * n)
    g.set_node_base(0)


def test_scan_subranges_add_up(small):
    g, og, lists, st = small
    whole = g.scan()
    parts = [g.scan(a, b) for a, b in [(0, 1), (1, 777), (777, 778), (778, 4096), (4096, 5000)]]
    assert sum(p["arcs"] for p in parts) == whole["arcs"]
    assert sum(p["chk"] for p in parts) % (1 << 64) == whole["chk"]
    for (a, b), p in zip([(0, 1), (1, 777)], parts):
        o = og.scan(a, b)
        assert (p["arcs"], p["chk"], p["nodes"]) == (o["arcs"], o["chk"], o["nodes"])


def test_corrupt_streams_fail_cleanly(W, small):
    """A damaged .graph must end in an error status or a (wrong) result — never a hang or a fault."""
    g, og, lists, st = small
    rng = np.random.default_rng(5)
    for trial in range(6):
        bad = st.graph.copy()
        for pos in rng.integers(0, len(bad), 40):
            bad[pos] ^= 1 << int(rng.integers(0, 8))
        h = W.BVGraph.from_memory(st.params, bad, st.offsets)
        try:
            h.scan()
        except (W.EOFException, W.IllegalStateException):
            pass
        h.close()
    # offsets that disagree with the stream are detected (SURVEY A.6 self-check)
    off = st.offsets.copy(); off[100:200] += 3
    h = W.BVGraph.from_memory(st.params, st.graph, off)
    with pytest.raises((W.EOFException, W.IllegalStateException)):
        h.scan()


def test_giant_node_takes_the_slow_path_and_stays_exact(W, tools, oracle):
    """A list far larger than the LDS pool (cf. BVGraphSlowTest's 2^30-outdegree node, scaled down)."""
    rng = np.random.default_rng(9)
    big = np.unique(rng.integers(0, 3_000_000, 150_000))
    lists = [[1, 2], big.tolist(), big[::2].tolist(), [5], list(range(100, 70_000)), []] + [[i, i + 1] for i in range(6, 200)]
    st = tools.store(lists, W.default_params())
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    deg, succ = g.decode_range(0, len(lists))
    assert deg.tolist() == [len(l) for l in lists]
    assert np.array_equal(succ, np.concatenate([np.asarray(l, dtype=np.int64) for l in lists if len(l)]))
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    r, o = g.scan(), og.scan()
    assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"]) and r["slow_blocks"] >= 1


def test_wide_ids_beyond_32_bits(W, tools, oracle):
    """Successor ids above 2^32 (the 'big' in webgraph-big): the 64-bit kernels are selected by node count."""
    n = 3000
    off, adj = tools.synth_adjacency(n, seed=4, chunk_nodes=1024)
    st = tools.store((off, adj), W.default_params(), chunk_nodes=1024)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    base = (1 << 33) + 12345
    g.set_node_base(base)
    deg, succ = g.decode_range(0, n)
    assert np.array_equal(succ, adj + base)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    assert g.scan()["chk"] == og.scan(0, n, node_base=base)["chk"]
    g.set_tuning(force_wide=True)
    assert g.scan()["chk"] == og.scan(0, n, node_base=base)["chk"]


def test_device_index_is_saved_and_loaded_back(W, tools, oracle, tmp_path, capfd, monkeypatch):
    """basename.bvgidx (bvg_save_index): the block plan and the residual skip index of one process are what the next one scans with --
    no index-building passes, the same lean blocks, the same checksum (cf. the cached offsets big list of BVGraph.java:1545-1555); a
    file that is older than the graph, or belongs to another graph, is ignored / refused."""
    import os, time
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_EMIT", "1")
    st = tools.synth_store(30000, seed=8, synth=tools.eu_like(mean_deg=70.0), threads=4)
    base = str(tmp_path / "g"); st.write(base)
    og = oracle.Graph.load(base); o = og.scan()
    g = W.BVGraph.load(base)
    r1 = g.scan(); r1 = g.scan()
    assert (r1["arcs"], r1["chk"]) == (o["arcs"], o["chk"]) and r1["index_entries"] > 0 and r1["lean_blocks"] > 0
    assert g.save_index() == base + ".bvgidx" and os.path.getsize(base + ".bvgidx") > 6 * r1["index_entries"]
    g.close()
    capfd.readouterr()
    h = W.BVGraph.load(base)                                            # picks the file up
    r2 = h.scan()
    err = capfd.readouterr().err
    assert "index loaded from" in err and "residual skip index: blocks" not in err, err
    assert (r2["arcs"], r2["chk"], r2["index_entries"], r2["lean_blocks"]) == (r1["arcs"], r1["chk"], r1["index_entries"], r1["lean_blocks"])
    d1, s1 = h.decode_range(100, 5000); d0, s0 = og.decode_range(100, 5000)
    assert np.array_equal(d1, d0) and np.array_equal(s1, s0)
    h.close()
    # an index of another graph is refused; one older than the graph is not even tried
    st2 = tools.synth_store(30000, seed=9, synth=tools.eu_like(mean_deg=70.0), threads=4)
    base2 = str(tmp_path / "h"); st2.write(base2)
    q = W.BVGraph.load(base2)
    with pytest.raises(W.IOException):
        q.load_index(base + ".bvgidx")
    assert q.scan()["arcs"] == st2.stats["arcs"]
    q.close()
    t = time.time() + 100
    os.utime(base + ".graph", (t, t))
    capfd.readouterr()
    h = W.BVGraph.load(base)
    assert h.scan()["chk"] == o["chk"] and "index loaded from" not in capfd.readouterr().err
    h.close()


def test_a_handle_without_index_neither_builds_nor_reads_one(W, tools, oracle, monkeypatch, capfd):
    """bvg_tuning.no_index (ABI 3): what bench.py times as `value_no_index`.  A flyweight with it scans index-less -- index_entries 0, no lean blocks, no
    index-building pass -- next to a handle that builds and uses the index; both equal the oracle, and the flyweight does not disturb the shared index."""
    monkeypatch.setenv("BVG_DEBUG", "1")
    st = tools.synth_store(40000, seed=31, synth=tools.eu_like(mean_deg=60.0), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    o = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets).scan()
    h = g.copy(); h.set_tuning(no_index=True)
    capfd.readouterr()
    for _ in range(2):
        r = h.scan()
        assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"]) and r["index_entries"] == 0 and r["lean_blocks"] == 0
    assert "residual skip index" not in capfd.readouterr().err, "the index-less handle built an index"
    r1 = g.scan()                                                       # the first scan of the other handle IS the index build (its validating pass reports the result)
    r2 = g.scan()
    assert (r1["arcs"], r1["chk"]) == (o["arcs"], o["chk"]) == (r2["arcs"], r2["chk"])
    assert r1["index_entries"] == r2["index_entries"] > 0 and r2["lean_blocks"] > 0 and r1["lean_blocks"] == 0
    assert capfd.readouterr().err.count("residual skip index: blocks") == 1
    r = h.scan()                                                        # still index-less, although the index now exists in the shared graph
    assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"]) and r["index_entries"] == 0 and r["lean_blocks"] == 0
    h.close(); g.close()


def test_work_order_and_giant_work_areas_do_not_change_results(W, tools, oracle, monkeypatch):
    """Round 4's launch-level changes against their round-3 forms: the XCD-aware work order (BVG_XCDS=1: plain order) and the giants' shared work-area slots
    (BVG_GBATCH=<n>: batched launches with one area per block) -- same {nodes, arcs, chk}, same lists."""
    st = tools.synth_store(15000, seed=33, synth=tools.eu_like(max_deg=30000, tail_alpha=1.6, mean_deg=40.0), threads=4)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    o = og.scan(); odeg, osucc = og.decode_range(0, 15000)
    for env in ({}, {"BVG_XCDS": "1"}, {"BVG_GBATCH": "7"}, {"BVG_XCDS": "3", "BVG_GBATCH": "1"}):
        for k in ("BVG_XCDS", "BVG_GBATCH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
        for _ in range(3):
            r = g.scan()
            assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"]), env
        deg, succ = g.decode_range(0, 15000)
        assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc), env
        g.close()


@pytest.mark.parametrize("shape", ["eu", "heavy_tail", "w0", "gamma_residuals"])
def test_dense_walk_builds_the_same_index_as_the_one_pass_build(W, tools, oracle, tmp_path, monkeypatch, shape):
    """Round 4 fills the skip entries by a dense walk (csrc/bvg_index.hip: one lane per long list, every coding) and validates the blocks in a pass
    that decodes WITH those entries and checks each of them against the stream; round 3 walked, filled and validated in one index-less pass of the
    row kernel (BVG_INDEX_WALK=0).  Both must leave the same index, byte for byte (entries, marks, plan: the payload of basename.bvgidx), and the same scans."""
    import os
    kw, synth, n = {}, tools.eu_like(mean_deg=70.0), 50000
    if shape == "heavy_tail": synth, n = tools.eu_like(max_deg=30000, tail_alpha=1.6, mean_deg=40.0), 20000
    if shape == "w0": synth, kw = tools.web_like(mean_deg=40.0), dict(window_size=0, max_ref_count=0, min_interval_length=0)
    if shape == "gamma_residuals": kw = dict(residual_coding=W.GAMMA, zeta_k=3)
    st = tools.synth_store(n, seed=23, params=W.default_params(**kw), synth=synth, threads=4)
    base = str(tmp_path / "g"); st.write(base)
    o = oracle.Graph.load(base).scan()
    files = {}
    for mode in ("0", None):
        if mode is None: monkeypatch.delenv("BVG_INDEX_WALK", raising=False)
        else: monkeypatch.setenv("BVG_INDEX_WALK", mode)
        g = W.BVGraph.load(base)
        g.build_index()
        r = g.scan(); r = g.scan()
        assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"]) and r["index_entries"] > 0, (shape, mode)
        p = str(tmp_path / ("idx_%s" % mode)); g.save_index(p); g.close()
        files[mode] = (open(p, "rb").read(), r["lean_blocks"], r["index_entries"])
    assert files["0"][1:] == files[None][1:], (files["0"][1:], files[None][1:])
    assert files["0"][0] == files[None][0], "the two builds left different index files"


@pytest.mark.parametrize("shape", ["dense", "sparse", "w0"])
def test_the_skip_index_granularity_is_a_property_of_the_index(W, tools, oracle, tmp_path, monkeypatch, shape):
    """Round 4 chooses the granularity of the residual skip index per graph (csrc/bvg_api.hip skip_granularity: one entry per 8 residuals from lists of 8 on
    for graphs with references below 40 arcs per node, per 16 from 16 on otherwise; rounds 1-3: per 16 from 24 on); the kernels take it from the index they
    are handed, and basename.bvgidx carries it.  Every granularity
    must give the oracle's scan and materialise (first scan = the build, second = the lean kernel on validated blocks); an index saved under one
    granularity must load and work in a process that would have chosen another; finer granularities hold more entries."""
    synth, n, kw = tools.eu_like(mean_deg=70.0), 40000, {}
    if shape == "sparse": synth, n = tools.web_like(mean_deg=11.0), 150000
    if shape == "w0": synth, n, kw = tools.web_like(mean_deg=30.0), 60000, dict(window_size=0, max_ref_count=0, min_interval_length=0)
    st = tools.synth_store(n, seed=29, params=W.default_params(**kw), synth=synth, threads=4)
    base = str(tmp_path / "g"); st.write(base)
    og = oracle.Graph.load(base); o = og.scan()
    entries, saved = {}, None
    for gran in (None, "24,16", "16,16", "8,8", "4,4", "9,2", "40,64"):
        if gran is None: monkeypatch.delenv("BVG_SKIP_GRAN", raising=False)
        else: monkeypatch.setenv("BVG_SKIP_GRAN", gran)
        g = W.BVGraph.load(base)
        for _ in range(2):
            r = g.scan()
            assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"]), (shape, gran)
        assert r["lean_blocks"] > 0, (shape, gran)
        a, b = n // 3, n // 3 + 5000
        deg, succ = g.decode_range(a, b)
        odeg, osucc = og.decode_range(a, b)
        assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc), (shape, gran)
        entries[gran] = r["index_entries"]
        if gran == "4,4": saved = g.save_index(str(tmp_path / "idx44"))
        g.close()
    assert entries["4,4"] > entries["8,8"] > entries["16,16"] > entries["24,16"] > entries["40,64"], entries
    assert entries[None] == (entries["8,8"] if shape == "sparse" else entries["16,16"]), (shape, entries)       # the per-graph choice
    monkeypatch.setenv("BVG_SKIP_GRAN", "24,16")                              # this process would build 24 / 16: the file's 4 / 4 entries are used as they are
    g = W.BVGraph.load(base)
    g.load_index(saved)
    r = g.scan()
    assert (r["arcs"], r["chk"], r["index_entries"]) == (o["arcs"], o["chk"], entries["4,4"]) and r["lean_blocks"] > 0
    g.close()


def test_a_damaged_or_foreign_index_file_is_refused(W, tools, oracle, tmp_path):
    """The lean scan kernel trusts the validation marks of basename.bvgidx, so the file is tied to EVERY byte of the stream and guarded
    by a checksum of its own payload (format 2): a .graph rewritten in place with the same size and other bytes in the middle, a
    flipped bit anywhere in the index, a mark turned from 'unvalidated' into 'validated', a halo beyond the kernels' limit, a truncated
    file -- each is refused (IOException) and the graph still scans right, on an index it builds itself."""
    import os
    st = tools.synth_store(40000, seed=18, synth=tools.eu_like(mean_deg=60.0), threads=4)
    base = str(tmp_path / "g"); st.write(base)
    o = oracle.Graph.load(base).scan()
    g = W.BVGraph.load(base)
    g.scan(); r = g.scan()
    assert r["chk"] == o["chk"] and r["lean_blocks"] > 0
    idx = g.save_index(); g.close()
    good = open(idx, "rb").read()

    def refused(data):
        open(idx, "wb").write(data)
        os.utime(idx, None)
        q = W.BVGraph.load(base)                                        # bvg_open tries the file by itself: a refusal must be silent and harmless
        try:
            with pytest.raises(W.IOException):
                q.load_index(idx)
            rr = q.scan(); rr = q.scan()
            assert (rr["arcs"], rr["chk"]) == (o["arcs"], o["chk"])
        finally:
            q.close()

    hdr = 128                                                           # sizeof(IndexHeader)
    assert len(good) > hdr + 4096
    for pos in (hdr + 3, len(good) // 2, len(good) - 5):                # a flipped bit in the plan, in the skip entries, in the values
        bad = bytearray(good); bad[pos] ^= 0x10
        refused(bytes(bad))
    refused(good[:-8])                                                  # truncated
    refused(good + b"\0" * 8)                                          # trailing bytes
    bad = bytearray(good); bad[8] ^= 1                                  # format version
    refused(bytes(bad))
    # the same index against a stream whose MIDDLE bytes changed (same size, same first and last 64 KiB): not this index's graph
    open(idx, "wb").write(good)
    gbytes = bytearray(open(base + ".graph", "rb").read())
    assert len(gbytes) > 3 * 65536
    mid = len(gbytes) // 2
    gbytes[mid] ^= 0x01
    base2 = str(tmp_path / "g2")
    for ext in (".properties", ".offsets"):
        open(base2 + ext, "wb").write(open(base + ext, "rb").read())
    open(base2 + ".graph", "wb").write(bytes(gbytes))
    q = W.BVGraph.load(base2)
    with pytest.raises(W.IOException):
        q.load_index(idx)
    q.close()
    # and the untouched file still loads
    q = W.BVGraph.load(base)
    q.load_index(idx)
    rr = q.scan()
    assert (rr["arcs"], rr["chk"], rr["lean_blocks"]) == (o["arcs"], o["chk"], r["lean_blocks"])
    q.close()


def test_successors_as_32_bit_ids_for_the_host_path(W, small, oracle):
    """bvg_decode_range32: the same lists as bvg_decode_range, ids as uint32 (what the NodeIterator mirror moves over PCIe and widens,
    NodeIterator.java:80-96); refused when an id could pass 2^32."""
    g, og, lists, st = small
    n = g.num_nodes()
    deg, succ = g.decode_range(0, n)
    d32, s32 = g.decode_range32(0, n)
    assert s32.dtype == np.uint32 and np.array_equal(d32, deg) and np.array_equal(s32.astype(np.int64), succ)
    d32, s32 = g.decode_range32(n // 3, n // 2)
    od, os_ = og.decode_range(n // 3, n // 2)
    assert np.array_equal(d32, od) and np.array_equal(s32, os_)
    h = g.copy()
    top = (1 << 32) - 1 - n                                             # the largest base that still fits: every id stays BELOW 0xFFFFFFFF, which stands for -1
    h.set_node_base(top)
    _, s32 = h.decode_range32(0, 100)
    assert np.array_equal(s32.astype(np.int64), og.decode_range(0, 100)[1] + top) and int(s32.max()) < 0xFFFFFFFF
    h.set_node_base(top + 1)
    with pytest.raises(W.UnsupportedOperationException):
        h.decode_range32(0, 100)
    it = W.NodeIterator(h, 0, batch_nodes=512)                          # beyond it the iterator moves int64
    it.next_long()
    assert it.successor_array().dtype == np.int64 and np.array_equal(it.successor_array(), og.successors(0) + (top + 1))
    it.close(); h.close()
    it = W.NodeIterator(g, 5, batch_nodes=300)                          # below: uint32 batches, widened per node
    x = it.next_long()
    assert it.batch()[3].dtype == np.uint32 and it.successor_array().dtype == np.int64 and np.array_equal(it.successor_array(), og.successors(x))
    it.close()


def test_mosaic_is_the_cycle_of_its_bases(W, tools, oracle):
    """bvg_mosaic: the streams of several DIFFERENT graphs back to back, the cycle repeated (the bench's workload): equals the host
    twin tools.mosaic_host bit for bit, decodes to the bases' lists shifted by their first node, checksums add up."""
    sts = [tools.synth_store(n, seed=sd, synth=sy, threads=2) for n, sd, sy in
           ((3000, 1, tools.eu_like(mean_deg=40.0)), (1777, 2, tools.web_like()), (4097, 3, tools.eu_like(mean_deg=90.0, p_copy=0.8)))]
    gs = [W.BVGraph.from_memory(st.params, st.graph, st.offsets) for st in sts]
    cycles = 3
    m = W.mosaic(gs, cycles)
    host = tools.mosaic_host(sts, cycles)
    assert m.num_nodes() == host.params.nodes and np.array_equal(m.offsets(), host.offsets)
    deg, succ = m.decode_range(0, m.num_nodes())
    og = oracle.Graph.from_memory(oracle.Params(**host.params.as_dict()), host.graph.tobytes(), host.offsets)
    odeg, osucc = og.decode_range(0, host.params.nodes)
    assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc)
    chk = arcs = 0; first = 0
    for c in range(cycles):
        for st in sts:
            o = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets).scan(0, st.params.nodes, node_base=first)
            r = m.scan(first, first + st.params.nodes)
            assert (r["arcs"], r["chk"]) == (o["arcs"], o["chk"]), (c, first)
            chk = (chk + o["chk"]) % (1 << 64); arcs += o["arcs"]; first += st.params.nodes
    r = m.scan()
    assert (r["arcs"], r["chk"]) == (arcs, chk)
    with pytest.raises(W.IllegalArgumentException):                    # bases must share the BV parameters
        st2 = tools.synth_store(500, seed=9, params=W.default_params(window_size=3), threads=1)
        W.mosaic([gs[0], W.BVGraph.from_memory(st2.params, st2.graph, st2.offsets)], 1)
    m.close()


def test_full_size_properties_on_a_tiled_graph(W, tools, oracle):
    """Size-independent properties at bench scale (a ~0.5 GiB tiled stream, hundreds of millions of arcs):
    (1) the checksum of K tiles equals the sum of K base scans with shifted node bases (translation
    invariance + additivity), (2) arcs = K x base arcs, (3) node-range shards add up to the whole,
    (4) sampled ranges deep inside the tiled graph materialise bit-exactly against the oracle."""
    n = 1 << 17
    st = tools.synth_store(n, seed=13, threads=8)
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    K = max(2, (512 << 20) // max(len(st.graph), 1))
    big = base.tile(K)
    assert big.num_nodes() == K * n
    whole = big.scan()
    assert whole["arcs"] == K * st.stats["arcs"] and whole["nodes"] == K * n
    want = 0
    for j in (0, 1, K // 2, K - 1):
        base.set_node_base(j * n)
        r = base.scan()
        part = big.scan(j * n, (j + 1) * n)
        assert (part["arcs"], part["chk"]) == (r["arcs"], r["chk"])
    base.set_node_base(0)
    b = big.split_by_bits(5)
    parts = [big.scan(int(b[i]), int(b[i + 1])) for i in range(5)]
    assert sum(p["arcs"] for p in parts) == whole["arcs"]
    assert sum(p["chk"] for p in parts) % (1 << 64) == whole["chk"]
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    for j, lo, hi in ((K - 1, 1000, 1300), (K // 3, n - 200, n), (1, 0, 150)):
        deg, succ = big.decode_range(j * n + lo, j * n + hi)
        odeg, osucc = og.decode_range(lo, hi)
        assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc + j * n)
    # the oracle agrees with tile 0 as a whole
    assert big.scan(0, n)["chk"] == og.scan()["chk"]


def test_successors_batch_random_access(W, small, cnr_golden):
    """Frontier-style random access: arbitrary order, repeats, chain heads and tails."""
    g, og, lists, st = small
    rng = np.random.default_rng(3)
    nodes = np.concatenate([rng.integers(0, g.num_nodes(), 3000), [0, 0, g.num_nodes() - 1, 7, 6, 5, 4, 3, 2, 1]])
    deg, succ = g.successors_batch(nodes)
    assert deg.tolist() == [len(lists[x]) for x in nodes]
    exp = [lists[x] for x in nodes if len(lists[x])]
    assert np.array_equal(succ, np.concatenate(exp))
    with pytest.raises(W.IllegalArgumentException):
        g.successors_batch([0, g.num_nodes()])
    d0, s0 = g.successors_batch([])
    assert len(d0) == 0 and len(s0) == 0
    c = W.BVGraph.load(CNR)
    nodes = rng.integers(0, c.num_nodes(), 20000)
    deg, succ = c.successors_batch(nodes)
    assert np.array_equal(succ, np.concatenate([cnr_golden[x] for x in nodes]))
    assert deg.tolist() == [len(cnr_golden[x]) for x in nodes]


def test_offsets_are_derived_when_absent(W, tools, oracle, tmp_path, cnr_csr):
    """loadSequential / loadOffline need no .offsets (BVGraph.java:1345-1464); BVGraph -O (writeOffsets, :2595-2609):
    the device derives the index from the stream; it must equal the encoder's / the fixture's offsets."""
    g = W.BVGraph.from_memory(W.parse_properties(open(CNR + ".properties").read()), open(CNR + ".graph", "rb").read(), None)
    assert np.array_equal(g.offsets(), oracle.Graph.load(CNR).offsets())
    deg, succ = g.decode_range(0, 5000)
    assert np.array_equal(deg, cnr_csr[0][:5000]) and np.array_equal(succ, cnr_csr[1][:int(cnr_csr[0][:5000].sum())])
    for kw in (dict(), dict(window_size=0, max_ref_count=0, min_interval_length=0), dict(residual_coding=1, outdegree_coding=1, reference_coding=2, block_count_coding=5, block_coding=1),
               dict(residual_coding=7), dict(zeta_k=5, min_interval_length=2)):
        st = tools.synth_store(6000, seed=17, params=W.default_params(**kw), chunk_nodes=1024, threads=2)
        h = W.BVGraph.from_memory(st.params, st.graph, None)
        assert np.array_equal(h.offsets(), st.offsets), kw
    base = str(tmp_path / "g")
    st.write(base)
    import os
    os.remove(base + ".offsets")
    with pytest.raises(W.IOException):
        W.BVGraph.load(base)                                                # the standard load needs the file
    q = W.BVGraph.load_sequential(base)
    assert np.array_equal(q.offsets(), st.offsets)
    q2 = W.BVGraph.load_offline(base)
    assert q2.scan()["arcs"] == st.stats["arcs"]


def test_offsets_are_derived_by_the_chunk_parallel_walk(W, tools, capfd, monkeypatch):
    """BVGraph -O (writeOffsets, BVGraph.java:2595-2609) by the chunk-parallel walk of csrc/bvg_derive.hip (the default since round 3):
    speculative walks, one code per lane and step, iterated to the one consistent walk.  It must reproduce the encoder's offsets
    exactly -- on a stream of thousands of chunks, without references, with other codings, with a window of 100, across a record
    of 300 000 residuals (dozens of chunks that cannot fall into step by themselves) -- in far fewer rounds than there are chunks."""
    monkeypatch.setenv("BVG_DEBUG", "1")
    st = tools.synth_store(1 << 18, seed=3, synth=tools.eu_like(), threads=8)
    big = tools.tile_host(st, 6)
    capfd.readouterr()
    g = W.BVGraph.from_memory(big.params, big.graph, None)
    err = capfd.readouterr().err
    assert "parallel walk ok" in err, err
    rounds = int(err.split("parallel walk ok (")[1].split(" rounds")[0])
    assert 2 <= rounds <= 1500, err                                          # (7 660 chunks: far fewer rounds than chunks)
    assert np.array_equal(g.offsets(), big.offsets)
    assert g.scan()["arcs"] == big.stats["arcs"]
    g.close()
    for kw in (dict(window_size=0, max_ref_count=0, min_interval_length=0), dict(residual_coding=1, outdegree_coding=1, reference_coding=2, block_count_coding=5, block_coding=1),
               dict(residual_coding=7), dict(window_size=100, max_ref_count=20), dict(zeta_k=1, min_interval_length=2)):      # (Golomb residuals of a web graph are codes of thousands of bits: no walk derives those)
        s2 = tools.synth_store(200000, seed=5, params=W.default_params(**kw), threads=4)
        capfd.readouterr()
        h = W.BVGraph.from_memory(s2.params, s2.graph, None)
        assert "parallel walk ok" in capfd.readouterr().err, kw               # (per parameter set: a silent fall-back to the sequential walk is a failure)
        assert np.array_equal(h.offsets(), s2.offsets), kw
        h.close()
    # one giant record in the middle of ordinary ones
    rng = np.random.default_rng(2)
    n = 400000
    lens = rng.integers(0, 9, n)
    lo = np.maximum(np.arange(n) - 40, 0)
    lists = [np.unique(lo[x] + rng.integers(0, 80, lens[x])) for x in range(n)]
    lists = [l[l < n] for l in lists]
    lists[2500] = np.unique(rng.integers(0, n, 600000))[:300000]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    s3 = tools.store((off, np.concatenate(lists).astype(np.int64)), W.default_params(), threads=4)
    assert int(np.diff(s3.offsets.astype(np.int64)).max()) > 10 * 32768       # the record spans more than ten chunks
    capfd.readouterr()
    h = W.BVGraph.from_memory(s3.params, s3.graph, None)
    assert "parallel walk ok" in capfd.readouterr().err
    assert np.array_equal(h.offsets(), s3.offsets)
    h.close()
    # a window beyond the ring of the parallel walk takes the sequential one
    s4 = tools.synth_store(3000, seed=6, params=W.default_params(window_size=200, max_ref_count=3), threads=2)
    capfd.readouterr()
    h = W.BVGraph.from_memory(s4.params, s4.graph, None)
    assert "not used" in capfd.readouterr().err and np.array_equal(h.offsets(), s4.offsets)
    h.close()
    # a truncated stream is still reported, not derived wrongly
    cut = st.graph[:len(st.graph) // 2].copy()
    with pytest.raises((W.EOFException, W.IllegalStateException)):
        W.BVGraph.from_memory(st.params, cut, None)


def test_offsets_are_derived_across_a_record_of_hundreds_of_chunks(W, tools, capfd, monkeypatch):
    """A hub with millions of residuals (what bvg_giant.hip exists for) spans hundreds of 4 KiB chunks of the bare stream; inside it the parallel walk of
    csrc/bvg_derive.hip settles exactly one chunk per round -- the crawl, not a stall: the derivation must finish on the parallel walk (round 4 gave up after
    256 such rounds and restarted the one-wavefront walk from bit 0) and reproduce the encoder's offsets."""
    monkeypatch.setenv("BVG_DEBUG", "1")
    rng = np.random.default_rng(11)
    n = 1 << 25
    hub = np.unique(rng.integers(0, n, 3300000)).astype(np.int64)
    few = np.sort(rng.choice(n, 20000, replace=False))                          # some ordinary records around it
    deg = np.zeros(n, dtype=np.int64); deg[few] = 3; deg[n // 3] = len(hub)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    succ = np.empty(int(off[-1]), dtype=np.int64)
    for x in few:
        if x != n // 3:
            succ[int(off[x]):int(off[x + 1])] = np.minimum(x + np.array([1, 5, 9]), n - 1)
    succ[int(off[n // 3]):int(off[n // 3 + 1])] = hub
    st = tools.store((off, succ), W.default_params(), threads=8)
    assert int(np.diff(st.offsets.astype(np.int64)).max()) > 520 * 32768         # the hub's record: more chunks than round 4's give-up rule allowed rounds
    capfd.readouterr()
    g = W.BVGraph.from_memory(st.params, st.graph, None)
    err = capfd.readouterr().err
    assert "parallel walk ok" in err and "giving up" not in err, err[-2000:]
    assert np.array_equal(g.offsets(), st.offsets)
    g.close()


def _cpu_transpose(n, deg, succ):
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    order = np.argsort(succ, kind="stable")                       # stable: sources stay increasing inside every target
    toff = np.concatenate([[0], np.cumsum(np.bincount(succ, minlength=n))]).astype(np.uint64)
    return toff, src[order]


def test_transpose_feed_matches_cpu_transpose(W, tools, oracle, small):
    """decode + device sort = Transform.transposeOffline's batches (Transform.java:1058-1160)."""
    g, og, lists, st = small
    n = g.num_nodes()
    deg, succ = og.decode_range(0, n)
    toff, tsucc = g.transpose()
    ctoff, ctsucc = _cpu_transpose(n, deg, succ)
    assert np.array_equal(toff, ctoff) and np.array_equal(tsucc, ctsucc)
    # transposing twice gives the graph back (TransformTest's involution check)
    t = tools.store((toff.astype(np.int64), tsucc), W.default_params())
    gt = W.BVGraph.from_memory(t.params, t.graph, t.offsets)
    toff2, tsucc2 = gt.transpose()
    assert np.array_equal(toff2, np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)) and np.array_equal(tsucc2, succ)
    gt.close()
    # degenerate inputs and the shard restriction
    for ls in ([], [[]], [[0]], [[1], [0]], [[] for _ in range(70)]):
        s2 = tools.store(ls, W.default_params())
        g2 = W.BVGraph.from_memory(s2.params, s2.graph, s2.offsets)
        to, ts = g2.transpose()
        d2 = np.array([len(l) for l in ls], dtype=np.int64); a2 = np.array([v for l in ls for v in l], dtype=np.int64)
        cto, cts = _cpu_transpose(len(ls), d2, a2) if len(ls) else (np.zeros(1, np.uint64), np.zeros(0, np.int64))
        assert np.array_equal(to, cto) and np.array_equal(ts, cts), ls
        g2.close()
    g.set_node_base(5)
    with pytest.raises(W.IllegalArgumentException):
        g.transpose()
    g.set_node_base(0)


def _cpu_symmetrize(n, deg, succ):
    """union(g, transpose(g)) (Transform.java:573-575) with numpy: the distinct pairs of both directions, source-major."""
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    keys = np.unique(np.concatenate([src * n + succ, succ * n + src])) if len(succ) else np.zeros(0, np.int64)
    s, t = keys // max(n, 1), keys % max(n, 1)
    soff = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))]).astype(np.uint64) if n else np.zeros(1, np.uint64)
    return soff, t.astype(np.int64)


def test_symmetrize_matches_cpu_union(W, tools, oracle, small):
    """Transform.symmetrizeOffline (Transform.java:546-575): the graph united with its transpose, on the device."""
    g, og, lists, st = small
    n = g.num_nodes()
    deg, succ = og.decode_range(0, n)
    soff, ssucc = g.symmetrize()
    csoff, cssucc = _cpu_symmetrize(n, deg, succ)
    assert np.array_equal(soff, csoff) and np.array_equal(ssucc, cssucc)
    # the result is its own transpose and symmetrising again changes nothing (TransformTest's checks on symmetrize)
    s2 = tools.store((soff.astype(np.int64), ssucc), W.default_params())
    g2 = W.BVGraph.from_memory(s2.params, s2.graph, s2.offsets)
    toff, tsucc = g2.transpose()
    assert np.array_equal(toff, soff) and np.array_equal(tsucc, ssucc)
    soff2, ssucc2 = g2.symmetrize()
    assert np.array_equal(soff2, soff) and np.array_equal(ssucc2, ssucc)
    g2.close()
    for ls in ([], [[]], [[0]], [[1], [0]], [[1], []], [[] for _ in range(70)], [[0, 1, 2], [2], [0]]):
        s3 = tools.store(ls, W.default_params())
        g3 = W.BVGraph.from_memory(s3.params, s3.graph, s3.offsets)
        so, ss = g3.symmetrize()
        d3 = np.array([len(l) for l in ls], dtype=np.int64); a3 = np.array([v for l in ls for v in l], dtype=np.int64)
        cso, css = _cpu_symmetrize(len(ls), d3, a3)
        assert np.array_equal(so, cso) and np.array_equal(ss, css), ls
        g3.close()
    import ctypes as C
    need = C.c_uint64()
    so = np.empty(n + 1, dtype=np.uint64)
    assert W.lib().bvg_symmetrize(g._h, so.ctypes.data, None, 0, C.byref(need)) == W.E_CAPACITY and need.value == len(cssucc)
    assert np.array_equal(so, csoff)                                           # the offsets come with the size query


def test_random_access_down_a_long_reference_chain(W, tools, oracle):
    """maxrefcount x window > 64: the chain of successors(x) reaches further back than a request block's halo holds (BVG:1084 recurses as
    deep as it goes).  Such requests leave the batch and are decoded through the block plan; found by tests/test_gpu_fuzz.py."""
    n = 400
    base = [n - 3, n - 2, n - 1]
    lists = [sorted(set(base + [x % 7, (x * 3) % 11 + 20])) for x in range(n)]          # every list copies most of the one before
    p = W.default_params(window_size=1, max_ref_count=1000)
    st = tools.store(lists, p)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    nodes = np.array([n - 1, 200, 0, 65, 66, n - 1], dtype=np.int64)
    deg, succ = g.successors_batch(nodes)
    assert deg.tolist() == [len(lists[x]) for x in nodes]
    assert succ.tolist() == [v for x in nodes for v in lists[x]]
    g.close()
