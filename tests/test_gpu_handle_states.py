"""Handles of one graph in different modes, taking turns.  The block plans, the residual skip index and its validation marks belong to the
graph and are shared by every bvg_copy() flyweight; the tuning (no_index 0 / 1 / 2, force_wide, block_bits), the node base and what a handle
learned about its blocks belong to the handle.  A stale mark, a stale learned split or a snapshot swapped under a handle would show as a
wrong list here.

1. A seeded random state machine: 2-4 handles on one graph, 20-40 operations (tuning, node base, scans, materialising calls, the node
   iterator, index build / save / load, copy / close), every result against the oracle or the CSR adjacency.
   BVG_STATE_FUZZ=<cases> (default 12), BVG_STATE_SEED=<seed> (default 1), BVG_STATE_FROM=<case>: every case draws from its own
   generator (seed, case), so one case replays alone.
2. Index provenance, pinned: the index a graph has is the one its first builder made; a handle of another mode or width that scans outside
   it widens it in its own form or leaves it alone, never replaces it (include/bvgraph_hip.h, bvg_tuning.no_index)."""
import os
import threading

import numpy as np
import pytest

from bvrecords import Record, assemble
from test_gpu_fuzz import _adjacency

pytestmark = pytest.mark.gpu

BASES = (0, 0xFFFFF000, (1 << 33) + 7, (1 << 40) + 1)          # test_gpu_modes.py::test_wide_ids_and_node_base
BLOCK_BITS = (0, 16384, 65536)


class _Case:
    """One graph: its bytes, the oracle, the CSR adjacency (from the oracle; equal to the generator's where there is one)."""

    def __init__(self, W, oracle, name, params, graph, offsets):
        self.W, self.name, self.params = W, name, params
        self.graph = np.ascontiguousarray(graph, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.og = oracle.Graph.from_memory(oracle.Params(**params.as_dict()), self.graph.tobytes(), self.offsets)
        self.n = int(params.nodes)
        self.deg, self.adj = self.og.decode_range(0, self.n)
        self.deg = np.asarray(self.deg, dtype=np.int32)
        self.cum = np.concatenate([[0], np.cumsum(self.deg, dtype=np.int64)])

    def open(self):
        return self.W.BVGraph.from_memory(self.params, self.graph, self.offsets)

    def lists(self, a, b, base):
        s = self.adj[self.cum[a]:self.cum[b]]
        return self.deg[a:b], np.where(s < 0, -1, s + base)                   # (a list that came out short is padded with -1, whatever the base)

    def scan(self, a, b, base):
        return self.og.scan(a, b, node_base=base, threads=4)


_GRAPHS = {}


def _fuzz_case(W, tools, oracle, rng):
    n = int(rng.choice([5000, 20000, 60000]))
    kw = dict(window_size=int(rng.choice([0, 1, 3, 7, 20, 70])), max_ref_count=int(rng.choice([0, 1, 3, 50, -1])),
              min_interval_length=int(rng.choice([0, 2, 4, 7])), zeta_k=int(rng.choice([1, 2, 3, 5])))
    if rng.random() < 0.3:
        kw.update(outdegree_coding=int(rng.choice([1, 2])), block_coding=int(rng.choice([1, 2, 5])), residual_coding=int(rng.choice([1, 2, 3, 6, 7])),
                  reference_coding=int(rng.choice([1, 2, 5])), block_count_coding=int(rng.choice([1, 2, 5])))
        if kw["residual_coding"] == 3:
            kw["zeta_k"] = int(rng.choice([1, 3, 5, 8]))
    off, adj = _adjacency(rng, n)
    st = tools.store((off, adj), W.default_params(**kw), threads=4)
    c = _Case(W, oracle, "fuzz n=%d %s" % (n, kw), st.params, st.graph, st.offsets)
    assert np.array_equal(c.deg, np.diff(off.astype(np.int64))) and np.array_equal(c.adj, adj), c.name
    return c


def _odd_case(W, tools, oracle):
    """test_malformed_streams.py::test_many_odd_nodes_among_ordinary_ones at 12 000 nodes: copy streams that overlap their residuals, every 97th node of
    every other run of 1 500 nodes, among ordinary records.  Their blocks fail validation and must never reach the lean kernel; the blocks of the clean
    runs are marked and take it."""
    if "odd" not in _GRAPHS:
        n = 12000
        st = tools.synth_store(n, seed=5, synth=tools.web_like(), threads=4)
        og0 = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
        deg0, succ0 = og0.decode_range(0, n)
        cum = np.concatenate([[0], np.cumsum(deg0)])
        recs, prev = [], None
        for x in range(n):
            l = succ0[cum[x]:cum[x + 1]].tolist()
            if x % 97 == 50 and (x // 1500) % 2 == 0 and recs and recs[-1].d >= 4:
                recs.append(Record(d=5, ref=1, blocks=[3], residuals=[prev[1], prev[2] + 1 if prev[2] + 1 not in prev else prev[-1] + 7]))
                prev = None
            else:
                recs.append(Record(d=len(l), residuals=l))
                prev = l
        g, offs, lists = assemble(recs)
        p = W.default_params().clone(nodes=n, arcs=int(sum(r.d for r in recs)))
        c = _Case(W, oracle, "odd blocks", p, np.frombuffer(g, dtype=np.uint8), offs)
        assert c.adj.tolist() == [v for l in lists for v in l]
        _GRAPHS["odd"] = c
    return _GRAPHS["odd"]


def _cnr_case(W, oracle):
    if "cnr" not in _GRAPHS:
        from conftest import CNR
        p = W.parse_properties(open(CNR + ".properties").read())
        off = W.decode_offsets(open(CNR + ".offsets", "rb").read(), p.nodes, p.offset_coding)
        _GRAPHS["cnr"] = _Case(W, oracle, "cnr-2000", p, np.fromfile(CNR + ".graph", dtype=np.uint8), off)
    return _GRAPHS["cnr"]


def _check_scan(c, r, a, b, base, what):
    o = c.scan(a, b, base)
    assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"]), what


def _run_case(W, tools, oracle, rng, case, log, tmp):
    kind = ("fuzz", "fuzz", "fuzz", "fuzz", "odd", "cnr")[case % 6]
    c = _fuzz_case(W, tools, oracle, rng) if kind == "fuzz" else (_odd_case(W, tools, oracle) if kind == "odd" else _cnr_case(W, oracle))
    n = c.n
    log.append("graph: %s" % c.name)
    first = c.open()
    hs = [[first, 0, dict(no_index=0, force_wide=False, block_bits=0)]]       # [handle, node base, tuning]
    for _ in range(int(rng.integers(1, 4))):
        hs.append([first.copy(), 0, dict(hs[0][2])])
    log.append("open + %d copies" % (len(hs) - 1))

    def rand_range(long):
        if long and n >= 4096:
            ln = int(rng.integers(4096, n + 1))
        else:
            ln = int(rng.integers(0, min(n, 4095) + 1))
        a = int(rng.integers(0, n - ln + 1))
        return a, a + ln

    try:
        for step in range(int(rng.integers(20, 41))):
            i = int(rng.integers(0, len(hs)))
            h, base, tun = hs[i]
            op = str(rng.choice(["tuning", "base", "scan", "scan", "scan", "decode", "decode", "decode32", "batch", "iter", "build", "save_load", "copy", "close"]))
            what = "case %d step %d: handle %d (base %#x, %s) %s" % (case, step, i, base, tun, op)
            if op == "tuning":
                tun = dict(no_index=int(rng.integers(0, 3)), force_wide=bool(rng.random() < 0.3), block_bits=int(rng.choice(BLOCK_BITS)))
                h.set_tuning(**tun); hs[i][2] = tun
                log.append(what + " -> %s" % tun)
            elif op == "base":
                base = int(rng.choice(BASES)); h.set_node_base(base); hs[i][1] = base
                log.append(what + " -> %#x" % base)
            elif op == "scan":
                a, b = rand_range(rng.random() < 0.6)
                log.append(what + " [%d, %d)" % (a, b))
                r = h.scan(a, b)
                _check_scan(c, r, a, b, base, what)
                if tun["no_index"] == 1:
                    assert r["index_entries"] == 0 and r["lean_blocks"] == 0, (what, r)
            elif op in ("decode", "decode32"):
                big = rng.random() < 0.5
                if big:
                    ln = int(rng.integers(n // 4, n + 1))
                else:
                    ln = int(rng.integers(0, max(n // 4, 1)))
                a = int(rng.integers(0, n - ln + 1)); b = a + ln
                log.append(what + " [%d, %d)" % (a, b))
                wd, ws = c.lists(a, b, base)
                if op == "decode32" and n + base > 0xFFFFFFFF:
                    with pytest.raises(W.UnsupportedOperationException):
                        h.decode_range32(a, b)
                    continue
                deg, succ = h.decode_range32(a, b) if op == "decode32" else h.decode_range(a, b)
                if op == "decode32":
                    succ = np.where(succ == 0xFFFFFFFF, -1, succ.astype(np.int64))   # (the -1 of a short list crosses as 0xFFFFFFFF)
                assert np.array_equal(deg, wd), what
                assert np.array_equal(succ, ws), what
            elif op == "batch":
                nodes = rng.integers(0, n, int(rng.integers(1, 200))).astype(np.int64)
                log.append(what + " %d nodes" % len(nodes))
                deg, succ = h.successors_batch(nodes)
                assert np.array_equal(deg, c.deg[nodes]), what
                assert np.array_equal(succ, np.concatenate([c.lists(x, x + 1, base)[1] for x in nodes])), what
            elif op == "iter":
                s = int(rng.integers(0, n))
                log.append(what + " from %d" % s)
                it = h.node_iterator(s)
                try:
                    for k in range(min(int(rng.integers(1, 6)), n - s)):
                        assert it.next_long() == s + k, what
                        assert it.outdegree() == c.deg[s + k], what
                        assert np.array_equal(it.successor_array(), c.lists(s + k, s + k + 1, base)[1]), what
                finally:
                    it.close()
            elif op == "build":
                a, b = rand_range(rng.random() < 0.5)
                e, nb = h.build_index(a, b)
                log.append(what + " [%d, %d) -> %d entries, %d bytes" % (a, b, e, nb))
            elif op == "save_load":
                path = os.path.join(tmp, "case%d_step%d.bvgidx" % (case, step))
                h.save_index(path)
                f = c.open()
                try:
                    f.set_tuning(block_bits=tun["block_bits"])
                    f.load_index(path)
                    r = f.scan()
                    log.append(what + " -> loaded; scan: %d entries, %d lean blocks" % (r["index_entries"], r["lean_blocks"]))
                    _check_scan(c, r, 0, n, 0, what)
                    a, b = rand_range(False)
                    deg, succ = f.decode_range(a, b)
                    wd, ws = c.lists(a, b, 0)
                    assert np.array_equal(deg, wd) and np.array_equal(succ, ws), what
                finally:
                    f.close()
                    os.remove(path)
            elif op == "copy":
                if len(hs) >= 4:
                    continue
                hs.append([h.copy(), base, dict(tun)])
                log.append(what + " -> handle %d" % (len(hs) - 1))
            elif op == "close":
                if len(hs) <= 1:
                    continue
                h.close(); hs.pop(i)
                log.append(what)
        # every handle that is left, over the whole graph
        for i, (h, base, tun) in enumerate(hs):
            r = h.scan()
            log.append("final scan, handle %d (base %#x, %s): %d entries, %d lean blocks" % (i, base, tun, r["index_entries"], r["lean_blocks"]))
            _check_scan(c, r, 0, n, base, "case %d final scan of handle %d" % (case, i))
    finally:
        for h, _, _ in hs:
            h.close()


def test_handles_in_different_modes_take_turns(W, tools, oracle, tmp_path):
    cases = int(os.environ.get("BVG_STATE_FUZZ", "12"))
    seed = int(os.environ.get("BVG_STATE_SEED", "1"))
    first = int(os.environ.get("BVG_STATE_FROM", "0"))
    for case in range(first, cases):
        log = []
        try:
            _run_case(W, tools, oracle, np.random.default_rng([seed, case]), case, log, str(tmp_path))
        except BaseException as e:
            raise AssertionError("handle state machine failed: BVG_STATE_SEED=%d BVG_STATE_FROM=%d BVG_STATE_FUZZ=%d\n  %s\n%s: %s"
                                 % (seed, case, case + 1, "\n  ".join(log), type(e).__name__, e)) from e
        if case % 50 == 49:
            print("handle states: %d of %d cases" % (case + 1, cases), flush=True)


# ---- index provenance ---------------------------------------------------------------------------------------------------------------------

N_PROV = 12000


@pytest.fixture(scope="module")
def prov(W, tools, oracle):
    """A graph whose marks-only index is not empty: ordinary lists with locality, and in each half two lists of 6 000 random residuals
    (marks only keeps entries for lists of >= 4 096).  E_full / E_marks: what build_index() leaves on fresh handles of mode 0 / 2."""
    rng = np.random.default_rng(2024)
    n = N_PROV
    lists = []
    for x in range(n):
        if x in (1000, 4000, 7000, 10000):
            lists.append(np.sort(rng.choice(n, 6000, replace=False)))
        else:
            k = int(rng.poisson(12))
            lists.append(np.unique(rng.integers(max(0, x - 300), min(n, x + 300), k)))
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum([l.size for l in lists])
    adj = np.concatenate(lists).astype(np.int64)
    st = tools.store((off, adj), W.default_params(), threads=4)
    c = _Case(W, oracle, "provenance", st.params, st.graph, st.offsets)

    def fresh(**tun):
        g = c.open()
        if tun:
            g.set_tuning(**tun)
        return g
    f0, f2 = fresh(), fresh(no_index=2)
    c.E_full, c.E_marks = f0.build_index()[0], f2.build_index()[0]
    f0.close(); f2.close()
    assert c.E_full > c.E_marks > 0, (c.E_full, c.E_marks)
    c.fresh = fresh
    return c


def _whole(c, h, base=0):
    r = h.scan()
    _check_scan(c, r, 0, c.n, base, "whole-graph scan")
    return r


def test_marks_only_flyweight_widens_a_full_index_in_its_form(prov):
    """A (mode 0) indexes the first half; a marks-only flyweight scanning the second half widens that index to the whole graph -- as a FULL index."""
    c, h = prov, prov.n // 2
    a = c.fresh(); b = a.copy(); b.set_tuning(no_index=2)
    _check_scan(c, a.scan(0, h), 0, h, 0, "A, first half")
    _check_scan(c, b.scan(h, c.n), h, c.n, 0, "marks-only flyweight, second half")
    for who in (a, b):
        r = _whole(c, who)
        assert r["index_entries"] == c.E_full and r["lean_blocks"] > 0, r
    b.close(); a.close()


def test_wide_flyweight_leaves_a_narrow_index_alone(prov):
    """A (narrow) indexes the first half; a force_wide flyweight scanning the second half does not replace it (it scans without it): the narrow
    handles still get the whole full index and the lean kernel."""
    c, h = prov, prov.n // 2
    a = c.fresh(); w = a.copy(); w.set_tuning(force_wide=True); b = a.copy()
    _check_scan(c, a.scan(0, h), 0, h, 0, "A, first half")
    rw = w.scan(h, c.n)
    _check_scan(c, rw, h, c.n, 0, "wide flyweight, second half")
    assert rw["index_entries"] == 0, rw
    for who in (a, b):
        r = _whole(c, who)
        assert r["index_entries"] == c.E_full and r["lean_blocks"] > 0, r
    assert _whole(c, w)["index_entries"] == 0                                   # ... and the wide handle stays without it
    deg, succ = w.decode_range(0, c.n)
    assert np.array_equal(deg, c.deg) and np.array_equal(succ, c.adj)
    w.close(); b.close(); a.close()


@pytest.mark.parametrize("how", ["build_index", "half_then_other_half"])
def test_a_marks_only_index_built_first_is_used_as_it_is(prov, how):
    """Mode 2 builds first: mode-0 handles use the marks-only index as it is, and widen it (when it covers half the graph) as a marks-only index."""
    c, h = prov, prov.n // 2
    m = c.fresh(no_index=2); a = m.copy(); a.set_tuning(no_index=0)
    if how == "build_index":
        assert m.build_index()[0] == c.E_marks
    else:
        _check_scan(c, m.scan(0, h), 0, h, 0, "marks-only handle, first half")
        _check_scan(c, a.scan(h, c.n), h, c.n, 0, "mode-0 flyweight, second half")
    for who in (a, m):
        r = _whole(c, who)
        assert r["index_entries"] == c.E_marks and r["lean_blocks"] > 0, r
    a.close(); m.close()


def test_four_modes_from_four_threads(prov):
    """Flyweights in modes 0 / 1 / 2 / force_wide scan alternating halves from four threads, three rounds each, after a mode-0 handle has indexed the first
    half.  Every result equals the oracle; at the end the graph holds that index, widened to the whole graph as a full narrow index, which the narrow
    handles use as it is and the wide one does without."""
    c, h = prov, prov.n // 2
    root = c.fresh()
    _check_scan(c, root.scan(0, h), 0, h, 0, "mode-0 handle, first half")
    tun = [dict(no_index=0), dict(no_index=1), dict(no_index=2), dict(force_wide=True)]
    hs = []
    for t in tun:
        x = root.copy(); x.set_tuning(**t); hs.append(x)
    want = {(0, h): c.scan(0, h, 0), (h, c.n): c.scan(h, c.n, 0)}
    errors, barrier = [], threading.Barrier(4)

    def work(k):
        try:
            barrier.wait()
            for rnd in range(3):
                for j in range(2):
                    a, b = ((0, h), (h, c.n))[(k + rnd + j) % 2]
                    r = hs[k].scan(a, b)
                    o = want[(a, b)]
                    if (r["nodes"], r["arcs"], r["chk"]) != (o["nodes"], o["arcs"], o["chk"]):
                        errors.append((k, rnd, a, b, r, o))
        except BaseException as e:
            errors.append((k, repr(e)))
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    r = [_whole(c, x) for x in hs]
    assert r[1]["index_entries"] == 0 and r[1]["lean_blocks"] == 0, r[1]
    assert r[0]["index_entries"] == r[2]["index_entries"] == c.E_full, r
    assert r[0]["lean_blocks"] > 0 and r[2]["lean_blocks"] > 0, r
    assert r[3]["index_entries"] == 0, r
    for x in hs:
        x.close()
    root.close()


def test_index_modes_above_two_are_refused(prov, W):
    g = prov.fresh()
    for bad in (3, 4, 0xFFFFFFFF):
        with pytest.raises(W.IllegalArgumentException):
            g.set_tuning(no_index=bad)
    g.set_tuning(no_index=2)                                                    # (the valid ones still pass)
    _whole(prov, g)
    g.close()


def test_index_of_a_wide_window_graph_loads_back(W, tools, oracle, tmp_path):
    """Windows above 64 run the global-memory kernel, whose block halos reach up to 8 192 nodes back (bvg_kernels.h, kMaxHaloBig): an index saved
    for such a graph loads back into a fresh handle (found by the state machine above: the loader held every halo to the 64 of narrower windows)."""
    n = 3000
    lists = [sorted(set([n - 3, n - 2, n - 1, x % 7, (x * 3) % 11 + 20])) for x in range(n)]       # every list copies most of the one before
    st = tools.store(lists, W.default_params(window_size=70, max_ref_count=-1))
    c = _Case(W, oracle, "wide window", st.params, st.graph, st.offsets)
    for bb in BLOCK_BITS:
        g = c.open(); g.set_tuning(block_bits=bb)
        _whole(c, g)
        path = str(tmp_path / ("w%d.bvgidx" % bb))
        g.save_index(path)
        f = c.open(); f.set_tuning(block_bits=bb)
        f.load_index(path)
        _whole(c, f)
        deg, succ = f.decode_range(0, n)
        assert np.array_equal(deg, c.deg) and np.array_equal(succ, c.adj)
        f.close(); g.close()
