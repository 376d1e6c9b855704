"""GPU: the offsets index derived on the device from a bare .graph (bvg_open_mem with offsets = NULL; BVGraph -O / writeOffsets,
BVGraph.java:2595-2609) -- the chunk-parallel speculative walk of csrc/bvg_derive.hip and the one-wavefront sequential walk of
csrc/bvg_derive_seq.hip -- differentially, bit for bit, over the parameter space, the chunk geometry, the three blind states, both round
kernels, streams the encoder never writes and streams that are wrong.

Every derivation runs on BOTH walks (default, and BVG_DERIVE_SEQ=1) and is compared with two independent CPU restatements: the offsets the
writer of the stream recorded and the oracle's own derivation (tests/derive_cases.py).  Which walk answered is asserted per case from the
BVG_DEBUG line of csrc/bvg_plan.hip, and the parallel walk's rounds are at most chunks + 1 (the induction in bvg_derive.hip's header).
BVG_DERIVE_WARM / BVG_DERIVE_CRAWL (test knobs) take the 8-chunk warm-up away and choose the round kernel, so that detect / adopt and both
kernels settle most of the chunks on inputs of a few chunks.

Found by this suite (regression tests below, named after what they found):
  * the sequential walk refused a reference that points before node 0 with BVG_E_STATE, the parallel walk derived the stream: the same
    stream opened or not depending on the walk.  The reference's sequential iterator accepts it (BVG:1018 indexes its fresh window,
    BVG:1030 reads outdegree 0 there; only BVG:701, ref > window, throws), so both walks now derive it.
  * the parallel walk did not look at a negative copy count (blocks that skip more than the referenced list has); the sequential walk
    refuses it (ERR_MALFORMED): now both do.
  * unary codes of more than 64 bits (a block of 64 kept elements in unary coding is one) sent the whole stream to the sequential walk:
    the parallel walk now reads them (test_unary_codes_beyond_64_bits; test_parameter_space[codings-*] on the dense graph).
"""
import ctypes as C

import numpy as np
import pytest

from bvrecords import PyBits, Record, assemble, int2nat
from derive_cases import (CHUNK_BITS, MAX_WINDOW, ROUTES, check_derivation, chunks_of, golomb_bound_ok, local_adjacency, open_on,
                          oracle_offsets, set_route, with_empty_nodes)
from test_gpu_fuzz import _adjacency
from test_gpu_long_codes import _graph as _long_code_graph
from test_malformed_streams import CASES as ODD_CASES, _graph as _odd_graph

pytestmark = pytest.mark.gpu


# ---- 1a. the parameter space ---------------------------------------------------------------------------------------------------------
def _sets():
    S = {"windows": [dict(window_size=w, max_ref_count=3 if w else 0) for w in (0, 1, 2, 3, 4, 7, 8, 63, 64, 65, 126, 127, 128, 200, MAX_WINDOW)],
         "refcounts": [dict(max_ref_count=m) for m in (0, 1, 3, -1)] + [dict(window_size=64, max_ref_count=-1)],
         "intervals": [dict(min_interval_length=m) for m in (0, 1, 2, 4, 7)],
         "zeta": [dict(zeta_k=k) for k in range(1, 8)],
         # every coding the header allows for a field (include/bvgraph_hip.h, bvg_params), each field alone ...
         "codings": [dict(outdegree_coding=1)] + [dict(reference_coding=c) for c in (1, 2)] + [dict(block_count_coding=c) for c in (1, 5)] +
                    [dict(block_coding=c) for c in (1, 5)] + [dict(residual_coding=c) for c in (1, 2, 7)] +
                    # ... and all together (the GEN instantiations of every kernel)
                    [dict(outdegree_coding=1, reference_coding=2, block_count_coding=5, block_coding=1, residual_coding=1),
                     dict(outdegree_coding=1, reference_coding=1, block_count_coding=1, block_coding=5, residual_coding=7, window_size=20, min_interval_length=2),
                     dict(outdegree_coding=2, reference_coding=2, block_count_coding=2, block_coding=2, residual_coding=2, zeta_k=1)],
         "golomb": [dict(residual_coding=3, zeta_k=m) for m in (1, 2, 3, 8)] + [dict(residual_coding=3, zeta_k=8, outdegree_coding=1, block_coding=5, reference_coding=2, block_count_coding=5)]}
    return S


SETS = _sets()


def _shapes(tools, group):
    if group == "golomb":                                                    # (residuals that fit 64 bits: derive_cases.golomb_bound_ok)
        return [("local", local_adjacency(np.random.default_rng(5), 3000, reach=9)), ("local_sparse", local_adjacency(np.random.default_rng(6), 2000, reach=9, deg=2))]
    return [("web_like", tools.synth_adjacency(2500, seed=3, synth=tools.web_like())),
            ("eu_like", tools.synth_adjacency(700, seed=4, synth=tools.eu_like())),
            ("fuzz", _adjacency(np.random.default_rng(9), 900))]


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("group", sorted(SETS))
def test_parameter_space(W, tools, oracle, capfd, monkeypatch, group, route):
    set_route(monkeypatch, route)
    settled = 0
    for name, (off, adj) in _shapes(tools, group):
        for kw in SETS[group]:
            p = W.default_params(**kw)
            if group == "golomb":
                assert golomb_bound_ok(off, adj, kw["zeta_k"])
            st = tools.store((off, adj), p)
            expect = "parallel" if p.window_size <= 127 else "fallback"
            settled += check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, expect, what=(name, kw, route))
    print("derive %s/%s: %d rounds in all" % (group, route, settled))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_chunks_that_restart_the_window(W, tools, oracle, capfd, monkeypatch, route):
    """The encoder's chunk_nodes restarts the reference window at every chunk of nodes: to the walk a record without reference, no more."""
    set_route(monkeypatch, route)
    off, adj = tools.synth_adjacency(2500, seed=3, synth=tools.web_like())
    for chunk in (64, 1000, 0):
        for kw in (dict(), dict(window_size=100, max_ref_count=-1)):
            st = tools.store((off, adj), W.default_params(**kw), chunk_nodes=chunk)
            check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, what=(chunk, kw))


def _degenerate():
    D = {"one_node": [[]], "one_node_loop": [[0]], "all_empty": [[] for _ in range(100)],
         "one_list_only": [[] if x != 50 else [3, 9, 50, 77] for x in range(100)],
         "complete_70": [list(range(70)) for _ in range(70)],
         "one_interval": [[] if x != 10 else list(range(20, 70)) for x in range(100)],
         # node 31 copies all of node 30 and has no block: the bc == 0 branch (BVG:1030); then one extra on top, one node further
         "copies_all_no_blocks": [[5, 9, 13, 40, 41, 90] if x in (30, 31) else ([5, 9, 13, 40, 41, 77, 90] if x == 32 else [x]) for x in range(100)]}
    return D


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape", sorted(_degenerate()))
def test_degenerate_graphs(W, tools, oracle, capfd, monkeypatch, shape, route):
    """(Streams of one chunk: no later round exists, so the routes differ in nothing here; they run for completeness.  The parameter-space
    streams above have 3 to 10 chunks, the geometry streams 12, the blind-state ones 10 to 20 and the tiled streams of the randomised
    test tens: with BVG_DERIVE_WARM=0 most of their chunks are settled by detect / adopt and the chosen round kernel, which
    derive_cases.check_route asserts from the debug lines.)"""
    set_route(monkeypatch, route)
    lists = _degenerate()[shape]
    for kw in (dict(), dict(window_size=1, max_ref_count=-1, min_interval_length=2), dict(window_size=0, max_ref_count=0, min_interval_length=0), dict(window_size=130)):
        st = tools.store(lists, W.default_params(**kw))
        if shape == "copies_all_no_blocks" and not kw:
            b = oracle.Bits(); g = np.frombuffer(st.graph.tobytes() + b"\0" * 16, dtype=np.uint8)
            oracle.lib().bvgo_bits_init(C.byref(b), g.ctypes.data, len(st.graph), int(st.offsets[31]))
            L = oracle.lib()
            assert (L.bvgo_read_gamma(C.byref(b)), L.bvgo_read_unary(C.byref(b)), L.bvgo_read_gamma(C.byref(b))) == (6, 1, 0)   # d, ref, no blocks
            assert b.pos == int(st.offsets[32])
        check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, "parallel" if st.params.window_size <= 127 else "fallback", what=(shape, kw))


# ---- 1b. chunk geometry --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twelve_chunks(tools):
    off, adj = tools.synth_adjacency(10000, seed=21, synth=tools.web_like())
    st = tools.store((off, adj))
    assert 11 <= chunks_of(st.graph) <= 13
    return off, adj, st


@pytest.mark.parametrize("route", ["default", "warm0_list", "warm0_crawl"])
@pytest.mark.parametrize("first", range(0, 72, 8))
def test_every_alignment_of_records_and_chunk_boundaries(W, tools, oracle, capfd, monkeypatch, twelve_chunks, first, route):
    """j empty nodes in front move every record and every code of a 12-chunk stream by j bits against the 32 768-bit chunk boundaries:
    over j = 0..71 a record that starts exactly on a boundary occurs, and for every j boundaries that fall inside a record (asserted over the
    whole sweep in test_the_sweep_meets_the_boundaries; a boundary inside a record moves through every bit of 72 consecutive ones, so it
    falls inside codes and between codes)."""
    set_route(monkeypatch, route)
    off, adj, base = twelve_chunks
    for j in range(first, first + 8):
        o2, a2 = with_empty_nodes(off, adj, j, j % 3)
        st = tools.store((o2, a2))
        assert np.array_equal(st.offsets[j:j + len(base.offsets)], base.offsets + np.uint64(j)) and int(st.offsets[-1]) == int(base.offsets[-1]) + j + j % 3
        check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, what=("lead", j))


def test_the_sweep_meets_the_boundaries(twelve_chunks):
    """What the sweep above claims, from the encoder's offsets: some j puts a record start exactly on a chunk boundary, and for every j
    some chunk boundary falls strictly inside a record."""
    off, adj, base = twelve_chunks
    o = base.offsets.astype(np.int64)
    on_boundary = [j for j in range(72) if np.any((o[1:-1] + j) % CHUNK_BITS == 0)]
    assert on_boundary, "no j in 0..71 puts a record start on a chunk boundary"
    for j in range(72):
        b = np.arange(1, chunks_of(base.graph)) * CHUNK_BITS
        inside = [x for x in b if not np.any(o + j == x) and x < o[-1] + j]
        assert inside, j


def _padded_to(tools, W, total_bits, seed=31):
    """A web-like stream of exactly total_bits bits: records, then empty nodes (one bit each) up to the length asked for."""
    n = max(1, int(total_bits / 42))
    for _ in range(20):
        off, adj = tools.synth_adjacency(n, seed=seed, synth=tools.web_like())
        st = tools.store((off, adj))
        if int(st.offsets[-1]) <= total_bits:
            break
        n = max(1, int(n * 0.93))
    trail = total_bits - int(st.offsets[-1])
    assert 0 <= trail < CHUNK_BITS
    st = tools.store(with_empty_nodes(off, adj, 0, trail))
    assert int(st.offsets[-1]) == total_bits
    return st


@pytest.mark.parametrize("route", ["default", "warm0_list", "warm0_crawl"])
@pytest.mark.parametrize("bits", [3000, 3001, CHUNK_BITS - 1, CHUNK_BITS, CHUNK_BITS + 1, 2 * CHUNK_BITS, 8 * CHUNK_BITS - 1, 8 * CHUNK_BITS, 8 * CHUNK_BITS + 1,
                                  9 * CHUNK_BITS, 10 * CHUNK_BITS, 10 * CHUNK_BITS + 8])
def test_streams_that_end_on_bytes_and_chunks(W, tools, oracle, capfd, monkeypatch, bits, route):
    """Less than one chunk, exactly 1, 2, 8, 9, 10 chunks (around the warm-up of 8), one bit before and behind a chunk boundary, a last byte
    without padding bits and with seven of them."""
    set_route(monkeypatch, route)
    st = _padded_to(tools, W, bits)
    assert len(st.graph) == (bits + 7) // 8 and chunks_of(st.graph) == -(-bits // CHUNK_BITS)
    if bits % CHUNK_BITS == 0:
        assert chunks_of(st.graph) == bits // CHUNK_BITS
    check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, what=bits)


# ---- 1c. the three blind states ------------------------------------------------------------------------------------------------------
def _sprinkle(lists, n, skip):
    for x in range(0, n, 37):
        if x not in skip:
            lists[x] = [min(n - 1, x + 1), min(n - 1, x + 5), min(n - 1, x + 11)] if x + 1 < n else []
    return lists


def _giant(kind):
    """(lists, giant node, params): one record that keeps a walk blind for more than three chunks, among ordinary records."""
    rng = np.random.default_rng(4)
    if kind == "residuals":                                                   # > 4 096 residuals left at a chunk boundary
        n, x = 200000, 700
        big = np.cumsum(rng.integers(2, 9, 36000)); kw = {}
        lists = [[] for _ in range(n)]; lists[x] = big[big < n].tolist()
        skip = {x}
    elif kind == "blocks":                                                    # node x copies every other element of node x - 1: 60 000 blocks of one
        n, x = 125000, 901
        lists = [[] for _ in range(n)]; lists[x - 1] = list(range(1000, 121000)); lists[x] = lists[x - 1][::2]; kw = {}
        skip = {x - 1, x}
    else:                                                                     # > 2 048 intervals: pairs of consecutive ids, min_interval_length 2
        n, x = 125000, 801
        left = np.arange(1000, 121000, 4); lists = [[] for _ in range(n)]; lists[x] = np.stack([left, left + 1], 1).ravel().tolist(); kw = dict(min_interval_length=2)
        skip = {x}
    return _sprinkle(lists, n, skip), x, kw


@pytest.mark.parametrize("route", ["default", "warm0_list", "warm0_crawl"])
@pytest.mark.parametrize("where", ["as_is", "next_starts_before_a_boundary", "next_starts_behind_a_boundary"])
@pytest.mark.parametrize("kind", ["residuals", "blocks", "intervals"])
def test_blind_states(W, tools, oracle, capfd, monkeypatch, kind, where, route):
    """blind_state() of bvg_derive.hip: thousands of residuals / blocks / intervals outstanding at a chunk boundary.  Such an exit state is
    handed on only when exact, so the chunks inside the record settle one per round.  The record spans at least three chunks (asserted),
    and in the two variants the record behind it starts within 64 bits of a chunk boundary."""
    set_route(monkeypatch, route)
    lists, x, kw = _giant(kind)
    off = np.zeros(len(lists) + 1, np.uint64); off[1:] = np.cumsum([len(l) for l in lists])
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists if len(l)])
    p = W.default_params(**kw)
    st = tools.store((off, adj), p)
    lead = 0
    if where != "as_is":
        target = CHUNK_BITS - 20 if where == "next_starts_before_a_boundary" else 7
        lead = (target - int(st.offsets[x + 1])) % CHUNK_BITS
        st = tools.store(with_empty_nodes(off, adj, lead, 0), p)
        d = int(st.offsets[lead + x + 1]) % CHUNK_BITS
        assert d == target and min(d, CHUNK_BITS - d) < 64
    a, b = int(st.offsets[lead + x]), int(st.offsets[lead + x + 1])
    assert b // CHUNK_BITS - a // CHUNK_BITS >= 3, "the record must span at least three chunks"
    # the record is what it is meant to be: its header, read with the oracle's bit reader
    L = oracle.lib(); bits = oracle.Bits(); g = np.frombuffer(st.graph.tobytes() + b"\0" * 16, dtype=np.uint8)
    L.bvgo_bits_init(C.byref(bits), g.ctypes.data, len(st.graph), a)
    d, ref = L.bvgo_read_gamma(C.byref(bits)), L.bvgo_read_unary(C.byref(bits))
    if kind == "residuals":
        assert d > 30000 and ref == 0 and L.bvgo_read_gamma(C.byref(bits)) == 0          # no reference, no intervals: residuals only
    elif kind == "blocks":
        assert d == 60000 and ref == 1 and L.bvgo_read_gamma(C.byref(bits)) > 100000     # one block per element of the referenced list
    else:
        assert d == 60000 and ref == 0 and L.bvgo_read_gamma(C.byref(bits)) == 30000     # 30 000 intervals
    check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, what=(kind, where, route))


# ---- 1e. streams the encoder never writes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "warm0_list"])
@pytest.mark.parametrize("case", sorted(ODD_CASES))
def test_legal_but_odd_records(W, oracle, capfd, monkeypatch, case, route):
    """tests/test_malformed_streams.py::_cases(): over-running copy blocks, the cap at d, lists that come out short.  Counts alone decide a
    record's length, so the derivation gives bvrecords' offsets (or a status: never BVG_OK with other offsets)."""
    set_route(monkeypatch, route)
    for lead, pad in [(0, 0), (5, 80), (70, 3), (0, 1500)]:
        recs = _odd_graph(case, pad, lead)
        g, offs, lists = assemble(recs)
        p = W.default_params().clone(nodes=len(recs), arcs=int(sum(r.d for r in recs)))
        check_derivation(W, oracle, capfd, monkeypatch, p, np.frombuffer(g, dtype=np.uint8), offs, what=(case, lead, pad))


@pytest.mark.parametrize("route", ["default", "warm0_crawl"])
def test_codes_of_32_to_40_bits(W, oracle, capfd, monkeypatch, route):
    """The streams of tests/test_gpu_long_codes.py: residual codes of 32 and 40 bits fit the walk's 64-bit window."""
    set_route(monkeypatch, route)
    recs = _long_code_graph(300)
    g, offs, lists = assemble(recs)
    p = W.default_params().clone(nodes=len(recs), arcs=int(sum(r.d for r in recs)))
    assert chunks_of(g) >= 3
    check_derivation(W, oracle, capfd, monkeypatch, p, np.frombuffer(g, dtype=np.uint8), offs)


def test_unary_codes_beyond_64_bits(W, oracle, capfd, monkeypatch):
    """REGRESSION (found by the per-set assertion of tests/test_gpu_api.py: block counts of 64 and 70 in unary coding sent a whole 200 000-node
    graph to the sequential walk without a word; that case itself is the next test).  Here the other unary field: a unary reference of 70 and of 100 (window 100) is a code of 71 and 101 bits, and the
    second one here straddles a chunk boundary (asserted): the parallel walk reads such codes a word at a time, as the sequential walk
    does, and no longer falls back."""
    base = [10 * (i + 1) for i in range(10)]
    plain = lambda x: Record(d=10, residuals=[v + x for v in base])
    offs0 = assemble([plain(x) for x in range(600)], window=100)[1].astype(np.int64)
    x2 = int(np.flatnonzero(offs0 + 7 < CHUNK_BITS)[-1])                       # gamma(10) is 7 bits: the reference starts behind them
    recs = [plain(x) for x in range(600)]
    recs[80] = Record(d=11, ref=70, blocks=[10], residuals=[5000])
    recs[x2] = Record(d=10, ref=100, blocks=[])
    g, offs, lists = assemble(recs, window=100)
    start = int(offs[x2]) + 7
    assert x2 > 180 and start < CHUNK_BITS < start + 101, "the 101-bit code must straddle the chunk boundary"
    p = W.default_params(window_size=100).clone(nodes=len(recs), arcs=int(sum(r.d for r in recs)))
    for route in ("default", "warm0_list", "warm0_crawl"):
        set_route(monkeypatch, route)
        check_derivation(W, oracle, capfd, monkeypatch, p, np.frombuffer(g, dtype=np.uint8), offs, what=route)


def test_unary_block_counts_and_blocks_of_64_and_more(W, oracle, capfd, monkeypatch):
    """REGRESSION, the case as it was found: block counts and blocks in unary coding.  Node 1 copies node 0's 200 elements through 70 blocks
    of one (a unary block count of 70: 71 bits), node 3 keeps 80 and skips 70 (unary blocks of 81 and 70 bits); the parallel walk derives
    the stream and does not fall back."""
    w = PyBits(); offs = []
    big = lambda x: Record(d=200, residuals=[x + 3 + 2 * i for i in range(200)])

    def odd(d, blocks, residuals, x):
        w.gamma(d); w.unary(1); w.unary(len(blocks))
        for i, b in enumerate(blocks):
            w.unary(b if i == 0 else b - 1)
        if residuals:
            w.gamma(0)                                                       # no intervals
            prev = None
            for i, r in enumerate(residuals):
                w.zeta(int2nat(r - x) if i == 0 else r - prev - 1, 3); prev = r
    n = 0
    for rep in range(40):                                                     # 40 groups: several chunks
        for kind in ("big", "count70", "big", "block80", "plain"):
            offs.append(len(w))
            if kind == "big": big(n).write(w, n, 7, 4, 3, 200)
            elif kind == "count70": odd(35 + 130, [1] * 70, [], n)            # even count: 35 kept + the 130 behind the blocks (BVG:1030)
            elif kind == "block80": odd(80 + 50 + 1, [80, 70], [n + 5000], n)  # keep 80, skip 70, the other 50 kept, one residual
            else: _plain(n).write(w, n, 7, 4, 3, 10)
            n += 1
    offs.append(len(w))
    g = np.frombuffer(w.tobytes(), dtype=np.uint8)
    assert chunks_of(g) >= 3
    p = W.default_params(block_count_coding=5, block_coding=5).clone(nodes=n, arcs=40 * (400 + 165 + 131 + 10))
    for route in ("default", "warm0_list", "warm0_crawl"):
        set_route(monkeypatch, route)
        check_derivation(W, oracle, capfd, monkeypatch, p, g, np.array(offs, dtype=np.uint64), what=route)


def test_a_run_of_zeros_to_the_end_is_no_unary_code(W, oracle, capfd, monkeypatch):
    """The last record's unary reference never ends: 200 zero bits up to the end of the stream.  EOFException from the oracle and both walks."""
    set_route(monkeypatch, "default")
    w = PyBits()
    recs = [_plain(x) for x in range(40)]
    for x, r in enumerate(recs):
        r.write(w, x, 7, 4, 3, r.d)
    w.gamma(5); w.put(0, 200)
    p = W.default_params().clone(nodes=41, arcs=405)
    _refused(W, oracle, capfd, monkeypatch, p, np.frombuffer(w.tobytes(), dtype=np.uint8), W.EOFException, -5)


# ---- 1f. status parity on streams that are wrong -------------------------------------------------------------------------------------
FIELDS = ["outdegree", "reference", "block_count", "block", "interval_count", "interval_left", "interval_length", "residual"]


def _stream_with_every_field(lead):
    """`lead` empty nodes, node `lead` = ten residuals, node lead + 1 = a record with every field of the state machine (no code of one bit).
    Returns (PyBits, offsets, {field: (first bit, last bit + 1) of one code of that kind in the last record})."""
    w = PyBits(); offs = []; at = {}
    for _ in range(lead):
        offs.append(len(w)); w.gamma(0)
    x = lead
    offs.append(len(w)); Record(d=10, residuals=[x + 10 * (i + 1) for i in range(10)]).write(w, x, 7, 4, 3, 10)
    x += 1
    offs.append(len(w))

    def put(name, f, *a):
        s = len(w); f(*a); at[name] = (s, len(w))
    put("outdegree", w.gamma, 14)                      # d = 14: 4 copied + 8 in an interval + 2 residuals
    put("reference", w.unary, 1)
    put("block_count", w.gamma, 2)
    put("block", w.gamma, 4); w.gamma(5)               # keep 4, skip 6 (written as 6 - 1): nothing is left to copy
    put("interval_count", w.gamma, 1)
    put("interval_left", w.gamma, int2nat(300 - x))
    put("interval_length", w.gamma, 8 - 4)
    put("residual", w.zeta, int2nat(500 - x), 3); w.zeta(40, 3)
    offs.append(len(w))
    return w, np.array(offs, dtype=np.uint64), at


@pytest.mark.parametrize("field", FIELDS)
def test_truncated_inside_each_field(W, oracle, capfd, monkeypatch, field):
    """The stream ends (on a byte, as files do) inside a code of each of the eight field kinds of the walk's state machine: EOFException
    from the bit stream, BVG_E_EOF, from the oracle and from both walks."""
    set_route(monkeypatch, "default")
    s, e = _stream_with_every_field(0)[2][field]
    assert e - s >= 2
    lead = (-(s + 1)) % 8                               # the cut falls one bit into the code
    w, offs, at = _stream_with_every_field(lead)
    s, e = at[field]
    cut = s + 1
    assert cut % 8 == 0 and s < cut < e
    whole = np.frombuffer(w.tobytes(), dtype=np.uint8)
    p = W.default_params().clone(nodes=len(offs) - 1, arcs=24)
    check_derivation(W, oracle, capfd, monkeypatch, p, whole, offs, what=field)      # (the whole stream is fine)
    _refused(W, oracle, capfd, monkeypatch, p, whole[:cut // 8].copy(), W.EOFException, -5)


def _refused(W, oracle, capfd, monkeypatch, p, graph, exc, ocode):
    """Both walks and the oracle's derivation refuse the stream with the same status."""
    with pytest.raises(oracle.OracleError) as oe:
        oracle_offsets(oracle, p, graph)
    assert oe.value.code == ocode
    for walk in ("parallel", "seq"):
        g, got, used, rounds = open_on(W, capfd, monkeypatch, p, graph, walk)
        if g is not None:
            g.close()
        assert got is exc, (walk, got)
        assert used == "fallback"                       # (the parallel walk flags the stream and the sequential one names the error)


def _plain(x):
    return Record(d=10, residuals=[x + 10 * (i + 1) for i in range(10)])


def test_more_nodes_than_records(W, oracle, capfd, monkeypatch):
    set_route(monkeypatch, "default")
    for n_recs in (3, 900):
        g, offs, lists = assemble([_plain(x) for x in range(n_recs)])
        for more in (1, 64, 5000):
            p = W.default_params().clone(nodes=n_recs + more, arcs=10 * n_recs)
            _refused(W, oracle, capfd, monkeypatch, p, np.frombuffer(g, dtype=np.uint8), W.EOFException, -5)


def test_fewer_nodes_than_records_is_legal(W, oracle, capfd, monkeypatch):
    """nodes smaller than the records present: the first nodes + 1 offsets."""
    set_route(monkeypatch, "default")
    g, offs, lists = assemble([_plain(x) for x in range(1200)])
    assert chunks_of(g) >= 3
    for n in (1, 63, 64, 65, 700, 1199):
        p = W.default_params().clone(nodes=n, arcs=10 * n)
        check_derivation(W, oracle, capfd, monkeypatch, p, np.frombuffer(g, dtype=np.uint8), offs[:n + 1], what=n)


@pytest.mark.parametrize("lead", [0, 3, 700])
def test_reference_above_the_window(W, oracle, capfd, monkeypatch, lead):
    """BVG:701: IllegalStateException, BVG_E_STATE, from the oracle and both walks (the parallel walk flags it and falls back, so the
    documented bit comes from the sequential walk)."""
    set_route(monkeypatch, "default")
    recs = [_plain(x) for x in range(lead + 12)] + [Record(d=3, ref=9, blocks=[3])] + [_plain(lead + 13 + x) for x in range(5)]
    w = PyBits()
    for x, r in enumerate(recs):
        r.write(w, x, 7, 4, 3, 0 if r.ref else r.d)
    p = W.default_params().clone(nodes=len(recs), arcs=10 * len(recs))
    _refused(W, oracle, capfd, monkeypatch, p, np.frombuffer(w.tobytes(), dtype=np.uint8), W.IllegalStateException, -2)


@pytest.mark.parametrize("blocks", [[], [2], [1, 3, 2]])
def test_reference_before_node_0_is_derived_by_both_walks(W, oracle, capfd, monkeypatch, blocks):
    """REGRESSION (found by this suite; the header's mapping and the oracle differed from the sequential walk here).  Node 2 refers to node
    2 - 5.  The reference's sequential iterator -- the one writeOffsets runs -- does not throw: refIndex = (x - ref + cyclicBufferSize) %
    cyclicBufferSize (BVG:1018) is a slot of its fresh window, outd[refIndex] is 0 (BVG:1030), only ref > windowSize throws (BVG:701).
    The sequential walk returned BVG_E_STATE (its `v > x` check), the parallel walk BVG_OK: one stream, two answers.  Both derive it now,
    as the oracle does; the record's length follows from the counts: copied = the kept blocks."""
    set_route(monkeypatch, "default")
    w = PyBits(); offs = []
    recs = [_plain(0), _plain(1), Record(d=6, ref=5, blocks=blocks, residuals=[])] + [_plain(3 + x) for x in range(40)]
    copied = sum(blocks[0::2]) + (0 - sum(blocks) if len(blocks) % 2 == 0 else 0)
    assert copied >= 0
    recs[2].residuals = [50 + 3 * i for i in range(6 - copied)]
    for x, r in enumerate(recs):
        offs.append(len(w)); r.write(w, x, 7, 4, 3, r.d - copied if x == 2 else r.d)
    offs.append(len(w))
    p = W.default_params().clone(nodes=len(recs), arcs=10 * len(recs))
    check_derivation(W, oracle, capfd, monkeypatch, p, np.frombuffer(w.tobytes(), dtype=np.uint8), np.array(offs, dtype=np.uint64), scan=False, what=blocks)


def _contradicting(kind, lead):
    recs = [_plain(x) for x in range(lead + 2)]
    x = lead + 2
    if kind == "blocks_skip_more_than_the_list_has":      # keep 0, skip 20 of a list of 10: copied = 0 + (10 - 20) < 0 (BVG:1030)
        odd, extra = Record(d=4, ref=1, blocks=[0, 20], residuals=[x + 7 * (i + 1) for i in range(14)]), 14
    elif kind == "blocks_copy_more_than_the_outdegree":    # keep all 10 of the list, d = 3: extra = -7
        odd, extra = Record(d=3, ref=1, blocks=[]), 0
    else:                                                  # an interval of 12 in a list of 5
        odd, extra = Record(d=5, intervals=[(x + 10, 12)]), 5
    recs.append(odd)
    recs += [_plain(x + 1 + i) for i in range(30)]
    w = PyBits()
    for i, r in enumerate(recs):
        r.write(w, i, 7, 4, 3, extra if r is odd else r.d)
    return len(recs), np.frombuffer(w.tobytes(), dtype=np.uint8)


@pytest.mark.parametrize("lead", [0, 900])
@pytest.mark.parametrize("kind", ["blocks_skip_more_than_the_list_has", "blocks_copy_more_than_the_outdegree", "interval_longer_than_the_extras"])
def test_counts_that_contradict_each_other_are_refused_by_both_walks(W, oracle, capfd, monkeypatch, kind, lead):
    """A negative copy count or a negative residual count: ERR_MALFORMED, BVG_E_EOF, from BOTH walks (the first kind is a REGRESSION test:
    the parallel walk did not look at the copy count and read d + 10 residuals on, the sequential walk refused).  The oracle is no
    reference for the status here: the Java builds a ResidualLongIterator that never stops at 0 (BVG:902-935, 1062-1064) and reads on
    through the next records, the oracle treats a count <= 0 as none (its one documented deviation, tests/test_malformed_streams.py), and
    the HIP path refuses instead of guessing.  What is pinned is that no walk returns BVG_OK."""
    set_route(monkeypatch, "default")
    n, graph = _contradicting(kind, lead)
    p = W.default_params().clone(nodes=n, arcs=10 * n)
    for walk in ("parallel", "seq"):
        g, got, used, rounds = open_on(W, capfd, monkeypatch, p, graph, walk)
        if g is not None:
            g.close()
        assert got is W.EOFException and used == "fallback", (walk, got, used)
