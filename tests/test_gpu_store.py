"""GPU: BVGraph.store on the device (bvg_store, csrc/bvg_encode.hip; SURVEY §8(f) rank 4, second half).
Reference: BVGraph.java:1595-1618 (intervalize), :1977-2159 (diffComp), :2216-2327 (reference selection), :2404-2457 (per-thread ranges).
The bar is byte-exactness: the reference's own fixture cnr-2000.graph / .offsets must be regenerated from the text golden, and on
synthetic graphs the device output must equal the CPU tooling's (which is itself held to the fixture and to hand-computed records,
tests/test_store.py) for every coding, window, chunking and degenerate shape; what was written must decode back to the adjacency.

The grid below the original tests covers what only the compressor has: windows of 64..127 (enc_choose_kernel's second group of lanes),
min_interval_length = 1, chunks that do not divide n or are shorter than the window, references that must be found beyond lane 63,
ties between lane groups, empty lists inside the window, one list of over 100 000 successors, every residual coding at its edge
parameter.  Every case compares offsets and bytes with the tooling AND decodes the device's bytes with the CPU oracle, which shares
no code with either encoder.  tests/test_emu.py runs this file on the host emulator in both lane orders."""
import functools

import numpy as np
import pytest

from conftest import CNR
from test_gpu_fuzz import _adjacency

pytestmark = pytest.mark.gpu


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64) if len(lists) else 0
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) and off[-1] else np.empty(0, np.int64)
    return off, adj


def test_cnr2000_fixture_is_regenerated_byte_for_byte(W, tools, cnr_golden):
    p = W.parse_properties(open(CNR + ".properties").read())
    graph, offsets = W.store(_csr(cnr_golden), p)
    assert graph.tobytes() == open(CNR + ".graph", "rb").read()
    assert tools.encode_offsets(offsets, p.offset_coding).tobytes() == open(CNR + ".offsets", "rb").read()


@pytest.mark.parametrize("kw", [
    dict(),
    dict(window_size=0, max_ref_count=0, min_interval_length=0),
    dict(window_size=1, max_ref_count=1, min_interval_length=2),
    dict(window_size=16, max_ref_count=-1, min_interval_length=3, zeta_k=5),
    dict(window_size=7, max_ref_count=3, min_interval_length=0),
    dict(outdegree_coding=1, block_coding=1, residual_coding=1, reference_coding=1, block_count_coding=1),
    dict(residual_coding=2, reference_coding=2, block_count_coding=5, block_coding=5),
    dict(residual_coding=7), dict(residual_coding=3, zeta_k=4),
])
@pytest.mark.parametrize("chunk", [0, 1000])
def test_device_store_equals_cpu_tooling(W, tools, kw, chunk):
    off, adj = tools.synth_adjacency(7000, seed=23, synth=tools.eu_like(mean_deg=40.0), chunk_nodes=1 << 16)
    p = W.default_params(**kw)
    want = tools.store((off, adj), p, chunk_nodes=chunk)
    graph, offsets = W.store((off, adj), p, chunk_nodes=chunk)
    assert np.array_equal(offsets, want.offsets), kw
    assert graph.tobytes() == want.graph.tobytes(), kw


def test_round_trip_through_the_hip_decoder(W, tools, oracle):
    off, adj = tools.synth_adjacency(20000, seed=29, synth=tools.web_like(), chunk_nodes=1 << 16)
    p = W.default_params().clone(nodes=20000, arcs=len(adj))
    graph, offsets = W.store((off, adj), p)
    g = W.BVGraph.from_memory(p, graph, offsets)
    deg, succ = g.decode_range(0, 20000)
    assert np.array_equal(deg, np.diff(off).astype(np.int32)) and np.array_equal(succ, adj)
    g.close()


def test_degenerate_adjacencies(W, tools):
    for lists in ([], [[]], [[0]], [[], [], []], [[1, 2], [0, 1, 2], [0, 1, 2]], [list(range(50))] * 50 + [[]] * 3 + [[5, 49]]):
        lists = [l for l in lists]
        n = len(lists)
        lists = [[v for v in l if v < max(n, 1)] for l in lists]
        p = W.default_params()
        want = tools.store(lists, p) if n else None
        graph, offsets = W.store(lists, p)
        if n:
            assert np.array_equal(offsets, want.offsets) and graph.tobytes() == want.graph.tobytes(), lists
        else:
            assert len(graph) == 0 and offsets.tolist() == [0]
    with pytest.raises(W.IllegalArgumentException):
        W.store([[1, 1], [0]], W.default_params())                  # duplicate successor (BVG:2141)
    with pytest.raises(W.IllegalArgumentException):
        W.store([[0, 5]], W.default_params())                       # successor outside the graph
    # the input check (enc_check_kernel) refuses, before any list is walked, offsets that do not describe adj[0 .. adj_off[nodes])
    u64, three = np.uint64, np.array([0, 1, 2], np.int64)
    for off, adj in [(np.array([0, 1000000, 3], u64), three),       # a list that ends beyond adj_off[nodes]
                     (np.array([0, 2, 1, 3], u64), three),          # offsets that decrease
                     (np.array([0, 5, 4, 3], u64), three),          # ... and start beyond the end as well
                     (np.array([1, 2, 3], u64), np.array([0, 0, 1], np.int64)),       # adj_off[0] != 0 (the lists themselves are fine)
                     (np.array([0, 2, 3], u64), np.array([-1, 0, 1], np.int64)),      # a negative successor
                     (np.array([0, 2, 3], u64), np.array([1, 0, 1], np.int64))]:      # a decreasing pair
        with pytest.raises(W.IllegalArgumentException):
            W.store((off, adj), W.default_params())


# ---- the grid: every case is held to the tooling's offsets and bytes, and the device's bytes to the oracle --------------------------

def _held_to_tooling_and_oracle(W, tools, oracle, adj, p, chunk=0):
    off, succ = adj if isinstance(adj, tuple) else _csr(adj)
    n = len(off) - 1
    want = tools.store((off, succ), p, chunk_nodes=chunk)
    graph, offsets = W.store((off, succ), p, chunk_nodes=chunk)
    assert np.array_equal(offsets, want.offsets), "offsets differ from node %d on" % int(np.argmax(offsets != want.offsets))
    assert graph.tobytes() == want.graph.tobytes()
    q = p.clone(nodes=n, arcs=len(succ))
    deg, dec = oracle.Graph.from_memory(oracle.Params(**q.as_dict()), graph.tobytes(), offsets).decode_range(0, n)
    assert np.array_equal(deg, np.diff(off.astype(np.int64))) and np.array_equal(dec, succ)
    return want


def _chosen_references(st):
    """The reference field of every record, read from the stored bits themselves (gamma outdegree, then the reference in its own
    coding); 0 where the list is empty.  For streams with a window and a gamma-coded outdegree only."""
    bits = np.unpackbits(np.frombuffer(st.graph.tobytes(), np.uint8))
    p = st.params
    assert p.window_size > 0 and p.outdegree_coding == W_GAMMA

    def unary(pos):
        k = 0
        while not bits[pos + k]: k += 1
        return k, pos + k + 1

    def low_bits(pos, b):
        v = 1
        for i in range(b): v = 2 * v + int(bits[pos + i])
        return v - 1, pos + b

    def gamma(pos):
        b, pos = unary(pos)
        return low_bits(pos, b)

    def delta(pos):
        b, pos = gamma(pos)
        return low_bits(pos, b)

    refs = []
    for x in range(len(st.offsets) - 1):
        d, pos = gamma(int(st.offsets[x]))
        refs.append({W_UNARY: unary, W_GAMMA: gamma, W_DELTA: delta}[p.reference_coding](pos)[0] if d else 0)
    return refs


W_DELTA, W_GAMMA, W_UNARY = 1, 2, 5


@functools.lru_cache(maxsize=None)
def _far_graph(n, seed, dists=(65, 3, 97, 64, 127, 30, 63), members=3, empty_every=5):
    """Short random lists, every fifth one empty, and among them families of (nearly) equal 40-successor lists `d` nodes apart: the
    next member of a family costs some 300 bits on its own and d + a few bits as a copy, so its reference is the member before it
    whenever the window and the chunk reach that far.  Returns (lists, {node: distance of the family member before it})."""
    rng = np.random.default_rng(seed)
    lists = []
    for x in range(n):
        lo, hi = max(0, x - 40), min(n, x + 40)
        lists.append(np.unique(rng.integers(lo, hi, int(rng.integers(1, 4)))) if x % empty_every else np.empty(0, np.int64))
    taken, second, k = set(), {}, 0
    for pos in range(1, n, 3):
        d = dists[k % len(dists)]; k += 1
        where = [pos + j * d for j in range(members)]
        if where[-1] >= n or taken.intersection(where): continue
        taken.update(where)
        cur = np.unique(rng.integers(0, n, 40))
        for j, y in enumerate(where):
            if j and rng.random() < 0.5:                                       # a member may drop one successor and gain another
                cur = np.union1d(np.delete(cur, int(rng.integers(0, cur.size))), rng.integers(0, n, 1))
            lists[y] = cur.astype(np.int64)
        second[where[1]] = d
    return lists, second


def _assert_far_references_taken(st, second, window, chunk, least):
    """a test that never takes the branch proves nothing: the references the graph was built for are the ones the tooling chose"""
    refs = _chosen_references(st)
    chain = []                                                                 # (a member before it that a full reference chain bars is out of reach too)
    for x, r in enumerate(refs): chain.append(chain[x - r] + 1 if r else 0)
    max_ref = st.params.max_ref_count if st.params.max_ref_count >= 0 else len(refs)
    reach = [y for y, d in second.items() if d <= window and (chunk == 0 or (y - d) // chunk == y // chunk) and chain[y - d] < max_ref]
    assert all(refs[y] == second[y] for y in reach), [(y, second[y], refs[y]) for y in reach if refs[y] != second[y]]
    assert sum(1 for y in reach if second[y] >= 64) >= least, "the graph holds too few references beyond the first 64"


@pytest.mark.parametrize("chunk", [0, 50, 333])
@pytest.mark.parametrize("max_ref", [1, 3, -1])
@pytest.mark.parametrize("window", [63, 64, 65, 100, 127])
def test_windows_around_and_beyond_one_lane_group(W, tools, oracle, window, max_ref, chunk):
    lists, second = _far_graph(1000, seed=41)
    p = W.default_params(window_size=window, max_ref_count=max_ref)
    want = _held_to_tooling_and_oracle(W, tools, oracle, lists, p, chunk)
    least = 0 if window < 64 or chunk == 50 else 3 if chunk or window < 127 else 10
    _assert_far_references_taken(want, second, window, chunk, least)


def test_a_window_of_128_is_unsupported(W):
    with pytest.raises(W.UnsupportedOperationException):
        W.store([[1], [0]], W.default_params(window_size=128))
    W.store([[1], [0]], W.default_params(window_size=127))


def _runs_graph(m, n=240):
    """extras with isolated elements and runs of exactly m - 1, m and m + 1, at the start, in the middle and at the end of a list, lists
    that are one single run, and lists that copy their predecessor and add such runs"""
    run = lambda a, l: list(range(a, a + l))
    lists = [[5, 20, 40], [5, 20, 40, 77], [9]]
    for l in (m - 1, m, m + 1):
        if l < 1: continue
        lists += [[3] + run(10, l) + [60], run(0, l) + [30 + l, 70], [2, 9] + run(n - l, l), run(7, l), run(100, l),
                  [3] + run(10, l) + [60] + run(90, l) + [200], run(0, l) + run(l + 1, l) + run(2 * l + 3, l)]
    lists += [run(50, 2 * m + 1), run(50, 2 * m + 1) + [150], [1] + run(50, 2 * m + 1) + run(160, m), []]
    lists += [[x] for x in range(len(lists), n)]
    return lists


@pytest.mark.parametrize("window", [0, 7])
@pytest.mark.parametrize("m", [1, 2, 3, 9])
def test_min_interval_lengths_on_runs_of_every_kind(W, tools, oracle, m, window):
    """min_interval_length = 1 means runs of two or more (BVG:1599-1604: an interval is opened only by v[i] + 1 == v[i + 1]); a lone extra
    stays a residual.  A compressor that turns it into an interval of length 1 still round-trips: only the bytes tell."""
    _held_to_tooling_and_oracle(W, tools, oracle, _runs_graph(m), W.default_params(min_interval_length=m, window_size=window))


def test_min_interval_length_1_on_a_dense_graph(W, tools, oracle):
    adj = tools.synth_adjacency(1500, seed=23, synth=tools.eu_like(mean_deg=40.0), chunk_nodes=1 << 16)
    _held_to_tooling_and_oracle(W, tools, oracle, adj, W.default_params(min_interval_length=1))


_CHUNK_N = 1200


@pytest.mark.parametrize("window", [1, 7, 70])
@pytest.mark.parametrize("chunk", [1, 2, 3, 63, 64, 65, 997, _CHUNK_N - 1, _CHUNK_N, _CHUNK_N + 5])
def test_chunks_that_do_not_divide_the_graph(W, tools, oracle, chunk, window):
    lists, second = _far_graph(_CHUNK_N, seed=43, dists=(1, 65, 2, 7, 30, 70, 3))
    want = _held_to_tooling_and_oracle(W, tools, oracle, lists, W.default_params(window_size=window), chunk)
    _assert_far_references_taken(want, second, window, chunk if chunk < _CHUNK_N else 0, 0)


_SHAPES = {
    "eu_like": lambda tools: tools.synth_adjacency(1500, seed=23, synth=tools.eu_like(mean_deg=40.0), chunk_nodes=1 << 16),
    "web_like": lambda tools: tools.synth_adjacency(3000, seed=29, synth=tools.web_like(), chunk_nodes=1 << 16),
    "fuzz_900": lambda tools: _adjacency(np.random.default_rng(3), 900),
    "fuzz_6000": lambda tools: _adjacency(np.random.default_rng(4), 6000),
    "far": lambda tools: _csr(_far_graph(1500, seed=47)[0]),
}


@pytest.mark.parametrize("kw", [dict(), dict(window_size=100, max_ref_count=-1), dict(window_size=127, max_ref_count=2, min_interval_length=2),
                                dict(window_size=31, max_ref_count=0), dict(window_size=64, max_ref_count=50, min_interval_length=1)],
                         ids=["default", "w100_unbounded", "w127_r2_i2", "w31_r0", "w64_r50_i1"])
@pytest.mark.parametrize("chunk", [0, 100])
@pytest.mark.parametrize("shape", sorted(_SHAPES))
def test_shapes(W, tools, oracle, shape, chunk, kw):
    _held_to_tooling_and_oracle(W, tools, oracle, _SHAPES[shape](tools), W.default_params(**kw), chunk)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
@pytest.mark.parametrize("window,chunk", [(7, 0), (127, 0), (127, 64), (64, 63)])
def test_graphs_of_about_one_tile(W, tools, oracle, n, window, chunk):
    lists, second = _far_graph(n, seed=n, dists=(127, 65, 100, 30, 62, 5), members=2)
    # (gamma-coded references: in so small a graph a unary 127 would cost more than the list it saves)
    want = _held_to_tooling_and_oracle(W, tools, oracle, lists, W.default_params(window_size=window, reference_coding=W_GAMMA), chunk)
    _assert_far_references_taken(want, second, window, chunk, 1 if (n, window, chunk) == (129, 127, 0) else 0)


@pytest.mark.parametrize("coding", [W_GAMMA, W_DELTA])
@pytest.mark.parametrize("max_ref,chosen", [(3, 63), (1, 64)])
def test_equally_cheap_references_in_two_lane_groups(W, tools, oracle, coding, max_ref, chosen):
    """Node 100 repeats the lists of nodes 36 and 37: references 63 and 64 cost the same (gamma and delta code 63 and 64 in equally many
    bits) and sit in different groups of 64 lanes.  The nearest wins (BVG:2262: only a smaller size replaces the best) -- unless its
    chain is full (node 37 copies node 36: with max_ref_count = 1 it cannot be referenced), and then the far one is taken."""
    rng = np.random.default_rng(53)
    n = 200
    lists = [np.unique(rng.integers(0, n, 2)) for _ in range(n)]
    lists[36] = lists[37] = lists[100] = np.unique(rng.integers(0, n, 40))
    p = W.default_params(window_size=100, max_ref_count=max_ref, reference_coding=coding)
    want = _held_to_tooling_and_oracle(W, tools, oracle, lists, p)
    refs = _chosen_references(want)
    assert (refs[37], refs[100]) == (1, chosen)


def _long_list_graph(n=120000):
    rng = np.random.default_rng(59)
    lists = [np.array([(x * 7919 + 1) % n], np.int64) for x in range(n)]
    lists[10] = np.flatnonzero(rng.random(n) < 0.97)                           # intervals and residuals by the thousand
    lists[11] = lists[10][rng.random(lists[10].size) < 0.98]                   # long copy blocks
    lists[12] = np.union1d(lists[11][::2], np.arange(500, 900))
    lists[13] = np.arange(n)                                                   # one single run
    assert lists[10].size >= 100000
    return _csr(lists)


@pytest.mark.parametrize("kw", [dict(), dict(min_interval_length=0), dict(block_coding=W_UNARY, block_count_coding=W_UNARY, min_interval_length=1)],
                         ids=["default", "no_intervals", "unary_blocks_i1"])
def test_one_list_of_over_100000_successors(W, tools, oracle, kw):
    _held_to_tooling_and_oracle(W, tools, oracle, _long_list_graph(), W.default_params(**kw), chunk=0)


def _copy_block_graph(n=400):
    """lists of some 300 successors that copy their predecessor but for a few holes: copy blocks of 10 to 200"""
    rng = np.random.default_rng(61)
    lists = [np.unique(rng.integers(0, n, 300))]
    for x in range(1, n):
        prev = lists[-1]
        keep = np.ones(prev.size, bool); keep[rng.integers(0, prev.size, int(rng.integers(0, 6)))] = False
        lists.append(np.union1d(prev[keep], rng.integers(0, n, int(rng.integers(0, 4)))) if x % 50 else np.unique(rng.integers(0, n, 300)))
    return lists


@pytest.mark.parametrize("kw", [dict(residual_coding=6, zeta_k=1), dict(residual_coding=6, zeta_k=7),
                                dict(residual_coding=3, zeta_k=1), dict(residual_coding=3, zeta_k=2), dict(residual_coding=3, zeta_k=8),
                                dict(residual_coding=7), dict(residual_coding=2), dict(residual_coding=1),
                                dict(block_coding=5, block_count_coding=5), dict(block_coding=5, block_count_coding=5, window_size=70, max_ref_count=-1),
                                dict(block_coding=1, block_count_coding=1, reference_coding=1, outdegree_coding=1)],
                         ids=["zeta1", "zeta7", "golomb1", "golomb2", "golomb8", "nibble", "gamma", "delta", "unary_blocks", "unary_blocks_w70", "all_delta"])
@pytest.mark.parametrize("graph", ["eu_like", "copy_blocks"])
def test_every_coding_at_its_edge_parameter(W, tools, oracle, graph, kw):
    adj = _SHAPES["eu_like"](tools) if graph == "eu_like" else _csr(_copy_block_graph())
    _held_to_tooling_and_oracle(W, tools, oracle, adj, W.default_params(**kw), chunk=0 if graph == "eu_like" else 97)
