"""GPU: EFGraph on the device (bvg_ef_*) against the model of tests/efgraph_model.py and the adjacency each test writes down: load,
outdegrees, decode, random access, scan, skipTo, refusals, and the device store byte for byte against the model's writer.
Shapes are the smallest at which the kernels can go wrong (word edges of every part of a record, both decode paths and their threshold,
one / several blocks and prefix-sum levels)."""
import ctypes as C
import os

import numpy as np
import pytest

import efgraph_model as M

pytestmark = pytest.mark.gpu

PACKED, CHUNKED = "1", "2"
_ENC = {}


def encode(key, lists, U, q, order="LITTLE_ENDIAN"):
    """The model's stream of `lists` (cached by `key`: the model is plain Python)."""
    k = (key, U, q, order)
    if k not in _ENC:
        _ENC[k] = M.store(lists, U, q, order)
    return _ENC[k]


def small_lists(n=150, seed=5):
    return M.random_lists(n, 10 * n, seed=seed, degrees=(0, 1, 2, 3, 63, 64, 65, min(n, 150)))


def params(W, n, arcs, U, q, order="LITTLE_ENDIAN"):
    return W.EFParams(nodes=n, arcs=arcs, upper_bound=U, log2_quantum=q, big_endian=int(order == "BIG_ENDIAN"))


def open_model(W, key, lists, U, q, order="LITTLE_ENDIAN", offsets=True):
    data, off, info = encode(key, lists, U, q, order)
    return W.EFGraph.from_memory(params(W, len(lists), info["arcs"], U, q, order), data, off if offsets else None)


def flat(lists):
    return np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if sum(len(l) for l in lists) else np.empty(0, np.int64)


def check_graph(g, lists, scan=True):
    n = len(lists)
    deg, succ = g.decode_range(0, n)
    assert np.array_equal(deg, [len(l) for l in lists])
    assert np.array_equal(succ, flat(lists))
    assert np.array_equal(g.outdegrees(), deg)
    if scan:
        r = g.scan()
        assert (r["nodes"], r["arcs"], r["chk"]) == (n, len(succ), M.scan_checksum(lists))


@pytest.mark.parametrize("ub", ["n", "n+7", "n2"])
@pytest.mark.parametrize("q", range(9))
def test_grid_of_quanta_and_upper_bounds(W, q, ub):
    """d in {0, 1, 2, 3, 63, 64, 65, n} among random lists; q = 0..8 gives P = 0 and P > 0 on tiny lists; sub-ranges and the last node."""
    n = 150
    lists = small_lists(n)
    U = {"n": n, "n+7": n + 7, "n2": n * n}[ub]
    g = open_model(W, "small", lists, U, q)
    assert (g.num_nodes(), g.upper_bound(), g.log2_quantum(), g.num_arcs()) == (n, U, q, sum(len(l) for l in lists))
    check_graph(g, lists)
    for a, b in ((0, 1), (3, 9), (64, 150), (149, 150), (7, 7)):
        deg, succ = g.decode_range(a, b)
        assert np.array_equal(deg, [len(l) for l in lists[a:b]]) and np.array_equal(succ, flat(lists[a:b]))
        r = g.scan(a, b)
        assert (r["nodes"], r["arcs"], r["chk"]) == (b - a, len(succ), sum(M.arc_mix(x, int(y)) for x in range(a, b) for y in lists[x]) & M.M64)
    off = g.offsets()
    r = g.scan(3, 9)
    assert r["graph_bytes"] == 8 * (((int(off[9]) - 1) >> 6) - (int(off[3]) >> 6) + 1) and r["index_bytes"] == 8 * 7
    g.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_node_counts_around_wavefront_and_block_edges(W, n):
    lists = M.random_lists(n, 6 * n, seed=n)
    g = open_model(W, ("count", n), lists, n, 2)
    check_graph(g, lists)
    g.close()


@pytest.fixture(scope="module")
def big():
    """70 000 nodes, about 2 10^5 arcs, a few long lists among them: several blocks, every level of the prefix sum, both decode paths."""
    n = 70000
    rng = np.random.default_rng(11)
    degs = rng.poisson(2.7, size=n)
    pool = rng.integers(0, n, size=int(degs.sum()))
    cuts = np.concatenate([[0], np.cumsum(degs)])
    lists = [np.unique(pool[cuts[x]:cuts[x + 1]]).astype(np.int64) for x in range(n)]
    for x, d in ((17, 5000), (40000, 3000), (69999, 2500)):
        lists[x] = np.sort(rng.choice(n, size=d, replace=False)).astype(np.int64)
    return lists


def test_70000_nodes(W, big, monkeypatch):
    g = open_model(W, "big", big, len(big), 3)
    check_graph(g, big)
    deg, succ = g.decode_range(39990, 40010)
    assert np.array_equal(succ, flat(big[39990:40010]))
    for path in (PACKED, CHUNKED):
        monkeypatch.setenv("BVG_EF_PATH", path)
        check_graph(g, big)
    g.close()


def test_all_empty_graph(W):
    for n in (1, 64, 1000):
        lists = [[] for _ in range(n)]
        g = open_model(W, ("empty", n), lists, n, 3)
        check_graph(g, lists)
        assert np.array_equal(g.skip_to(np.arange(n), np.zeros(n, np.int64)), np.full(n, -1))
        g.close()


@pytest.mark.parametrize("d", [4095, 4096, 4097])
def test_one_long_list_chunk_carry(W, d, monkeypatch):
    """One list of d successors in an 8 192-node graph: 8192 + d + 1 upper bits = more than three chunks of the chunked kernel, and more than
    three wavefronts of the packed one."""
    n = 8192
    rng = np.random.default_rng(d)
    lists = [[] for _ in range(n)]
    lists[100] = np.sort(rng.choice(n, size=d, replace=False)).astype(np.int64)
    lists[101] = np.array([5, 8191], dtype=np.int64)
    lists[8191] = np.array([0], dtype=np.int64)
    g = open_model(W, ("long", d), lists, n, 8)
    for path in (None, PACKED, CHUNKED):
        if path:
            monkeypatch.setenv("BVG_EF_PATH", path)
        check_graph(g, lists)
        deg, succ = g.successors_batch([100, 8191, 100])
        assert np.array_equal(deg, [d, 1, d]) and np.array_equal(succ, np.concatenate([lists[100], lists[8191], lists[100]]))
    g.close()


@pytest.mark.parametrize("n,d,bits", [(40, 22, 63), (40, 23, 64), (40, 24, 65), (80, 47, 128)])
def test_upper_regions_ending_at_word_edges(W, n, d, bits, monkeypatch):
    """Every node has outdegree d, l = 0, so every upper region is exactly `bits` long; records of one length land on every bit of a word."""
    assert M.lower_bits(d + 1, n) == 0 and n + d + 1 == bits
    rng = np.random.default_rng(bits)
    lists = [np.sort(rng.choice(n, size=d, replace=False)).astype(np.int64) for _ in range(n)]
    g = open_model(W, ("region", bits), lists, n, 1)
    for path in (None, CHUNKED):
        if path:
            monkeypatch.setenv("BVG_EF_PATH", path)
        check_graph(g, lists)
    g.close()


def _lists_with_offset(target_mod, want_total_mod=None):
    """Lists whose node 20 starts on bit `target_mod` of a word (and, optionally, whose stream is a whole number of words)."""
    n, U, q = 64, 64, 2
    rng = np.random.default_rng(3)
    bits = [M.record_bits(d, U, q) for d in range(9)]
    while True:
        head = rng.integers(0, 9, size=21)
        if sum(bits[d] for d in head[:20]) % 64 == target_mod and head[20] >= 4:
            break
    while True:
        tail = rng.integers(0, 9, size=n - 21)
        if want_total_mod is None or sum(bits[d] for d in np.concatenate([head, tail])) % 64 == want_total_mod:
            break
    return [np.sort(rng.choice(n, size=int(d), replace=False)).astype(np.int64) for d in np.concatenate([head, tail])], U, q


def test_record_starting_on_bit_63(W):
    lists, U, q = _lists_with_offset(63)
    data, off, _ = M.store(lists, U, q)
    assert int(off[20]) % 64 == 63                                            # (the unary part of gamma(d >= 4) crosses the word edge)
    g = W.EFGraph.from_memory(params(W, len(lists), -1, U, q), data, off)
    check_graph(g, lists)
    g2 = W.EFGraph.from_memory(params(W, len(lists), -1, U, q), data, None)
    assert np.array_equal(g2.offsets(), off)
    check_graph(g2, lists)
    g.close(); g2.close()


def test_stream_of_a_whole_number_of_words(W):
    lists, U, q = _lists_with_offset(63, want_total_mod=0)
    data, off, _ = M.store(lists, U, q)
    assert int(off[-1]) % 64 == 0 and len(data) == int(off[-1]) // 8 + 8      # the extra word
    for o in (off, None):
        g = W.EFGraph.from_memory(params(W, len(lists), -1, U, q), data, o)
        check_graph(g, lists)
        g.close()
    g = W.EFGraph.from_memory(params(W, len(lists), -1, U, q), data[:-8], off)   # the records themselves end with the last full word
    check_graph(g, lists)
    g.close()


def test_lower_bits_zero_thirteen_and_above_32(W):
    n = 200
    lists = M.random_lists(n, 12 * n, seed=21, degrees=(99, 0, 200, 1, 99))
    full = [np.arange(10, dtype=np.int64) for _ in range(10)]                  # d + 1 > U: l = 0
    assert M.lower_bits(11, 10) == 0
    g = open_model(W, "full", full, 10, 0)
    check_graph(g, full)
    g.close()
    assert M.lower_bits(100, 1 << 20) == 13 and M.lower_bits(100, 1 << 40) == 33 and M.lower_bits(1, 1 << 40) == 40
    for U in (1 << 20, 1 << 40):                                               # 100 fields of 13 / 33 bits: most straddle a word edge
        for q in (0, 8):
            g = open_model(W, "wide", lists, U, q)
            check_graph(g, lists)
            nodes = np.repeat(np.arange(n), 5); bounds = np.tile(np.array([0, 1, 57, 150, 199]), n)
            model = M.Graph(n, U, q, *encode("wide", lists, U, q)[:2])
            want = [model.skip_to(int(x), int(b)) for x, b in zip(nodes, bounds)]
            assert np.array_equal(g.skip_to(nodes, bounds), want)
            g.close()


def test_successors_batch_repeats_and_both_paths(W, monkeypatch):
    lists = small_lists()
    g = open_model(W, "small", lists, 150, 3)
    rng = np.random.default_rng(8)
    nodes = np.concatenate([[7, 7, 149, 0, 7, 4, 5, 6, 4], rng.integers(0, 150, size=300)])
    for path in (None, PACKED, CHUNKED):
        if path:
            monkeypatch.setenv("BVG_EF_PATH", path)
        deg, succ = g.successors_batch(nodes)
        assert np.array_equal(deg, [len(lists[x]) for x in nodes]) and np.array_equal(succ, flat([lists[x] for x in nodes]))
    deg, succ = g.successors_batch([])
    assert len(deg) == 0 and len(succ) == 0
    with pytest.raises(W.IllegalArgumentException):
        g.successors_batch([0, 150])
    with pytest.raises(W.IllegalArgumentException):
        g.successors_batch([-1])
    g.close()


@pytest.mark.parametrize("q", [0, 1, 3, 8])
@pytest.mark.parametrize("ub", ["n", "n+7", "n2"])
def test_skip_to_every_bound_of_every_node(W, q, ub, monkeypatch):
    """Against a linear search in the adjacency (EFGraphTest.testSkipFirst), with the pointers and with BVG_EF_NOPTR=1."""
    n = 150
    lists = small_lists(n)
    U = {"n": n, "n+7": n + 7, "n2": n * n}[ub]
    g = open_model(W, "small", lists, U, q)
    nodes = np.repeat(np.arange(n), n + 2); bounds = np.tile(np.arange(-1, n + 1), n)
    want = np.empty(len(nodes), np.int64)
    for x in range(n):
        a = np.asarray(lists[x])
        i = np.searchsorted(a, np.arange(-1, n + 1))
        want[x * (n + 2):(x + 1) * (n + 2)] = np.where(i < len(a), np.append(a, -1)[np.minimum(i, len(a))], -1)
    assert np.array_equal(g.skip_to(nodes, bounds), want)
    monkeypatch.setenv("BVG_EF_NOPTR", "1")
    assert np.array_equal(g.skip_to(nodes, bounds), want)
    monkeypatch.delenv("BVG_EF_NOPTR")
    far = np.array([U, U + 1, 1 << 62], dtype=np.int64)
    assert np.array_equal(g.skip_to(np.full(3, 7), far), [-1, -1, -1])
    with pytest.raises(W.IllegalArgumentException):
        g.skip_to([n], [0])
    g.close()


def test_skip_to_long_lists_uses_pointers(W, big, monkeypatch):
    """Lists long enough that bound >> l passes many quanta: the pointer route and the plain walk agree with the adjacency."""
    n = len(big)
    g = open_model(W, "big", big, n, 3)
    rng = np.random.default_rng(2)
    nodes = np.concatenate([np.full(2000, 17), np.full(2000, 40000), rng.integers(0, n, size=4000)])
    bounds = rng.integers(0, n, size=len(nodes))
    want = np.array([(lambda a, i: int(a[i]) if i < len(a) else -1)(big[x], int(np.searchsorted(big[x], b))) for x, b in zip(nodes, bounds)])
    assert np.array_equal(g.skip_to(nodes, bounds), want)
    monkeypatch.setenv("BVG_EF_NOPTR", "1")
    assert np.array_equal(g.skip_to(nodes, bounds), want)
    g.close()


def test_scan_equals_bvgraph_scan_of_the_same_adjacency(W, big):
    g = open_model(W, "big", big, len(big), 3)
    bytes_, offs = W.store(big)
    bv = W.BVGraph.from_memory(W.default_params(nodes=len(big), arcs=sum(len(l) for l in big)), bytes_, offs)
    r, b = g.scan(), bv.scan()
    assert (r["nodes"], r["arcs"], r["chk"]) == (b["nodes"], b["arcs"], b["chk"])
    r, b = g.scan(1000, 50000), bv.scan(1000, 50000)
    assert (r["nodes"], r["arcs"], r["chk"]) == (b["nodes"], b["arcs"], b["chk"])
    assert r["kernel_ms"] > 0 and r["launches"] >= 4 and r["slow_blocks"] == r["lean_blocks"] == r["index_entries"] == 0
    g.close(); bv.close()


def test_capacity_contract(W):
    lists = small_lists()
    g = open_model(W, "small", lists, 150, 3)
    L = W.lib()
    total = sum(len(l) for l in lists)
    need = C.c_uint64(0)
    deg = np.full(150, -7, np.int32); succ = np.full(total, -7, np.int64)
    assert L.bvg_ef_decode_range(g._h, 0, 150, deg.ctypes.data, None, 0, C.byref(need)) == W.E_CAPACITY and need.value == total
    assert L.bvg_ef_decode_range(g._h, 0, 150, deg.ctypes.data, succ.ctypes.data, total - 1, C.byref(need)) == W.E_CAPACITY and need.value == total
    assert np.all(succ == -7)                                                  # nothing written
    assert L.bvg_ef_decode_range(g._h, 0, 150, None, succ.ctypes.data, total, C.byref(need)) == 0 and np.array_equal(succ, flat(lists))
    nodes = np.array([7, 7], np.int64)
    assert L.bvg_ef_successors_batch(g._h, nodes.ctypes.data, 2, deg.ctypes.data, succ.ctypes.data, 2 * len(lists[7]) - 1, C.byref(need)) == W.E_CAPACITY
    assert need.value == 2 * len(lists[7])
    assert L.bvg_ef_decode_range(g._h, 1, 1, None, None, 0, C.byref(need)) == 0 and need.value == 0     # node 1 is empty; so is the range
    assert L.bvg_ef_decode_range(g._h, 5, 4, None, None, 0, C.byref(need)) == W.E_ARG
    assert L.bvg_ef_decode_range(g._h, 0, 151, None, None, 0, C.byref(need)) == W.E_ARG
    with pytest.raises(W.IllegalArgumentException):
        g.outdegrees(0, 151)
    g.close()


def test_offsets_derived_big_endian_copies_and_files(W, tmp_path):
    lists = small_lists()
    n, U, q = 150, 157, 2
    le, off, info = encode("small", lists, U, q)
    be = encode("small", lists, U, q, "BIG_ENDIAN")[0]
    g = open_model(W, "small", lists, U, q, offsets=False)
    assert np.array_equal(g.offsets(), off)
    check_graph(g, lists)
    b = open_model(W, "small", lists, U, q, "BIG_ENDIAN")
    check_graph(b, lists)
    c = g.copy()
    g.close()                                                                  # a flyweight outlives the handle it was copied from
    check_graph(c, lists)
    assert np.array_equal(c.skip_to([4, 4], [0, 149]), [lists[4][0], -1 if lists[4][-1] < 149 else 149])
    c.close(); b.close()
    for order, data in (("LITTLE_ENDIAN", le), ("BIG_ENDIAN", be)):
        base = str(tmp_path / order)
        open(base + ".graph", "wb").write(data)
        open(base + ".offsets", "wb").write(M.write_delta_offsets(off))
        open(base + ".properties", "w").write("#EFGraph properties\nnodes=%d\narcs=%d\nupperbound=%d\nquantum=%d\nbyteorder=%s\ngraphclass=it.unimi.dsi.big.webgraph.EFGraph\nversion=0\n"
                                              % (n, info["arcs"], U, 1 << q, order))
        for mode in (W.LOAD_STANDARD, W.LOAD_MAPPED, W.LOAD_SEQUENTIAL, W.LOAD_OFFLINE):
            f = W.EFGraph.load(base, mode=mode)
            assert (f.num_arcs(), f.upper_bound(), f.log2_quantum()) == (info["arcs"], U, q) and np.array_equal(f.offsets(), off)
            check_graph(f, lists, scan=mode == W.LOAD_STANDARD)
            f.close()
        os.remove(base + ".offsets")
        with pytest.raises(W.IOException):
            W.EFGraph.load(base)
        W.EFGraph.load(base, mode=W.LOAD_OFFLINE).close()


def _body_device_buffers(W, torch):
    lists = small_lists()
    total = sum(len(l) for l in lists)
    data, off, info = encode("small", lists, 150, 3)
    words = torch.from_numpy(np.frombuffer(data, dtype=np.int64).copy()).cuda()
    offs = torch.from_numpy(off.astype(np.int64)).cuda()
    g = W.EFGraph.from_device(params(W, 150, info["arcs"], 150, 3), words.data_ptr(), len(data), offs.data_ptr(), keep=(words,))
    del offs                                                                   # the offsets were copied
    check_graph(g, lists)
    L = W.efgraph._ef_fns()
    d_deg = torch.full((150,), -7, dtype=torch.int32, device="cuda"); d_succ = torch.full((total + 3,), -7, dtype=torch.int64, device="cuda"); need = C.c_uint64()
    assert L.bvg_ef_decode_range_dev(g._h, 0, 150, d_deg.data_ptr(), d_succ.data_ptr(), total - 1, C.byref(need)) == W.E_CAPACITY and need.value == total
    torch.cuda.synchronize()
    assert bool((d_succ == -7).all())
    assert L.bvg_ef_decode_range_dev(g._h, 0, 150, d_deg.data_ptr(), d_succ.data_ptr(), total + 3, C.byref(need)) == 0 and need.value == total
    torch.cuda.synchronize()
    assert np.array_equal(d_deg.cpu().numpy(), [len(l) for l in lists]) and np.array_equal(d_succ.cpu().numpy()[:total], flat(lists))
    assert bool((d_succ[total:] == -7).all())                                  # nothing behind the last list
    for bad in (params(W, 150, info["arcs"], 150, 3, "BIG_ENDIAN"), ):
        with pytest.raises(W.IllegalArgumentException):
            W.EFGraph.from_device(bad, words.data_ptr(), len(data), words.data_ptr())
    with pytest.raises(W.IllegalArgumentException):
        W.EFGraph.from_device(params(W, 150, info["arcs"], 150, 3), words.data_ptr(), len(data) - 1, words.data_ptr())
    g.close()


def test_words_and_outputs_on_the_device():
    """torch tensors: in a fresh child process that imports torch before the product library (one HIP runtime: tests/test_gpu_device_buffers.py)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "device_buffers"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _raw_decode(W, g, a, b, cap):
    deg = np.full(max(b - a, 1), -7, np.int32); succ = np.full(max(cap, 1), -7, np.int64); need = C.c_uint64(0)
    st = W.lib().bvg_ef_decode_range(g._h, a, b, deg.ctypes.data, succ.ctypes.data, cap, C.byref(need))
    return st, deg[:b - a], succ[:cap], int(need.value)


def test_refusals_leave_healthy_requests_right(W, monkeypatch):
    lists = small_lists()
    n, U, q = 150, 150, 2
    data, off, info = encode("small", lists, U, q)
    total = info["arcs"]
    p = params(W, n, total, U, q)
    victim = 64                                                                 # any node with successors, away from the ends
    assert len(lists[victim]) >= 3
    before = sum(len(l) for l in lists[:victim])

    # (a) wrong offsets: one entry moved by a bit -- the two records beside it fail the length check
    bad_off = off.copy(); bad_off[victim] += 1
    g = W.EFGraph.from_memory(p, data, bad_off)
    st, deg, succ, _ = _raw_decode(W, g, 0, n, total)
    assert st == W.E_EOF and np.all(succ == -7) and np.all(deg == -7)           # nothing written
    with pytest.raises(W.EOFException):
        g.scan()
    with pytest.raises(W.EOFException):
        g.skip_to([victim], [0])
    with pytest.raises(W.EOFException):
        g.successors_batch([3, victim])
    for a, b in ((0, victim - 1), (victim + 1, n)):                             # the ranges beside them
        d, s = g.decode_range(a, b)
        assert np.array_equal(s, flat(lists[a:b]))
    assert np.array_equal(g.successors_batch([3, 149])[1], flat([lists[3], lists[149]]))
    assert np.array_equal(g.skip_to([3], [0]), [lists[3][0]])
    g.close()

    # (b) a flipped bit in gamma(d): the closed form no longer matches the offsets
    words = np.frombuffer(data, dtype="<u8").copy()
    pos = int(off[victim])                                                      # the first bit of the unary part
    words[pos >> 6] ^= np.uint64(1 << (pos & 63))
    g = W.EFGraph.from_memory(p, words.tobytes(), off)
    st, deg, succ, _ = _raw_decode(W, g, 0, n, total)
    assert st in (W.E_EOF, W.E_UNSUPPORTED) and np.all(succ == -7)
    d, s = g.decode_range(victim + 1, n)
    assert np.array_equal(s, flat(lists[victim + 1:]))
    d, s = g.decode_range(0, victim)
    assert np.array_equal(s, flat(lists[:victim]))
    with pytest.raises(W.EOFException):
        W.EFGraph.from_memory(p, words.tobytes()[:int(off[victim]) // 8], None)  # a truncated stream cannot be derived
    g.close()

    # (c) an upper region with two ones removed: BVG_E_EOF, the slot no one is left for is -1, every other list of the call is intact
    d_v = len(lists[victim])
    l = M.lower_bits(d_v + 1, U)
    upper = int(off[victim + 1]) - ((U >> l) + d_v + 1)
    words = np.frombuffer(data, dtype="<u8").copy()
    for e in (1, 2):                                                            # remove the ones of elements 1 and 2: d - 1 ones are left
        bit = upper + (int(lists[victim][e]) >> l) + e
        assert (int(words[bit >> 6]) >> (bit & 63)) & 1
        words[bit >> 6] ^= np.uint64(1 << (bit & 63))
    g = W.EFGraph.from_memory(p, words.tobytes(), off)
    for path in (None, PACKED, CHUNKED):
        if path:
            monkeypatch.setenv("BVG_EF_PATH", path)
        st, deg, succ, need = _raw_decode(W, g, 0, n, total)
        assert st == W.E_EOF and need == total and np.array_equal(deg, [len(x) for x in lists])
        assert np.array_equal(succ[:before], flat(lists[:victim])) and np.array_equal(succ[before + d_v:], flat(lists[victim + 1:]))
        mine = succ[before:before + d_v]
        assert mine[-1] == -1 and mine[0] == lists[victim][0] and np.all(mine[:-1] >= 0) and np.all(mine[:-1] < (1 << 62))
        with pytest.raises(W.EOFException):
            g.scan()
        assert np.array_equal(g.decode_range(victim + 1, n)[1], flat(lists[victim + 1:]))
    g.close()


# ---------------------------------------------------------------- store

@pytest.mark.parametrize("ub", ["n", "n+7", "n2", "2^40"])
@pytest.mark.parametrize("q", range(9))
def test_store_byte_exact(W, q, ub):
    n = 150
    lists = small_lists(n)
    U = {"n": n, "n+7": n + 7, "n2": n * n, "2^40": 1 << 40}[ub]
    for order in ("LITTLE_ENDIAN", "BIG_ENDIAN"):
        data, off, _ = encode("small", lists, U, q, order)
        graph, offsets = W.store_efgraph(lists, U, q, order)
        assert np.array_equal(offsets, off)
        assert graph.tobytes() == data


def test_store_shapes(W, big):
    cases = [("big", big, len(big), 3)]
    for d in (4095, 4097):
        n = 8192
        lists = [[] for _ in range(n)]
        lists[100] = np.sort(np.random.default_rng(d).choice(n, size=d, replace=False)).astype(np.int64)
        lists[101] = np.array([5, 8191], dtype=np.int64); lists[8191] = np.array([0], dtype=np.int64)
        cases.append((("long", d), lists, n, 8))
    cases += [(("empty", 64), [[] for _ in range(64)], 64, 3), ("full", [np.arange(10, dtype=np.int64) for _ in range(10)], 10, 0), (("none", 0), [], 0, 4)]
    for key, lists, U, q in cases:
        data, off, _ = encode(key, lists, U, q)
        graph, offsets = W.store_efgraph(lists, U, q)
        assert np.array_equal(offsets, off) and graph.tobytes() == data, key
    lists, U, q = _lists_with_offset(63, want_total_mod=0)                     # the extra word
    data, off, _ = M.store(lists, U, q)
    graph, offsets = W.store_efgraph(lists, U, q)
    assert graph.tobytes() == data and len(graph) == int(off[-1]) // 8 + 8


def test_store_refusals(W):
    ok = ([0, 2, 3], [0, 1, 1])
    W.store_efgraph((np.array(ok[0], np.uint64), np.array(ok[1], np.int64)))
    for off, succ in (([1, 2, 3], [0, 1, 1]), ([0, 2, 1], [0, 1, 1]), ([0, 2, 3], [1, 0, 1]), ([0, 2, 3], [0, 0, 1]), ([0, 2, 3], [0, 2, 1]), ([0, 2, 3], [-1, 1, 1])):
        with pytest.raises(W.IllegalArgumentException):
            W.store_efgraph((np.array(off, np.uint64), np.array(succ, np.int64)))
    with pytest.raises(W.IllegalArgumentException):
        W.store_efgraph([[0], [1]], upper_bound=1)                             # upper_bound < nodes
    with pytest.raises(W.IllegalArgumentException):
        W.store_efgraph([[0], [1]], log2_quantum=-1)
    with pytest.raises(W.IllegalArgumentException):
        W.store_efgraph([[0], [1]], byteorder="MIDDLE_ENDIAN")


def test_cnr_2000_round_trip(W, cnr_golden, tmp_path):
    """BV load -> to_efgraph (files written) -> EF load: the lists are the golden's, the scan is the BV scan's."""
    from conftest import CNR
    bv = W.BVGraph.load(CNR)
    base = str(tmp_path / "cnr-ef")
    ef = bv.to_efgraph(basename=base, batch_arcs=1 << 20)
    n = bv.num_nodes()
    assert ef.num_nodes() == n and ef.num_arcs() == bv.num_arcs()
    loaded = W.EFGraph.load(base)
    props = dict(l.strip().split("=", 1) for l in open(base + ".properties") if "=" in l)
    assert props["graphclass"] == "it.unimi.dsi.big.webgraph.EFGraph" and props["quantum"] == "256" and props["byteorder"] == "LITTLE_ENDIAN" and "upperbound" not in props
    assert int(props["bitsforoutdegrees"]) + int(props["bitsforsuccessors"]) == int(loaded.offsets()[-1])
    assert props["bitspernode"] == W.efgraph._format3(os.path.getsize(base + ".graph") * 8 / n)
    for g in (ef, loaded):
        deg, succ = g.decode_range(0, n)
        assert np.array_equal(deg, [len(a) for a in cnr_golden]) and np.array_equal(succ, np.concatenate(cnr_golden))
    r, b = loaded.scan(), bv.scan()
    assert (r["nodes"], r["arcs"], r["chk"]) == (b["nodes"], b["arcs"], b["chk"])
    assert W.efgraph_main(["-q", "4", base, str(tmp_path / "again")]) == 0      # EFGraph -> EFGraph with another quantum
    again = W.EFGraph.load(str(tmp_path / "again"))
    assert again.log2_quantum() == 4 and again.scan()["chk"] == b["chk"]
    assert W.efgraph_main([base]) == 1                                          # no destination: a message, not a crash
    for g in (ef, loaded, again, bv):
        g.close()


if __name__ == "__main__":
    import sys
    import torch                                                              # (before the product library)
    torch.cuda.init()
    _HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_HERE), _HERE]
    os.environ.setdefault("BVG_TEST_KNOBS", "1")
    import webgraph_big_amd
    globals()["_body_" + sys.argv[1]](webgraph_big_amd, torch)
    print("CHILD OK")
