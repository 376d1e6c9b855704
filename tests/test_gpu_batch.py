"""GPU: random access -- bvg_successors_batch, and the frontier route of bvg_bfs_visit that runs the same body -- differentially, list for
list: outdegree_gather_kernel, plan_halo_kernel on a per-call plan, batch_deep_kernel and the one-by-one decode of the requests it takes
out, the a.batch branches of the row, giant and generic kernels, the shared prefix sum, the second prepare() when the workspace moves.

Every test compares outdegrees AND successors with batch_cases.expected(): the adjacency the test itself wrote down (for the
hand-assembled streams: the pure-Python iterators of tests/bvrecords.py, held against the oracle's decode of the same bytes in
test_hand_assembled_streams_decode_as_written).  Where a test says "reach" it has read it back from the stream with
batch_cases.own_reach(); nothing here asserts which route the library took, except the `deep` counter of item 10.

FOUND: no wrong list, outdegree or status at this commit.
Two things these comparisons cannot see, found by mutating the library:
- The order in which the deep requests are decoded.  batch_halos (csrc/bvg_api.hip) sorts the list batch_deep_kernel wrote, but the loop
  that decodes it reads nodes[q.index] and writes at succ + q.at for every entry by itself, and so does the frontier route
  (csrc/bvg_bfs.hip): without the sort every list, outdegree and count is the same.  The order only decides WHICH status a call returns
  when two deep requests of one batch fail differently, which no stream here does.  No test can fail on it; an open question for the
  library is whether the sort should stay at all.
- A missing second preparation after the workspace moved reads the freed workspace, whose values are usually still there: every list
  comes out right.  tests/emu/batch_replay.cpp replays the calls of test_workspace_growth_between_the_two_preparations as a program of
  its own under AddressSanitizer (tests/test_emu.py::test_workspace_growth_replayed_under_address_sanitizer, opt-in: BVG_EMU_ASAN=1)."""
import ctypes as C

import numpy as np
import pytest

import batch_cases as BC
from bvrecords import PyBits, Record, assemble
from test_gpu_bfs import cpu_bfs, csr_of_lists

pytestmark = pytest.mark.gpu

K = BC.constants()
H = K["max_halo"]                                          # 64: reaches up to H fit a request block, H + 1 and more do not
REACHES = (0, 1, 2, H - 2, H - 1, H, H + 1, H + 2, 2 * H - 1, 2 * H, 2 * H + 1, 200)
SEGMENTS = [(r, k) for r in REACHES for k in ("wide", "ones", "mixed")]
KNOBS = ("BVG_GIANT", "BVG_NOSKIP", "BVG_EMIT", "BVG_DBG", "BVG_BFS_ROUTE", "BVG_BFS_BATCH_ARCS", "BVG_BFS_SMALL")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


class Hand:
    def __init__(self, W, w):
        self.st, self.ends = BC.chain_stream(W, w, SEGMENTS, seed=1, min_nodes=4200 if w == 7 else 0)
        self.reach = BC.reaches(self.st)
        self.n = int(self.st.params.nodes)
        self.deg = np.array([len(l) for l in self.st.lists])
        # requests whose own chain is short while a chain of the next window - 1 nodes passes H or more nodes behind them
        self.beside = [x for x in range(self.n) if self.reach[x] < H and BC.beyond_a_block(self.st, self.reach, x)]
        self.deep = [x for x in range(self.n) if self.reach[x] > H]
        self.ordinary = [x for x in range(self.n) if not BC.beyond_a_block(self.st, self.reach, x)]


@pytest.fixture(scope="module")
def hand(W):
    made = {}
    def get(w):
        if w not in made:
            made[w] = Hand(W, w)
        return made[w]
    return get


def _open(W, st, **tuning):
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    if tuning:
        g.set_tuning(**tuning)
    return g


@pytest.mark.parametrize("w", BC.HAND_WINDOWS)
def test_hand_assembled_streams_decode_as_written(W, oracle, hand, w):
    """The reference of the hand-assembled cases, checked once: the oracle reads the same bytes as the iterators of tests/bvrecords.py,
    sequentially and by random access, and the stream holds the reaches the tests rely on (own_reach and the one-pass reaches() agree)."""
    h = hand(w)
    og = oracle.Graph.from_memory(oracle.Params(**h.st.params.as_dict()), h.st.graph.tobytes(), h.st.offsets)
    deg, succ = og.decode_range(0, h.n)
    assert deg.tolist() == [len(l) for l in h.st.lists] and succ.tolist() == [v for l in h.st.lists for v in l]
    for x in h.ends:
        assert og.successors(x).tolist() == h.st.lists[x]
    assert [int(h.reach[e]) for e in h.ends] == [r for r, _ in SEGMENTS]
    assert all(BC.own_reach(h.st.params, h.st.graph, h.st.offsets, x) == h.reach[x] for x in h.ends + h.beside[:10])
    hops = set()
    for (r, kind), e in zip(SEGMENTS, h.ends):
        hops.update((kind, v) for v in BC.hops_of(kind, r, w))
    assert ("wide", w) in hops and ("ones", 1) in hops and {("mixed", w), ("mixed", 1)} <= hops
    if w > 1:
        assert len(h.beside) >= 6 and any(h.deg[x] == 0 for x in h.beside) and any(h.deg[x] > 0 for x in h.beside)
    assert any(h.deg[x] == 0 for x in h.ordinary) and len(h.deep) > 100


# ---- 1. the reach boundary ----
@pytest.mark.parametrize("w", BC.HAND_WINDOWS)
def test_reach_boundary(W, hand, w):
    """One request per reach in 0, 1, 2, 62 .. 66, 127 .. 129, 200 and per hop pattern (single hops of w, hops of 1, mixed), singly and then all
    in one batch in three orders; with them the requests whose own chain is short while the chain of a node of the next w - 1 passes 64 or
    more nodes behind them (plan_halo_kernel walks `window` nodes from the block's first, so those may or may not be taken out of the batch:
    the lists must be right either way)."""
    h = hand(w)
    for r in (H - 1, H, H + 1, H + 2):
        assert r in [int(h.reach[e]) for e in h.ends]
    g = _open(W, h.st)
    reqs = h.ends + h.beside[:12] + h.beside[-4:]
    for x in reqs:
        BC.check_batch(g, h.st.lists, [x], ("single", w, x, int(h.reach[x])))
    rng = np.random.default_rng(w)
    for name, order in (("as_listed", reqs), ("reversed", reqs[::-1]), ("shuffled", [reqs[i] for i in rng.permutation(len(reqs))])):
        BC.check_batch(g, h.st.lists, order, ("batch", w, name))
    g.close()


# ---- 2. deep and ordinary requests together ----
@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 255, 256, 257, 1500])
def test_deep_and_ordinary_together(W, hand, count):
    """Batches of `count` requests of which none, one, half and all are deep (reach of 65 and more, or beside such a chain): among them the
    same deep node three times and deep requests without successors next to deep requests with lists -- the deep lists are written at
    succ + cum[i] after the batch has been copied out, and both must land where the prefix sums say.  Every batch is asked twice on the same
    handle, the second time with another deep set, for state left behind."""
    h = hand(7)
    g = _open(W, h.st)
    empty_deep = [x for x in h.beside if h.deg[x] == 0]
    assert empty_deep and all(h.reach[x] > H for x in h.deep)
    rng = np.random.default_rng(count)
    for share in ("none", "one", "half", "all"):
        for again in (0, 1):
            k = {"none": 0, "one": 1, "half": count // 2, "all": count}[share]
            if share == "one" and count == 1:
                k = 1
            pool = rng.permutation(h.deep + empty_deep)
            deep = [int(pool[i % len(pool)]) for i in range(k)]
            if k >= 5:
                deep[1] = deep[3] = deep[0]                                   # the same deep node three times
                deep[2] = empty_deep[again % len(empty_deep)]                 # between them one without successors
            nodes = np.array(deep + [int(x) for x in rng.choice(h.ordinary, count - k)], dtype=np.int64)
            nodes = nodes[rng.permutation(count)]
            BC.check_batch(g, h.st.lists, nodes, ("deep share", share, count, again))
    g.close()


# ---- 3. batch sizes across the levels of the prefix sum ----
@pytest.fixture(scope="module")
def scan_graph(tools, W):
    rng = np.random.default_rng(3)
    n = 2000
    lists = [np.unique(rng.integers(0, n, int(rng.poisson(3)))) if x % 2 else np.empty(0, np.int64) for x in range(n)]
    for x in range(0, n, 200):
        lists[x + 1] = np.unique(rng.integers(0, n, 400))                      # the long lists
    return BC.store_lists(tools, lists, W.default_params())


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 4096, 65535, 65536, 65537, 70000])
def test_batch_sizes_across_the_prefix_sum(W, scan_graph, count):
    """Request counts on both sides of one workgroup of the shared prefix sum (kScanTile = 1024 requests) and of one pass of its serial level
    (64 partial sums: 65 536 requests), over 2 000 nodes with repeats: runs of requests without successors longer than a tile, and one long
    list in every tile.  The prefix sums are not visible through the ABI: they are checked through the position of every list."""
    T = K["scan_tile"]
    assert T == 1024 and count in (1, T - 1, T, T + 1, 4 * T, 64 * T - 1, 64 * T, 64 * T + 1, 70000)
    st = scan_graph
    deg = np.array([len(l) for l in st.lists])
    zeros, longs = np.flatnonzero(deg == 0), np.flatnonzero(deg > 300)
    rng = np.random.default_rng(count)
    nodes = rng.integers(0, 2000, count)
    for lo in range(T // 2, count, 3 * T):                                     # a run of T + 100 empty requests every three tiles, across tile borders
        hi = min(count, lo + T + 100)
        nodes[lo:hi] = rng.choice(zeros, hi - lo)
    for t in range(0, count, T):                                               # one long list per tile, at a position of its own
        nodes[min(count - 1, t + (t // T * 37) % T)] = longs[(t // T) % len(longs)]
    g = _open(W, st)
    BC.check_batch(g, st.lists, nodes, ("prefix sum", count))
    g.close()


# ---- 4. every tier in one batch ----
@pytest.fixture(scope="module")
def tier_graph(tools, W):
    """Lists of 0, 1, 63, 64, 65 successors, one just under and one just over each LDS pool class (kClasses of csrc/bvg_sched.hip), one of
    40 000; after each long list a neighbour that copies most of it."""
    rng = np.random.default_rng(4)
    n = 41000
    lists = [np.empty(0, np.int64)] * n
    lengths = [0, 1, 63, 64, 65] + [p + s for p in K["pools"] for s in (-1, 1)] + [40000]
    special = []
    for i, d in enumerate(lengths):
        x = 50 + 37 * i
        lists[x] = np.sort(rng.choice(n, d, replace=False)).astype(np.int64)
        if d >= 63:
            keep = lists[x][rng.random(d) < 0.95]
            lists[x + 1] = np.unique(np.concatenate([keep, rng.integers(0, n, 5)]))
            special.append(x + 1)
        special.append(x)
    for x in range(2000, 2300):
        lists[x] = np.unique(rng.integers(x - 50, x + 50, int(rng.poisson(5))))
    st = BC.store_lists(tools, lists, W.default_params())
    st.special = special
    return st


@pytest.mark.parametrize("mode", ["as_is", "giant", "force_slow", "force_wide"])
def test_every_tier_in_one_batch(W, monkeypatch, tier_graph, mode):
    """One batch with a request of every class -- tier 0, the four pool classes, the giant kernel, lists that copy a long neighbour -- in an
    order that interleaves them with short and empty lists; as is, on the giant kernel for every block, on the generic kernel and on the
    64-bit kernels."""
    assert K["pools"] == (2048, 4096, 8192, 12288)
    st = tier_graph
    if mode == "giant":
        monkeypatch.setenv("BVG_GIANT", "2")
    g = _open(W, st, **({"force_slow": True} if mode == "force_slow" else {"force_wide": True} if mode == "force_wide" else {}))
    rng = np.random.default_rng(44)
    small = [int(x) for x in rng.integers(2000, 2300, 3 * len(st.special))] + [0, 40999]
    order = [int(x) for x in rng.permutation(st.special)]
    nodes = [x for i, s in enumerate(order) for x in (s, small[2 * i], small[2 * i + 1])] + small[2 * len(order):] + order[:3]
    BC.check_batch(g, st.lists, nodes, ("tiers", mode))
    g.close()


# ---- 5. the capacity contract and the growth of the workspace ----
def _raw(W, g, nodes, cap, with_succ=True, guard=64):
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    deg = np.full(len(nodes) + guard, -7, dtype=np.int32)
    succ = np.full(cap + guard, -7, dtype=np.int64)
    need = C.c_uint64(123456789)
    r = W.lib().bvg_successors_batch(g._h, nodes.ctypes.data if len(nodes) else None, len(nodes), deg.ctypes.data, succ.ctypes.data if with_succ else None, cap, C.byref(need))
    assert (deg[len(nodes):] == -7).all() and (succ[cap:] == -7).all(), "written behind the capacity"
    return r, int(need.value), deg[:len(nodes)], succ[:cap]


def test_capacity_contract(W, hand):
    """succ = NULL with capacity 0 and capacity total - 1: BVG_E_CAPACITY, *n_succ = the total, the outdegrees filled, no successor written;
    capacity = total: 0.  A batch without arcs and succ = NULL: 0.  With deep requests in the batch, and without."""
    h = hand(7)
    g = _open(W, h.st)
    empty = [x for x in h.ordinary if h.deg[x] == 0][:5]
    for nodes in (h.ordinary[300:340], h.deep[:3] + h.ordinary[300:310] + h.deep[50:52]):
        edeg, esucc = BC.expected(h.st.lists, nodes)
        total = len(esucc)
        for cap, with_succ in ((0, False), (total - 1, True), (0, True)):
            r, need, deg, succ = _raw(W, g, nodes, cap, with_succ)
            assert r == W.E_CAPACITY and need == total and np.array_equal(deg, edeg) and (succ == -7).all(), (cap, with_succ)
        r, need, deg, succ = _raw(W, g, nodes, total)
        assert r == 0 and need == total and np.array_equal(deg, edeg) and np.array_equal(succ, esucc)
    r, need, deg, succ = _raw(W, g, empty, 0, with_succ=False)
    assert r == 0 and need == 0 and not deg.any()
    g.close()


def test_arguments_out_of_range(W, hand):
    """A negative id and id = nodes: BVG_E_ARG, before anything is written -- *n_succ included, which keeps what the caller put there (the
    header does not say; this pins what the code does).  count = 0 is NOT an error at this commit: 0, *n_succ = 0 (an empty frontier has
    an empty answer; a negative count is BVG_E_ARG).  A contract question rather than a bug: pinned as it is."""
    h = hand(7)
    g = _open(W, h.st)
    for nodes in ([5, -1, 6], [5, h.n], [-(1 << 40)], [h.n + (1 << 33), 3]):
        r, need, deg, succ = _raw(W, g, nodes, 100)
        assert r == W.E_ARG and need == 123456789 and (deg == -7).all() and (succ == -7).all(), nodes
    r, need, deg, succ = _raw(W, g, [], 100)
    assert r == 0 and need == 0 and (succ == -7).all()
    need = C.c_uint64(55)
    one = np.array([5], dtype=np.int64)
    assert W.lib().bvg_successors_batch(g._h, one.ctypes.data, -1, None, None, 0, C.byref(need)) == W.E_ARG and need.value == 55
    BC.check_batch(g, h.st.lists, [5, h.n - 1, 0], "after the refusals")
    g.close()


def growth_calls(h, with_deep):
    """(name, requests) of the calls of the workspace-growth test: tiny, large, tiny again, large reversed."""
    tiny = [x for x in h.ordinary if h.deg[x] == 1][:2]
    assert len(tiny) == 2
    rng = np.random.default_rng(5)
    big = [int(x) for x in rng.choice([x for x in h.ordinary if h.deg[x] >= 5], 2500)]
    if with_deep:
        big[100:2500:25] = [int(x) for x in rng.choice(h.deep, 96)]
    assert sum(h.deg[x] for x in big) > 5000 * sum(h.deg[x] for x in tiny)
    return [("tiny", tiny), ("large", big), ("tiny_again", tiny), ("large_again", big[::-1])]


@pytest.mark.parametrize("with_deep", [False, True])
def test_workspace_growth_between_the_two_preparations(W, hand, with_deep):
    """On a fresh handle: a call with a tiny total, then one whose total is thousands of times larger -- the successors no longer fit the
    workspace, it moves, and the preparation (requests, outdegrees, prefix sums, plan, halos, deep list) is made again in the new one --
    then the tiny one again.  Without deep requests in the large call, and with.
    What this comparison CANNOT see: a library that leaves the second preparation out reads the plan, the halos and the prefix sums from
    the workspace it has just freed, and the values are usually still there, on the host emulator and on the device alike: every list
    comes out right.  The same calls are therefore replayed by a program of its own under AddressSanitizer on the host emulator
    (tests/emu/batch_replay.cpp, tests/test_emu.py::test_workspace_growth_replayed_under_address_sanitizer), which reports that read."""
    h = hand(7)
    g = _open(W, h.st)
    for what, nodes in growth_calls(h, with_deep):
        BC.check_batch(g, h.st.lists, nodes, (what, with_deep))
    g.close()


# ---- 6. handles ----
@pytest.mark.parametrize("kind", BC.HANDLE_KINDS)
def test_handles(W, hand, kind):
    """The same request set -- ordinary and deep requests, the ends of the graph -- through a handle with a node base (1 000, and one beyond
    2^32: the successors are shifted, the requests stay local), a bvg_copy, a bvg_tile of 3 copies (requests in every copy, among them the
    first `window` nodes of copies 1 and 2, whose records reference nothing before their copy), handles with no_index 1 and 2, and a handle
    on which a full scan has built the skip index (`plain` is the one on which none has)."""
    h = hand(7)
    keep, g, lists, base = BC.open_kind(W, h.st, kind)
    rng = np.random.default_rng(6)
    local = [0, h.n - 1] + h.ends + h.beside[:6] + [int(x) for x in rng.choice(h.ordinary, 80)] + h.deep[10:14]
    if kind == "tile":
        nodes = [c * h.n + x for c in range(3) for x in local] + [c * h.n + j for c in (1, 2) for j in range(8)]
        nodes = [nodes[i] for i in rng.permutation(len(nodes))]
    else:
        nodes = [local[i] for i in rng.permutation(len(local))]
    for _ in range(2):
        BC.check_batch(g, lists, nodes, ("handle", kind), base=base)
    for x in keep[::-1]:
        x.close()


# ---- 7. the parameter space ----
def _parameter_sets():
    sets, i = [], 0
    for w in BC.WINDOWS:
        for m in BC.MAX_REF_COUNTS:
            # (shapes in rotation, but a window of 1 with 63, 64 or 65 references on "copies": the encoder-made chains that end exactly there)
            shape = "copies" if w == 1 and m in (H - 1, H, H + 1) else BC.SHAPES[i % 4]
            sets.append(dict(window_size=w, max_ref_count=m, min_interval_length=(0, 2, 4)[i % 3], zeta_k=(1, 3, 5)[(i // 3) % 3], shape=shape))
            i += 1
    rng = np.random.default_rng(7)
    for j in range(8):                                                        # non-default codings, at windows and reference counts that make chains
        kw = {k: int(rng.choice(v)) for k, v in BC.CODINGS.items()}
        kw.update(window_size=(7, 20, 64, 70)[j % 4], max_ref_count=(65, -1, 64, 1000)[j % 4], min_interval_length=(0, 2, 4)[j % 3], zeta_k=(1, 3, 5)[j % 3], shape=BC.SHAPES[(j + 2) % 4])
        sets.append(kw)
    return sets


PARAMETER_SETS = _parameter_sets()


def _set_id(kw):
    cod = "-".join(str(kw[k]) for k in BC.CODINGS) if "residual_coding" in kw else "default"
    return "w%d-m%d-i%d-k%d-%s-%s" % (kw["window_size"], kw["max_ref_count"], kw["min_interval_length"], kw["zeta_k"], kw["shape"], cod)


@pytest.mark.parametrize("kw", PARAMETER_SETS, ids=_set_id)
def test_parameter_space(W, tools, kw):
    """Encoder-made graphs of 1 500 nodes: windows 1 .. 127 x reference counts 1 .. 1 000 and unbounded, with interval lengths 0 / 2 / 4,
    zeta 1 / 3 / 5 and four shapes in rotation (among them "copies most of a near neighbour"), then non-default codings at the windows
    that make long chains.  Every node is requested, in a random permutation with 10 % repeats.
    The reaches of the graph that is SENT are read back with reaches() (own_reach over every node) wherever the codings are the default
    ones: no chain is longer than max_ref_count hops of at most `window` nodes; a window of 1 with 63, 64 and 65 references on "copies"
    ends chains exactly at the reaches 63, 64 and 65; on "copies", 63 and more references (or no bound) put chains on both sides of 64
    nodes at every window, and 3 references stay within 3 windows.  With non-default codings the reach is NOT read (own_reach reads gamma
    outdegrees and unary references only): those sets are compared list for list like the others, at windows and reference counts at
    which the default codings make long chains, but that a chain of theirs ends at a boundary is not shown."""
    kw = dict(kw)
    shape = kw.pop("shape")
    w, m = kw["window_size"], kw["max_ref_count"]
    rng = np.random.default_rng([w, m + 1, kw["zeta_k"], kw.get("residual_coding", 0)])
    n = 1500
    st = BC.store_lists(tools, BC.shape_lists(shape, n, rng, tools), W.default_params(**kw))
    if "residual_coding" not in kw:
        top = int(BC.reaches(st).max())
        print("reach", _set_id(dict(kw, shape=shape)), top)
        assert m < 0 or top <= m * w, (top, kw)
        if shape == "copies":
            if w == 1 and m in (H - 1, H, H + 1):
                assert top == m, (top, kw)
            elif m < 0 or m >= H - 1:
                assert top > H + 1, (top, kw)
    nodes = np.concatenate([rng.permutation(n), rng.integers(0, n, n // 10)])
    nodes = nodes[rng.permutation(len(nodes))]
    g = _open(W, st)
    BC.check_batch(g, st.lists, nodes, ("parameters", kw, shape))
    g.close()


# ---- 8. wide windows: the halo as a count ----
@pytest.fixture(scope="module")
def wide_hand(W):
    """Window 70: one chain of 117 hops of 70 and then hops of 1, so that five consecutive nodes have the reaches kMaxHaloBig - 2 .. + 2."""
    big, w = K["max_halo_big"], 70
    rng = np.random.default_rng(8)
    lead = 90
    n = lead + big + 2 + 300
    on = {lead + i * w: w for i in range(1, (big - 2) // w + 1)}
    top = lead + ((big - 2) // w) * w
    x = top
    while x - lead < big + 2:
        x += 1; on[x] = 1
    recs, lists = [], []
    for x in range(n):
        if x == lead or x not in on:
            l = sorted(set(int(v) for v in rng.integers(0, n, int(rng.integers(0, 4)) if x != lead else 6)))
            l = [v for i, v in enumerate(l) if i == 0 or v - l[i - 1] > 1]
            recs.append(Record(d=len(l), residuals=l)); lists.append(l)
            continue
        src = lists[x - on[x]]
        keep = np.ones(len(src), dtype=bool); keep[x % len(src)] = False
        copied = [v for v, f in zip(src, keep) if f]
        own = next(v for v in (int(v) for v in rng.integers(0, n, 50)) if all(abs(v - c) > 1 for c in copied))
        recs.append(BC.copy_record(x, on[x], src, keep, [own])); lists.append(sorted(copied + [own]))
    graph, offsets, out = assemble(recs, window=w)
    assert out == lists
    st = BC.Stream(W.default_params(window_size=w).clone(nodes=n, arcs=sum(len(l) for l in lists)), graph, offsets, lists)
    return st, lead, big


def test_wide_window_reaches_around_the_halo_count(W, oracle, wide_hand):
    """Window 70 (the windows 65 .. 127 run on the generic kernel, the halo a count up to kMaxHaloBig = 8 192, decoded whole): requests at the
    reaches 8 190 .. 8 194 on a graph of about 9 000 short lists, the first of the chain, node w - 1 and node 0; singly and in one batch."""
    st, lead, big = wide_hand
    assert big == 8192
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    ends = [lead + big + s for s in (-2, -1, 0, 1, 2)]
    for x in ends:
        assert og.successors(x).tolist() == st.lists[x]
    assert [BC.own_reach(st.params, st.graph, st.offsets, x) for x in ends] == [big - 2, big - 1, big, big + 1, big + 2]
    g = _open(W, st)
    reqs = ends + [lead, lead + 70, 69, 0, int(st.params.nodes) - 1]
    for x in reqs:
        BC.check_batch(g, st.lists, [x], ("wide single", x))
    BC.check_batch(g, st.lists, reqs[::-1] + reqs, "wide batch")
    g.close()


# ---- 9. streams that are wrong ----
def _filler(x, k=6):
    return Record(d=k, residuals=[x + 3 + 5 * i for i in range(k)])


def _wrong_streams(W):
    """name -> (params, graph, offsets, lists by the iterators of tests/bvrecords.py, the odd node).  40 plain nodes, the odd one at 20."""
    out = {}
    for name, odd, at in (("reference_beyond_the_window", Record(d=4, ref=9, blocks=[3], residuals=[7]), 20),
                          ("reference_before_node_0", Record(d=4, ref=5, blocks=[3], residuals=[7]), 2),
                          ("copy_block_over_runs", Record(d=13, ref=1, blocks=[3, 2, 9], residuals=[7]), 20),
                          ("truncated_record", _filler(39, 12), 39)):
        recs = [_filler(x) for x in range(40)]
        for back in (1, 5, 9):
            if at - back >= 0:
                recs[at - back] = Record(d=10, residuals=[100 + 10 * i for i in range(10)])
        recs[at] = odd
        if name == "reference_before_node_0":                                  # (the iterators need a list to copy from: there is none)
            lists, w, offs = None, PyBits(), [0]
            for x, rec in enumerate(recs):
                rec.write(w, x, 7, 4, 3, len(rec.residuals)); offs.append(len(w))
            graph, offsets = w.tobytes(), np.array(offs, dtype=np.uint64)
        else:
            graph, offsets, lists = assemble(recs, window=7)
        if name == "truncated_record":
            graph = graph[:len(graph) - 3]
            offsets = np.minimum(offsets, np.uint64(8 * len(graph)))
        p = W.default_params().clone(nodes=40, arcs=-1)
        out[name] = (p, np.frombuffer(bytes(graph), dtype=np.uint8), offsets, lists, at)
    return out


# what bvg_decode_range(x, x + 1) does with the odd node of each stream at this commit: recorded, not invented
RANGE_DECODE_OF_THE_ODD_NODE = {
    "reference_beyond_the_window": "E_STATE",
    "reference_before_node_0": "E_STATE",
    "copy_block_over_runs": "short list padded with -1",
    "truncated_record": "E_EOF",
}


@pytest.mark.parametrize("name", sorted(RANGE_DECODE_OF_THE_ODD_NODE))
def test_wrong_streams_in_a_batch(W, name):
    """A reference beyond the window, a reference before node 0, a copy block that over-runs the referenced list and a record that the file
    cuts short, each requested in a batch next to healthy nodes: the batch ends with the status that bvg_decode_range(x, x + 1) gives for
    the odd node (RANGE_DECODE_OF_THE_ODD_NODE: what the range decode does at this commit), or hands out the same -1-padded list, and where
    the call succeeds the healthy requests' lists are intact.  The healthy requests alone always decode."""
    p, graph, offsets, lists, at = _wrong_streams(W)[name]
    g = W.BVGraph.from_memory(p, graph, offsets)
    L = W.lib()
    deg1 = np.zeros(1, np.int32); succ1 = np.full(64, -7, np.int64); need = C.c_uint64(0)
    r1 = L.bvg_decode_range(g._h, at, at + 1, deg1.ctypes.data, succ1.ctypes.data, 64, C.byref(need))
    what = RANGE_DECODE_OF_THE_ODD_NODE[name]
    assert r1 == {"E_STATE": W.E_STATE, "E_EOF": W.E_EOF}.get(what, 0), (name, r1)
    healthy = [x for x in (0, 3, 8, 12, 25, 27, 33, 36) if x not in (at, at - 1, at - 5, at - 9)][:5]
    nodes = healthy[:2] + [at] + healthy[2:] + [at]
    r, n_succ, deg, succ = _raw(W, g, nodes, 400)
    assert r == r1, (name, r, r1)
    plain = {x: [x + 3 + 5 * i for i in range(6)] for x in healthy}
    if r == 0:
        odd = succ1[:int(need.value)].tolist()
        assert -1 in odd and (lists is None or odd == lists[at])
        exp = [v for x in nodes for v in (odd if x == at else plain[x])]
        assert n_succ == len(exp) and succ[:n_succ].tolist() == exp and deg.tolist() == [len(odd) if x == at else 6 for x in nodes]
    r, n_succ, deg, succ = _raw(W, g, healthy, 400)
    assert r == 0 and succ[:n_succ].tolist() == [v for x in healthy for v in plain[x]]
    g.close()


# ---- 10. the frontier route sees the same lists ----
def test_frontier_route_sees_the_same_lists(W, monkeypatch, hand):
    """bvg_bfs_visit on its frontier route runs the same three steps.  On the graph of item 2: a visit from the end of a chain of reach 200
    against the plain breadth-first search of tests/test_gpu_bfs.py (distances and queue), its `deep_requests` counter positive; a visit
    inside the first 300 nodes -- plain lists with targets among themselves, no chain anywhere near -- with the counter 0.  The route
    over-approximates (item 1: a request beside a long chain may be counted too), so the counter is asserted only where both readings agree:
    positive when a frontier node has own_reach >= 65, zero when no frontier node is within a window of such a chain."""
    monkeypatch.setenv("BVG_BFS_ROUTE", "frontier")
    h = hand(7)
    off, adj = csr_of_lists(h.st.lists)
    g = _open(W, h.st)
    for start, deep_expected in ((h.ends[-1], True), (7, False)):
        queue, cuts, dist, _ = cpu_bfs(off, adj, start)
        assert len(queue) > 20
        assert any(h.reach[x] > H for x in queue) if deep_expected else not any(BC.beyond_a_block(h.st, h.reach, int(x)) for x in queue)
        with g.breadth_first_visit() as v:
            assert v.visit(start) == len(queue)
            assert np.array_equal(v.dist, dist) and np.array_equal(v.queue, queue) and np.array_equal(v.cut_points, cuts)
            c = v.counters()
            assert c["frontier_levels"] > 0 and c["sweep_levels"] == 0
            assert (c["deep_requests"] > 0) == deep_expected, c
    g.close()
