"""Graphs, request patterns and the one reference of the random-access suite: shared by tests/test_gpu_batch.py (the deterministic
cases) and tests/test_gpu_batch_fuzz.py (seeded draws).

THE REFERENCE is the adjacency the test itself wrote down: expected(lists, nodes) is the outdegrees and the concatenation of lists[x]
in request order, in plain Python / numpy.  It calls no library.  For the hand-assembled streams `lists` comes from the pure-Python
iterators of tests/bvrecords.py (tests/test_gpu_batch.py holds them against the oracle's decode of the same bytes, once per stream).

own_reach() reads the stream itself -- the gamma outdegree and the unary reference of record after record -- and says how far before x
the reference chain of x goes.  The tests use it only to assert that a case set holds the reaches it claims (a test of the boundary has
requests at reach 63, 64, 65 and 66); no assertion concerns the route the library took.

The numbers the cases are placed around are read from the sources (constants()): kMaxHalo, kMaxHaloBig and kMaxWindow of
csrc/bvg_kernels.h, kScanTile of csrc/bvg_kernels.hip, kMaxPool / kClasses of csrc/bvg_sched.hip.  A request block's halo is a mask of
kMaxHalo nodes before x: plan_halo_kernel refuses a chain whose node lies kMaxHalo or more nodes before x - 1, that is a reach of
kMaxHalo + 1 = 65 and more (kMaxHaloBig + 1 = 8193 and more for windows above kMaxWindow)."""
import functools
import os
import re

import numpy as np

from bvrecords import Record, assemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgraph-big_amd", "csrc")

WINDOWS = (1, 3, 7, 20, 64, 70, 127)                     # the encoder-made chains
MAX_REF_COUNTS = (1, 3, 63, 64, 65, 1000, -1)
HAND_WINDOWS = (1, 2, 7, 64)                             # the hand-assembled chains
PATTERNS = ("every", "reversed", "permutation", "repeats", "ends", "zeros", "one", "alternating")
SHAPES = ("local", "empty_runs", "copies", "crawl")
# the non-default codings tests/test_gpu_fuzz.py draws from (include/bvgraph_hip.h: DELTA = 1, GAMMA = 2, GOLOMB = 3, UNARY = 5, ZETA = 6, NIBBLE = 7)
CODINGS = dict(outdegree_coding=(1, 2), block_coding=(1, 2, 5), residual_coding=(1, 2, 3, 6, 7), reference_coding=(1, 2, 5), block_count_coding=(1, 2, 5))


@functools.lru_cache(maxsize=None)
def constants():
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    def const(text, name):
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, text)
        assert m, "no `constexpr <type> %s = <number>;` in the sources any more" % name
        return int(m.group(1))
    kh, kk, ks = src("bvg_kernels.h"), src("bvg_kernels.hip"), src("bvg_sched.hip")
    max_pool = const(ks, "kMaxPool")
    line = next((l for l in ks.splitlines() if "kClasses[4]" in l and "{" in l), None)
    assert line, "no initialiser of kClasses[4] in bvg_sched.hip any more"
    pools = []
    for e in line[line.index("{") + 1:line.index("}")].split(","):          # each entry: kMaxPool, kMaxPool / N or kMaxPool * N / M
        m = re.fullmatch(r"kMaxPool(?: \* (\d+))?(?: / (\d+))?", e.replace("(", "").replace(")", "").strip())
        assert m, "an entry of kClasses that is neither kMaxPool / N nor (kMaxPool * N) / M: %r in %r" % (e.strip(), line.strip())
        pools.append(max_pool * int(m.group(1) or 1) // int(m.group(2) or 1))
    pools = tuple(pools)
    assert len(pools) == 4 and pools[-1] == max_pool and list(pools) == sorted(pools), line
    return dict(max_halo=const(kh, "kMaxHalo"), max_halo_big=const(kh, "kMaxHaloBig"), max_window=const(kh, "kMaxWindow"),
                scan_tile=const(kk, "kScanTile"), pools=pools)


# ---- the reference ----
def expected(lists, nodes):
    """(outdegrees, successors) of the requests, in request order."""
    deg = np.array([len(lists[int(x)]) for x in nodes], dtype=np.int64)
    succ = np.array([int(v) for x in nodes for v in lists[int(x)]], dtype=np.int64)
    return deg, succ


def check_batch(g, lists, nodes, what, base=0):
    """One bvg_successors_batch call against expected(): outdegrees and successors, element for element."""
    nodes = np.asarray(nodes, dtype=np.int64)
    try:
        deg, succ = g.successors_batch(nodes)
    except BaseException:
        print("batch that raised:", what, flush=True)
        raise
    edeg, esucc = expected(lists, nodes)
    esucc = np.where(esucc >= 0, esucc + base, esucc)                       # (the -1 of a short list is no node: it is not shifted)
    assert np.array_equal(deg.astype(np.int64), edeg), (what, "outdegrees: first difference at request %d" % int(np.argmax(deg[:len(edeg)] != edeg)))
    assert len(succ) == len(esucc), (what, len(succ), len(esucc))
    if not np.array_equal(succ, esucc):
        at = int(np.argmax(succ != esucc)); req = int(np.searchsorted(np.cumsum(edeg), at, side="right"))
        raise AssertionError((what, "successors: first difference at element %d (request %d, node %d): got %d, expected %d" % (at, req, int(nodes[req]), int(succ[at]), int(esucc[at]))))


@functools.lru_cache(maxsize=8)
def _bit_string(graph_bytes):
    return "".join(format(b, "08b") for b in graph_bytes)


def _hop(s, offsets, w, y):
    """The reference of record y as the chain follows it: 0 where it has none (or one that no decoder follows)."""
    p = int(offsets[y]); one = s.index("1", p); k = one - p                  # gamma: k zeros, then k + 1 bits of d + 1
    if w == 0 or int(s[one:one + k + 1], 2) - 1 == 0:
        return 0                                                             # no successors: no reference field
    r = s.index("1", one + k + 1) - (one + k + 1)                            # unary
    return 0 if r > w or r > y else r


def own_reach(params, graph_bytes, offsets, x):
    """How far before x the reference chain of x goes (0: x has no reference).  Default codings only."""
    s, y = _bit_string(bytes(graph_bytes)), int(x)
    while True:
        r = _hop(s, offsets, int(params.window_size), y)
        if r == 0:
            return int(x) - y
        y -= r


def reaches(st):
    """own_reach of every node of a stored graph (default codings), each chain node read once."""
    s, out = _bit_string(bytes(st.graph)), []
    for x in range(int(st.params.nodes)):
        r = _hop(s, st.offsets, int(st.params.window_size), x)
        out.append(r + out[x - r] if r else 0)
    return np.array(out, dtype=np.int64)


def beyond_a_block(st, reach, x):
    """A node x + j of the `window` nodes from x whose chain passes kMaxHalo (kMaxHaloBig) or more nodes behind x - 1: plan_halo_kernel walks
    them all, so x may or may not be decoded apart from its batch.  j = 0 is own_reach(x) >= 65."""
    w, n = int(st.params.window_size), len(reach)
    lim = constants()["max_halo_big" if w > constants()["max_window"] else "max_halo"]
    return any(reach[x + j] - j > lim for j in range(min(w, n - x)))


# ---- hand-assembled chains ----
class Stream:
    """A graph in memory with the adjacency it was made from: params, graph (uint8), offsets, lists."""

    def __init__(self, params, graph, offsets, lists):
        self.params, self.graph, self.offsets, self.lists = params, np.frombuffer(bytes(graph), dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.uint64), lists


def copy_record(x, ref, ref_list, keep, own, interval=None):
    """The record of x = (the elements of ref_list with keep[i]) + own elements (+ one interval), with the copy blocks of the mask."""
    runs, cur, k = [], True, 0
    for f in keep:
        if bool(f) != cur:
            runs.append(k); cur, k = bool(f), 0
        k += 1
    runs.append(k)
    copied = [v for v, f in zip(ref_list, keep) if f]
    ivs = [interval] if interval else []
    d = len(copied) + len(own) + sum(n for _, n in ivs)
    return Record(d=d, ref=ref, blocks=runs[:-1], intervals=ivs, residuals=sorted(own))          # (the last run is implied by the parity of the block count)


def hops_of(kind, reach, w):
    """The hops of a chain of `reach` nodes, first hop first: "wide" single hops of w, "ones" hops of 1, "mixed" both and w // 2."""
    if kind == "ones" or w == 1:
        return [1] * reach
    if kind == "wide":
        return ([reach % w] if reach % w else []) + [w] * (reach // w)
    out, pat, i = [], (w, 1, max(1, w // 2), 1, 1, w), 0
    while sum(out) < reach:
        out.append(min(pat[i % len(pat)], reach - sum(out))); i += 1
    return out[::-1]


def chain_stream(W, window, segments, seed, lead=300, gap=3, tail=40, min_nodes=0):
    """A hand-assembled stream of chains.  segments: (reach, hop kind) each: a chain that ends at a node of that reach; the nodes between
    the chain's nodes have no reference, the one before the chain's end has no successors where the last hop allows it.  Every list is a
    base set (targets inside the first `lead` nodes) minus a few, plus a few own elements.  The first `lead` nodes are plain lists with
    targets below `lead` (a closed region without references).  Returns (Stream, the end node of every segment)."""
    rng = np.random.default_rng([seed, window])
    n = max(lead + sum(r + 1 + gap + window for r, _ in segments) + tail, min_nodes)
    recs, lists, ends = [], [], []
    def own_elems(x, avoid, k):
        out = set()
        while len(out) < k:
            v = int(rng.integers(0, n))
            if v not in avoid and not any(abs(v - o) < 2 for o in out):     # (no two consecutive: residuals, not an interval the writer left out)
                out.add(v)
        return sorted(out)
    def plain(x, closed=False):
        k = int(rng.integers(0, 7)) if x % 5 else 0
        l = sorted(set(int(v) for v in rng.integers(0, lead if closed else n, k)))
        l = [v for i, v in enumerate(l) if i == 0 or v - l[i - 1] > 1]
        return Record(d=len(l), residuals=l), l
    def put(rec, l):
        recs.append(rec); lists.append(l)
    for x in range(lead):
        put(*plain(x, closed=True))
    base = sorted(set(int(v) for v in rng.integers(0, lead, 9)))
    for reach, kind in segments:
        for _ in range(gap + window):                                       # (no chain of the next segment's first nodes reaches the last segment)
            put(*plain(len(recs)))
        start = len(recs)
        hops = hops_of(kind, reach, window) if reach else []
        on = set(np.cumsum([0] + hops).tolist())
        for i in range(reach + 1):
            x = start + i
            if i not in on:
                if i == reach - 1:
                    put(Record(d=0), [])
                else:
                    put(*plain(x))
                continue
            if i == 0:
                l = sorted(set(base + own_elems(x, set(base), 2)))
                l = [v for j, v in enumerate(l) if j == 0 or v - l[j - 1] > 1]
                put(Record(d=len(l), residuals=l), l)
                continue
            ref = hops[sorted(on).index(i) - 1]
            src = lists[x - ref]
            keep = np.ones(len(src), dtype=bool)
            keep[rng.integers(0, len(src), 1 if len(src) > 6 else 0)] = False
            if i % 7 == 3 and len(src) > 4:
                keep[:2] = False                                             # (an empty first block)
            copied = [v for v, f in zip(src, keep) if f]
            interval = None
            if i % 11 == 5:
                left = max(copied) + 2 + int(rng.integers(0, 5))
                if left + 4 < n:
                    interval = (left, 4)
            taken = set(copied) | (set(range(interval[0] - 1, interval[0] + 6)) if interval else set())
            own = own_elems(x, taken | set(v + 1 for v in copied) | set(v - 1 for v in copied), 1 + (len(copied) < 8))
            rec = copy_record(x, ref, src, keep, own, interval)
            put(rec, sorted(copied + own + (list(range(interval[0], interval[0] + 4)) if interval else [])))
        ends.append(start + reach)
    while len(recs) < n:
        put(*plain(len(recs)))
    graph, offsets, out_lists = assemble(recs, window=window)
    assert out_lists == lists, "the iterators of tests/bvrecords.py read the records as they were meant"
    p = W.default_params(window_size=window).clone(nodes=n, arcs=int(sum(len(l) for l in lists)))
    return Stream(p, graph, offsets, lists), ends


# ---- encoder-made graphs ----
def _unique(a):
    return np.unique(np.asarray(a, dtype=np.int64))


def shape_lists(shape, n, rng, tools=None):
    """The adjacency of an n-node graph as a list of sorted int64 arrays."""
    if n == 1:
        return [np.array([0] if rng.random() < 0.5 else [], dtype=np.int64)]
    if shape == "crawl":
        off, adj = tools.synth_adjacency(n, seed=int(rng.integers(0, 1 << 30)), synth=tools.web_like(mean_deg=8.0, max_deg=400))
        return [adj[int(off[x]):int(off[x + 1])].copy() for x in range(n)]
    lists = []
    for x in range(n):
        lo, hi = max(0, x - 60), min(n, x + 61)
        if shape == "local":                                                 # sparse lists with locality, one in six empty, some consecutive runs
            k = 0 if rng.random() < 0.17 else int(rng.poisson(6))
            l = _unique(rng.integers(lo, hi, k))
            if rng.random() < 0.2:
                s0 = int(rng.integers(0, n)); l = _unique(np.concatenate([l, np.arange(s0, min(n, s0 + int(rng.integers(2, 9))))]))
        elif shape == "empty_runs":                                          # tests/sweep_cases.py: empty runs at the start, in the middle and at the end, one long list
            third = (5 * x) // n
            l = _unique(rng.integers(0, n, int(rng.poisson(3)))) if third in (1, 3) else np.empty(0, np.int64)
            if x == (3 * n) // 10:
                l = _unique(rng.choice(n, min(n, 150), replace=False))
        else:                                                                # "copies": most of a near neighbour's list, a few elements of its own
            back = 1 if rng.random() < 0.7 else int(rng.integers(2, 4))
            if x >= back and len(lists[x - back]) and rng.random() < 0.98:
                prev = lists[x - back]
                l = _unique(np.concatenate([prev[rng.random(len(prev)) < 0.93], rng.integers(0, n, int(rng.integers(0, 3)))]))
            else:
                l = _unique(rng.integers(0, n, int(rng.integers(4, 20))))
        lists.append(l)
    return lists


def store_lists(tools, lists, params):
    st = tools.store([l for l in lists], params, threads=2)
    st.lists = lists
    return st


# ---- request patterns ----
def requests(pattern, n, deg, deep, rng, count=None):
    """Node ids of one batch.  deg: the outdegrees; deep: the nodes of the largest reach, largest first (may be empty); count: the number
    of requests where the pattern has no size of its own."""
    count = count or n
    allx = np.arange(n, dtype=np.int64)
    ordinary = np.setdiff1d(allx, deep) if len(deep) < n else allx
    if pattern == "every":
        return allx
    if pattern == "reversed":
        return allx[::-1].copy()
    if pattern == "permutation":
        return np.resize(rng.permutation(allx), count)
    if pattern == "repeats":                                                 # one node 300 times, among others: a deep one where there is one, and an ordinary one
        r = rng.integers(0, n, count + 600)
        for x in ([int(deep[0])] if len(deep) else []) + [int(ordinary[len(ordinary) // 2])]:
            r[rng.choice(len(r), 300, replace=False)] = x
        return r.astype(np.int64)
    if pattern == "ends":
        return np.array([0, n - 1], dtype=np.int64)
    if pattern == "zeros":
        z = np.flatnonzero(np.asarray(deg) == 0)
        return np.resize(z, min(count, max(len(z), 1))).astype(np.int64) if len(z) else np.array([0], dtype=np.int64)
    if pattern == "one":
        return np.array([int(deep[0]) if len(deep) else n // 2], dtype=np.int64)
    if pattern == "alternating":
        a = np.resize(deep if len(deep) else allx, (count + 1) // 2); b = np.resize(rng.permutation(ordinary), (count + 1) // 2)
        return np.stack([a, b], axis=1).reshape(-1)[:count].astype(np.int64)
    raise KeyError(pattern)


# ---- handles ----
HANDLE_KINDS = ("plain", "base_1000", "base_2^32", "copy", "tile", "no_index_1", "no_index_2", "indexed")


def open_kind(W, st, kind, tuning=None):
    """(handles to close, the handle to ask, the lists it must answer with, the node base): the same graph through a handle of each kind.
    tile: 3 copies, node c * n + x holds lists[x] + c * n."""
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    tuning = dict(tuning or {})
    lists, base, keep = st.lists, 0, [g]
    if kind.startswith("no_index"):
        tuning["no_index"] = int(kind[-1])
    if tuning:
        g.set_tuning(**tuning)
    if kind == "base_1000" or kind == "base_2^32":
        base = 1000 if kind == "base_1000" else (1 << 32) + 12345
        g.set_node_base(base)
    elif kind == "copy":
        g = g.copy(); keep.append(g)
    elif kind == "tile":
        n = int(st.params.nodes)
        g = g.tile(3); keep.append(g)
        lists = [np.asarray(l, dtype=np.int64) + c * n for c in range(3) for l in st.lists]
    elif kind == "indexed":
        g.scan(); g.build_index()
    return keep, g, lists, base
