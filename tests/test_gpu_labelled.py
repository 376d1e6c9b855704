"""GPU: arc-labelled graphs on the device (bvg_lgraph_*), list for list and label for label against the model (tests/labelled_model.py); the
label stream byte for byte against the CPU writer (tooling.store_labels); the files against BitStreamArcLabelledImmutableGraph.load.
The yardsticks that exist stay the yardsticks: the unlabelled transforms for the underlying graphs, bvg_store's refusals for from_csr."""
import ctypes as C
import os

import numpy as np
import pytest

import labelled_model as LM
from conftest import CNR
from test_gpu_text import DeviceBytes

pytestmark = pytest.mark.gpu

GAMMA, FIXED, LIST = 1, 2, 3
N_CNR = 325557
STRATEGIES = [LM.KEEP_FIRST, LM.MIN, LM.MAX]


def lgraph(W, g, kind=GAMMA, width=0):
    return W.LabelledGraph.from_csr(g[0], g[1], g[2], kind, width)


def holds(lg, want, kind=None, width=None):
    """The resident graph holds the model's offsets, successors and labels (and closes)."""
    with lg:
        off, adj, lab = lg.csr()
        assert lg.num_nodes() == LM.nodes(want) and lg.num_arcs() == len(adj) == len(lab) == int(off[-1])
        assert np.array_equal(off, want[0]), "offsets differ"
        assert np.array_equal(adj, want[1]), "successors differ"
        assert np.array_equal(lab, want[2]), "labels differ"
        assert lab.dtype == np.int32 and adj.dtype == np.int64 and off.dtype == np.uint64
        if kind is not None:
            assert (lg.kind, lg.width) == (kind, width)
    return True


def rows(lists, labels=None):
    """A labelled graph from successor lists; labels default to 1 + the arc's index."""
    n = len(lists)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]) if n else np.zeros(1)
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if n and off[-1] else np.empty(0, np.int64)
    return LM.make(off, adj, np.arange(1, len(adj) + 1) if labels is None else labels)


@pytest.fixture(scope="module")
def cnr_labelled(cnr_csr):
    deg, succ = cnr_csr
    off = np.concatenate([[0], np.cumsum(deg.astype(np.int64))])
    g = LM.make(off, succ, np.zeros(len(succ)))
    return LM.make(off, succ, (31 * LM.sources(g) + succ) % (1 << 13))


@pytest.fixture(scope="module")
def cnr_lg(W, cnr_labelled):
    g = lgraph(W, cnr_labelled, FIXED, 13)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cnr_transposed(cnr_labelled):
    return LM.transpose(cnr_labelled)


def stored(W, tools, g, kind, width):
    """The graph compressed by the tooling and opened as a BitStreamArcLabelledImmutableGraph."""
    st = tools.store((g[0], g[1]))
    bv = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    sl = tools.store_labels(kind, width, g[2], g[0])
    return W.BitStreamArcLabelledImmutableGraph.from_memory(bv, kind, width, sl.stream, sl.offsets)


# ---- from_csr / get / underlying

@pytest.mark.parametrize("kind, width", [(GAMMA, 0), (FIXED, 9)])
def test_round_trip_and_the_smallest_graphs(W, kind, width):
    rng = np.random.default_rng(1)
    g = LM.random_graph(rng, 300, 0.05, heavy=True, lab_max=(1 << 9) - 1)
    assert holds(lgraph(W, g, kind, width), g, kind, width)
    for small in (rows([]), rows([[]]), rows([[0]]), rows([[], [0, 1], []])):
        assert holds(lgraph(W, small, kind, width), small, kind, width)
    with lgraph(W, g, kind, width) as lg, lg.underlying() as u:
        off, adj = u.csr()
        assert np.array_equal(off, g[0]) and np.array_equal(adj, g[1]) and u.num_nodes() == 300
        want = W.ParsedGraph.from_csr(g[0], g[1]).store()
        got = u.store()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])    # bvg_text_store applies to it


def test_from_csr_refuses_what_the_unlabelled_path_refuses(W):
    u64, three = np.uint64, np.array([0, 1, 2], np.int64)
    for off, adj in [(np.array([0, 2, 3], u64), np.array([1, 1, 0], np.int64)),       # duplicate successor
                     (np.array([0, 2], u64), np.array([0, 5], np.int64)),             # successor outside the graph
                     (np.array([0, 1000000, 3], u64), three),                         # a list that ends beyond adj_off[nodes]
                     (np.array([0, 2, 1, 3], u64), three),                            # offsets that decrease
                     (np.array([0, 5, 4, 3], u64), three),                            # ... and start beyond the end as well
                     (np.array([1, 2, 3], u64), np.array([0, 0, 1], np.int64)),       # adj_off[0] != 0
                     (np.array([0, 2, 3], u64), np.array([-1, 0, 1], np.int64)),      # a negative successor
                     (np.array([0, 2, 3], u64), np.array([1, 0, 1], np.int64))]:      # a decreasing pair
        with pytest.raises(W.IllegalArgumentException):
            W.ParsedGraph.from_csr(off, adj)                                          # the yardstick refuses it ...
        with pytest.raises(W.IllegalArgumentException):
            W.LabelledGraph.from_csr(off, adj, np.zeros(len(adj), np.int32), GAMMA)   # ... and so does the labelled path


def test_from_csr_refuses_labels_outside_their_class(W):
    g = rows([[0, 1], [1]])
    for labels, kind, width in [([0, -1, 2], GAMMA, 0),                               # a negative gamma label
                                ([0, 8, 2], FIXED, 3),                                # a fixed label equal to 2^width
                                ([0, 0, 1], FIXED, 0),                                # width 0 with a non-zero label
                                ([0, -1, 0], FIXED, 31)]:
        with pytest.raises(W.IllegalArgumentException):
            W.LabelledGraph.from_csr(g[0], g[1], labels, kind, width)
    for labels, kind, width in [([0, 7, 2], FIXED, 3), ([0, 0, 0], FIXED, 0), ([0, (1 << 31) - 1, 5], FIXED, 31), ([0, (1 << 31) - 1, 5], GAMMA, 0)]:
        assert holds(W.LabelledGraph.from_csr(g[0], g[1], labels, kind, width), LM.make(g[0], g[1], labels))
    with pytest.raises(W.IllegalArgumentException):
        W.LabelledGraph.from_csr(g[0], g[1], [0, 0, 0], FIXED, 32)
    with pytest.raises(W.UnsupportedOperationException):
        W.LabelledGraph.from_csr(g[0], g[1], [0, 0, 0], LIST, 3)


def test_device_forms_and_the_capacity_contract(W):
    g = LM.random_graph(np.random.default_rng(2), 200, 0.1, lab_max=100)
    n, m = 200, len(g[1])
    d_off, d_adj, d_lab = DeviceBytes(g[0].tobytes()), DeviceBytes(g[1].tobytes()), DeviceBytes(g[2].tobytes())
    bad = g[2].copy(); bad[m // 2] = -3
    d_bad = DeviceBytes(bad.tobytes())
    o_off, o_adj, o_lab = DeviceBytes(bytes(8 * (n + 1))), DeviceBytes(bytes(8 * m)), DeviceBytes(bytes(4 * m))
    try:
        with pytest.raises(W.IllegalArgumentException):
            W.LabelledGraph.from_csr_dev(n, d_off.ptr, d_adj.ptr, d_bad.ptr, GAMMA)
        with W.LabelledGraph.from_csr_dev(n, d_off.ptr, d_adj.ptr, d_lab.ptr, GAMMA) as lg:
            L = W.labelled._labelled_fns()
            for caps in ((n, m, m), (n + 1, m - 1, m), (n + 1, m, m - 1)):
                assert L.bvg_lgraph_get_dev(lg._h, o_off.ptr, caps[0], o_adj.ptr, caps[1], o_lab.ptr, caps[2]) == W.E_CAPACITY
            assert not o_off.get().any() and not o_adj.get().any() and not o_lab.get().any()          # nothing was written
            lg.csr_dev(o_off.ptr, n + 1, o_adj.ptr, m, o_lab.ptr, m)
            assert o_off.get().tobytes() == g[0].tobytes() and o_adj.get().tobytes() == g[1].tobytes() and o_lab.get().tobytes() == g[2].tobytes()
            stream, offsets = lg.store_labels()
            s_dev, l_dev = DeviceBytes(bytes(len(stream))), DeviceBytes(bytes(8 * (n + 1)))
            try:
                nb = C.c_uint64()
                assert L.bvg_lgraph_store_labels_dev(lg._h, s_dev.ptr, len(stream) - 1, C.byref(nb), l_dev.ptr) == W.E_CAPACITY and nb.value == len(stream)
                assert not s_dev.get().any()
                assert lg.store_labels_dev(s_dev.ptr, len(stream), l_dev.ptr) == len(stream)
                assert s_dev.get().tobytes() == stream.tobytes() and l_dev.get().tobytes() == offsets.tobytes()
            finally:
                s_dev.free(); l_dev.free()
    finally:
        for d in (d_off, d_adj, d_lab, d_bad, o_off, o_adj, o_lab):
            d.free()


@pytest.mark.parametrize("kind, width", [(GAMMA, 0), (FIXED, 11)])
def test_from_graph_equals_the_arrays_it_was_built_from(W, tools, kind, width):
    g = LM.random_graph(np.random.default_rng(3), 400, 0.04, heavy=True, lab_max=(1 << 11) - 1)
    bs = stored(W, tools, g, kind, width)
    try:
        assert holds(W.LabelledGraph.from_graph(bs), g, kind, width)
        assert holds(W.transpose_labelled(bs), LM.transpose(g), kind, width)          # a source is converted once
    finally:
        bs.close(); bs.g.close()


def test_a_list_labelled_graph_is_refused(W, tools):
    g = rows([[0, 1], [1]])
    st = tools.store((g[0], g[1]))
    bv = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    sl = tools.store_label_lists(5, np.array([0, 1, 3, 3], np.uint64), np.array([1, 2, 3], np.int32), g[0])
    bs = W.BitStreamArcLabelledImmutableGraph.from_memory(bv, LIST, 5, sl.stream, sl.offsets)
    try:
        with pytest.raises(W.UnsupportedOperationException):
            W.LabelledGraph.from_graph(bs)
    finally:
        bs.close(); bv.close()
    with pytest.raises(W.IllegalArgumentException):
        W.transpose_labelled([[0]])


# ---- transpose

def test_transpose_small_shapes(W):
    for g in (rows([[0], [], [0, 1, 3], []]),                                         # loops, empty rows, node 3 only a target
              rows([]), rows([[]]), rows([[0]]),
              LM.from_arcs(5001, np.arange(1, 5001), np.zeros(5000), np.arange(5000) % 97)):   # a star: the centre has 5 000 predecessors
        t = LM.transpose(g)
        assert holds(W.transpose_labelled(lgraph(W, g)), t, GAMMA, 0)
        with W.transpose_labelled(lgraph(W, g)) as once:
            assert holds(W.transpose_labelled(once), g)                                # twice: the original, labels included


def test_transpose_of_cnr(W, cnr_lg, cnr_transposed):
    with W.transpose_labelled(cnr_lg) as t:
        off, adj, lab = t.csr()
        assert (t.kind, t.width) == (FIXED, 13)
        assert np.array_equal(off, cnr_transposed[0]) and np.array_equal(adj, cnr_transposed[1]) and np.array_equal(lab, cnr_transposed[2])
        bv = W.BVGraph.load(CNR)
        try:
            with t.underlying() as u, W.transpose_graph(bv) as want:
                assert all(np.array_equal(p, q) for p, q in zip(u.csr(), want.csr()))
        finally:
            bv.close()


# ---- union

def _union_cases():
    big = list(range(0, 10000, 2))                                                    # one row of 5 000 successors
    n = 10000
    def pad(lists):
        return lists + [[] for _ in range(n - len(lists))]
    return [("empty-empty", rows([[], []]), rows([[], []])),
            ("empty-nonempty", rows([[], [0]]), rows([[0, 1], [0, 1]])),
            ("nonempty-empty", rows([[0, 1], [0, 1]]), rows([[], [0]])),
            ("identical", rows([[0, 2], [1], []], [5, 6, 7]), rows([[0, 2], [1], []], [1, 9, 7])),
            ("disjoint", rows([[0, 2], [0], []]), rows([[1], [1, 2], [2]])),
            ("interleaved", rows([[0, 2, 4, 6], [1, 2, 3], [], [3], [], [], [], []]), rows([[1, 2, 3, 5, 7], [0, 2, 4], [0], [], [], [], [], [7]])),
            ("giant-against-1", rows(pad([big])), rows(pad([[4]]), [3])),
            ("giant-against-2", rows(pad([[3, 4]]), [0, 1]), rows(pad([big]))),
            ("more-nodes-in-b", rows([[0, 1], [1]]), rows([[1], [], [0, 3], [3]])),
            ("more-nodes-in-a", rows([[1], [], [0, 3], [3]]), rows([[0, 1], [1]])),
            ("no-nodes-in-a", rows([]), rows([[0, 1], [1]]))]


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name, a, b", _union_cases(), ids=[c[0] for c in _union_cases()])
def test_union_rows(W, strategy, name, a, b):
    want = LM.union(a, b, strategy)
    with lgraph(W, a) as ga, lgraph(W, b) as gb:
        assert holds(W.union_labelled(ga, gb, strategy), want, GAMMA, 0)
        da, db = LM.to_dict(a), LM.to_dict(b)
        assert int(want[0][-1]) == len(da) + len(db) - len(set(da) & set(db))
        with W.union_labelled(ga, gb, strategy) as u, u.underlying() as uu, ga.underlying() as ua, gb.underlying() as ub, W.union(ua, ub) as plain:
            assert all(np.array_equal(p, q) for p, q in zip(uu.csr(), plain.csr()))    # the underlying result is the unlabelled union


def test_keep_first_differs_exactly_on_common_arcs_with_different_labels(W):
    rng = np.random.default_rng(4)
    a, b = LM.random_graph(rng, 150, 0.2, lab_max=3), LM.random_graph(rng, 170, 0.2, heavy=True, lab_max=3)
    with lgraph(W, a) as ga, lgraph(W, b) as gb, W.union_labelled(ga, gb) as ab, W.union_labelled(gb, ga) as ba:
        (o1, s1, l1), (o2, s2, l2) = ab.csr(), ba.csr()
        assert np.array_equal(o1, o2) and np.array_equal(s1, s2)
        da, db = LM.to_dict(a), LM.to_dict(b)
        src = LM.sources((o1, s1, l1))
        got = {(int(x), int(y)) for x, y in zip(src[l1 != l2], s1[l1 != l2])}
        assert got == {k for k in set(da) & set(db) if da[k] != db[k]} and got
        assert ab.num_arcs() == len(da) + len(db) - len(set(da) & set(db))


def _exact(rng, n, arcs):
    """A labelled graph of n nodes with exactly `arcs` arcs."""
    cells = rng.choice(n * n, size=arcs, replace=False)
    return LM.from_arcs(n, cells // n, cells % n, rng.integers(0, 1000, arcs))


@pytest.mark.parametrize("arcs", [255, 256, 257, 65535, 65536, 65537])
def test_sizes_around_the_blocks_of_the_prefix_sum(W, tools, arcs):
    """Arc counts and row starts one below, at and above 256 and 65 536: the workgroup size and the tile of the shared prefix sum."""
    rng = np.random.default_rng(arcs)
    n = 40 if arcs < 1000 else 400
    a, b = _exact(rng, n, arcs), _exact(rng, n, arcs)
    with lgraph(W, a) as ga, lgraph(W, b) as gb:
        assert holds(W.union_labelled(ga, gb, LM.MAX), LM.union(a, b, LM.MAX))
        assert holds(W.union_labelled(ga, ga, LM.MIN), a)                              # every arc common: exactly `arcs` arcs out
        assert holds(W.transpose_labelled(ga), LM.transpose(a))
        assert holds(W.filter_labelled_arcs(ga, "LOWER_BOUND", lower_bound=500), LM.filter(a, LM.LOWER_BOUND, lower_bound=500))
        stream, offsets = ga.store_labels()
    sl = tools.store_labels(GAMMA, 0, a[2], a[0])
    assert stream.tobytes() == sl.stream.tobytes() and np.array_equal(offsets, sl.offsets)


def test_union_refuses_differing_classes(W):
    g = rows([[0, 1], [1]], [1, 0, 1])
    with lgraph(W, g, GAMMA) as a, lgraph(W, g, FIXED, 3) as b, lgraph(W, g, FIXED, 4) as c:
        for x, y in ((a, b), (b, a), (b, c)):
            with pytest.raises(W.IllegalArgumentException):
                W.union_labelled(x, y)
        assert holds(W.union_labelled(b, b), g, FIXED, 3)
        with pytest.raises(W.IllegalArgumentException):
            W.union_labelled(a, a, "SUM")


# ---- symmetrize

def test_symmetrize_of_cnr_keeps_the_graphs_labels(W, cnr_lg, cnr_labelled, cnr_transposed):
    want = LM.union(cnr_labelled, cnr_transposed, LM.KEEP_FIRST)
    with W.symmetrize_labelled(cnr_lg) as s:
        off, adj, lab = s.csr()
        assert np.array_equal(off, want[0]) and np.array_equal(adj, want[1]) and np.array_equal(lab, want[2])
        n = N_CNR
        keys = LM.sources((off, adj, lab)) * n + adj
        gk = LM.sources(cnr_labelled) * n + cnr_labelled[1]
        assert np.array_equal(lab[np.searchsorted(keys, gk)], cnr_labelled[2])          # (x, y) keeps g's label wherever g has the arc
    with W.transpose_labelled(cnr_lg) as t, W.union_labelled(cnr_lg, t) as u:
        assert holds(u, want, FIXED, 13)                                               # union with the transpose: the same graph


def test_symmetrize_with_min_is_label_symmetric(W, cnr_lg, cnr_labelled, cnr_transposed):
    want = LM.union(cnr_labelled, cnr_transposed, LM.MIN)
    with W.symmetrize_labelled(cnr_lg, LM.MIN) as s:
        off, adj, lab = s.csr()
        assert np.array_equal(off, want[0]) and np.array_equal(adj, want[1]) and np.array_equal(lab, want[2])
        t = LM.transpose((off, adj, lab))
        assert np.array_equal(t[1], adj) and np.array_equal(t[2], lab)


# ---- filter

def test_lower_bound_follows_the_code_not_the_javadoc(W):
    g = LM.random_graph(np.random.default_rng(5), 200, 0.15, heavy=True, lab_max=20)
    top = int(g[2].max())
    with lgraph(W, g) as lg:
        assert holds(W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=0), g)                          # all kept
        none = W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=top + 1)
        assert none.num_nodes() == 200 and none.num_arcs() == 0 and holds(none, LM.filter(g, LM.LOWER_BOUND, lower_bound=top + 1))
        assert holds(W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=-7), g)                         # a negative bound
        with W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=top) as f:                             # a label present: kept (>=)
            assert f.num_arcs() == int((g[2] == top).sum()) > 0
        for bound in (1, 7, top):
            assert holds(W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=bound), LM.filter(g, LM.LOWER_BOUND, lower_bound=bound))
        with pytest.raises(W.IllegalArgumentException):
            W.filter_labelled_arcs(lg, "NO_LOOPS", lower_bound=3)
        with pytest.raises(W.IllegalArgumentException):
            W.filter_labelled_arcs(lg, "LOWER_BOUND")
        with pytest.raises(W.IllegalArgumentException):
            W.filter_labelled_arcs(lg, "LOWER_BOUND", node_class=np.zeros(200), lower_bound=1)


def test_no_loops_and_class_filters_carry_the_labels(W):
    rng = np.random.default_rng(6)
    g = LM.random_graph(rng, 250, 0.1, heavy=True, lab_max=1000)
    cls = rng.integers(0, 3, 250)
    with lgraph(W, g, FIXED, 10) as lg:
        assert holds(W.filter_labelled_arcs(lg, "NO_LOOPS"), LM.filter(g, LM.NO_LOOPS), FIXED, 10)
        assert holds(W.filter_labelled_arcs(lg, "SAME_CLASS", node_class=cls), LM.filter(g, LM.SAME_CLASS, node_class=cls), FIXED, 10)
        assert holds(W.filter_labelled_arcs(lg, "DIFFERENT_CLASS", node_class=cls), LM.filter(g, LM.DIFFERENT_CLASS, node_class=cls), FIXED, 10)
        with pytest.raises(W.IllegalArgumentException):
            W.filter_labelled_arcs(lg, "SAME_CLASS", node_class=cls[:-1])
        with pytest.raises(W.IllegalArgumentException):
            W.filter_labelled_arcs(lg, "NO_LOOPS", node_class=cls)


# ---- the label writer

def spread(labels, rng, n=None):
    """A graph whose arcs carry `labels` in order: rows of random lengths, with nodes without arcs at the start, in the middle and at the end."""
    m = len(labels)
    n = n or max(8, int(np.sqrt(m)) + 6)
    lens = []
    left = m
    while left:
        lens.append(int(min(left, rng.integers(1, n - 1))))
        left -= lens[-1]
        if rng.random() < 0.3:
            lens.append(0)
    lens = [0, 0] + lens[:len(lens) // 2] + [0, 0, 0] + lens[len(lens) // 2:] + [0]
    n = max(n, len(lens))
    lens += [0] * (n - len(lens))
    return rows([list(range(l)) for l in lens], labels)


def writes_like_the_tooling(W, tools, g, kind, width):
    sl = tools.store_labels(kind, width, g[2], g[0])
    with lgraph(W, g, kind, width) as lg:
        stream, offsets = lg.store_labels()
    assert len(stream) == len(sl.stream) == (int(sl.offsets[-1]) + 7) // 8
    assert stream.tobytes() == sl.stream.tobytes(), "label stream differs"
    assert np.array_equal(offsets, sl.offsets), "label offsets differ"
    return True


@pytest.mark.parametrize("width", [0, 1, 7, 8, 13, 31])
def test_writer_fixed_widths(W, tools, width):
    rng = np.random.default_rng(width)
    top = (1 << width) - 1
    for labels in (np.zeros(300), np.full(300, top), rng.integers(0, top + 1, 777), np.array([top, 0] * 40 + [top])):
        assert writes_like_the_tooling(W, tools, spread(labels, rng), FIXED, width)
    if width == 0:
        with lgraph(W, spread(np.zeros(50), rng), FIXED, 0) as lg:
            stream, offsets = lg.store_labels()
            assert len(stream) == 0 and not offsets.any()                              # an empty stream, offsets all zero


def test_writer_gamma_codes_at_every_bit_of_a_word(W, tools):
    """0, 1, 2^k - 2, 2^k - 1, 2^k for k up to 30 and 2^31 - 1 (a 63-bit code): each one starting at every bit of a 64-bit word, so that it also
    straddles the word's border wherever it is longer than what is left."""
    rng = np.random.default_rng(31)
    specials = sorted({0, 1, (1 << 31) - 1} | {v for k in range(1, 31) for v in ((1 << k) - 2, (1 << k) - 1, 1 << k)})
    length = lambda v: 2 * (int(v + 1).bit_length() - 1) + 1
    for part in (specials[:24], specials[24:48], specials[48:72], specials[72:]):
        labels, pos, starts = [], 0, set()
        for v in part:
            for target in range(64):
                k = (target - pos) % 64
                labels += [0] * k; pos += k                                            # gamma(0) is one bit
                starts.add((v, pos % 64))
                labels.append(v); pos += length(v)
        assert len(starts) == 64 * len(part)
        assert writes_like_the_tooling(W, tools, spread(np.array(labels), rng), GAMMA, 0)
    assert length((1 << 31) - 1) == 63
    assert writes_like_the_tooling(W, tools, spread(np.full(130, (1 << 31) - 1), rng), GAMMA, 0)


def test_writer_stream_ends(W, tools):
    """Streams that end on the last bit of a byte and of a 64-bit word, and one bit after; a graph without arcs; arc counts around 256 and 65 536."""
    rng = np.random.default_rng(9)
    for m in (7, 8, 9, 63, 64, 65, 127, 128, 129):
        assert writes_like_the_tooling(W, tools, spread(rng.integers(0, 2, m), rng), FIXED, 1)
        assert writes_like_the_tooling(W, tools, spread(np.zeros(m), rng), GAMMA, 0)
    for empty in (rows([]), rows([[]]), rows([[], [], []])):
        assert writes_like_the_tooling(W, tools, empty, GAMMA, 0) and writes_like_the_tooling(W, tools, empty, FIXED, 5)
    for m in (255, 256, 257, 65535, 65536, 65537):
        assert writes_like_the_tooling(W, tools, spread(rng.integers(0, 1 << 13, m), rng), FIXED, 13)
        assert writes_like_the_tooling(W, tools, spread(rng.integers(0, 5000, m), rng), GAMMA, 0)


def test_writer_on_cnr(W, tools, cnr_lg, cnr_labelled):
    sl = tools.store_labels(FIXED, 13, cnr_labelled[2], cnr_labelled[0])
    stream, offsets = cnr_lg.store_labels()
    assert stream.tobytes() == sl.stream.tobytes() and np.array_equal(offsets, sl.offsets)


# ---- files

@pytest.mark.parametrize("kind, width", [(GAMMA, 0), (FIXED, 12)])
def test_write_then_load(W, tmp_path, kind, width):
    g = LM.random_graph(np.random.default_rng(10), 500, 0.03, heavy=True, lab_max=(1 << 12) - 1)
    base = str(tmp_path / "lab")
    with lgraph(W, g, kind, width) as lg:
        lg.write(base)
    props = dict(tuple(s.strip() for s in line.split("=", 1)) for line in open(base + ".properties").read().splitlines())
    assert props == {"graphclass": "it.unimi.dsi.big.webgraph.labelling.BitStreamArcLabelledImmutableGraph",
                     "underlyinggraph": base + "-underlying",                          # an absolute destination keeps its path (Transform.java:2376)
                     "labelspec": "it.unimi.dsi.big.webgraph.labelling." + ("GammaCodedIntLabel(FOO)" if kind == GAMMA else "FixedWidthIntLabel(FOO,12)")}
    bs = W.BitStreamArcLabelledImmutableGraph.load(base)
    try:
        deg, succ, lab = bs.decode_range(0, 500)
        assert np.array_equal(np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), g[0].astype(np.int64))
        assert np.array_equal(succ, g[1]) and np.array_equal(lab, g[2])
    finally:
        bs.close(); bs.g.close()
    bv = W.BVGraph.load(base + "-underlying")
    try:
        assert bv.num_nodes() == 500 and bv.num_arcs() == len(g[1])
    finally:
        bv.close()
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        with lgraph(W, g, kind, width) as lg:
            lg.write("rel")
        assert "underlyinggraph = rel-underlying\n" in open("rel.properties").read()  # a relative one: the file name alone
    finally:
        os.chdir(cwd)
    bs = W.BitStreamArcLabelledImmutableGraph.load(str(tmp_path / "rel"))
    try:
        assert np.array_equal(bs.decode_range(0, 500)[2], g[2])
    finally:
        bs.close(); bs.g.close()


def _tooling_files(tools, tmp_path, name, g, kind, width):
    base = str(tmp_path / name)
    tools.store((g[0], g[1])).write(base + "-underlying")
    tools.store_labels(kind, width, g[2], g[0]).write(base, name + "-underlying")
    return base


def _loaded(W, base, n):
    bs = W.BitStreamArcLabelledImmutableGraph.load(base)
    try:
        deg, succ, lab = bs.decode_range(0, n)
        return LM.make(np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ, lab)
    finally:
        bs.close(); bs.g.close()


def test_command_line_on_files_written_by_the_tooling(W, tools, tmp_path, capsys):
    rng = np.random.default_rng(11)
    a, b = LM.random_graph(rng, 300, 0.05, heavy=True, lab_max=255), LM.random_graph(rng, 300, 0.05, lab_max=255)
    fa, fb = _tooling_files(tools, tmp_path, "a", a, FIXED, 8), _tooling_files(tools, tmp_path, "b", b, FIXED, 8)
    out = str(tmp_path / "out")
    assert W.labelled_transform_main(["transposeOffline", fa, out + "-t"]) == 0
    assert LM.equal(_loaded(W, out + "-t", 300), LM.transpose(a))
    assert W.labelled_transform_main(["symmetrizeOffline", fa, out + "-s", "MIN"]) == 0
    assert LM.equal(_loaded(W, out + "-s", 300), LM.symmetrize(a, LM.MIN))
    assert W.labelled_transform_main(["union", fa, fb, out + "-u", "KEEP_FIRST"]) == 0
    assert LM.equal(_loaded(W, out + "-u", 300), LM.union(a, b))
    assert W.labelled_transform_main(["larcfilter", fa, out + "-f", "LowerBound(100)"]) == 0
    assert LM.equal(_loaded(W, out + "-f", 300), LM.filter(a, LM.LOWER_BOUND, lower_bound=100))
    assert W.labelled_transform_main(["larcfilter", fa, out + "-n", "NO_LOOPS"]) == 0
    assert LM.equal(_loaded(W, out + "-n", 300), LM.filter(a, LM.NO_LOOPS))
    capsys.readouterr()
    assert W.labelled_transform_main(["larcfilter", fa + "-underlying", out + "-x", "NO_LOOPS"]) == 1
    assert "Filtering on labelled arcs requires a labelled graph" in capsys.readouterr().err
