"""GPU: Transform on the device (bvg_transform_*), list for list against the model (tests/transform_model.py).  The yardsticks that exist
stay the yardsticks: the golden text for what a graph holds, BVGraph.transpose / symmetrize for the transposed and symmetrised graphs,
bvg_store's refusals for what from_csr refuses.

The lexicographic order is the one the reference's comparator computes (the larger successor first, Transform.java:2028-2029), not the
one its javadoc describes; tests/test_transform_model.py pins the model's keys to both comparators."""
import ctypes as C

import numpy as np
import pytest

import transform_model as M
from conftest import CNR
from test_gpu_text import DeviceBytes

pytestmark = pytest.mark.gpu

N_CNR = 325557


@pytest.fixture(scope="module")
def cnr(W):
    g = W.BVGraph.load(CNR)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cnr_model(cnr_csr):
    deg, succ = cnr_csr
    return np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ


@pytest.fixture(scope="module")
def cnr_parsed(W, cnr_model):
    g = W.ParsedGraph.from_csr(*cnr_model)
    yield g
    g.close()


@pytest.fixture(scope="module")
def cnr_perm(cnr_model):
    rng = np.random.default_rng(2000)
    perm = rng.permutation(N_CNR).astype(np.int64)
    inv = np.empty_like(perm); inv[perm] = np.arange(N_CNR)
    return perm, inv


def graph_of(W, lists):
    return W.ParsedGraph.from_csr(*M.csr(lists))


def holds(g, want):
    """The resident graph holds the model's lists (and closes)."""
    with g:
        off, adj = g.csr()
        assert g.num_nodes() == len(want[0]) - 1 and g.num_arcs() == len(adj) == int(off[-1])
        assert np.array_equal(off.astype(np.int64), np.asarray(want[0]).astype(np.int64)), "offsets differ"
        assert np.array_equal(adj, want[1]), "successors differ"
    return True


def random_lists(rng, n, dens=None):
    dens = rng.choice([0.0, 0.02, 0.2, 0.6]) if dens is None else dens
    return [np.flatnonzero(rng.random(n) < dens) for _ in range(n)]


# ---- from_csr / identity

def test_identity_of_cnr_is_the_golden_text(W, cnr, cnr_model):
    assert holds(W.identity_graph(cnr), cnr_model)


def test_from_csr_and_identity_of_a_resident_graph(W, cnr_parsed, cnr_model):
    assert cnr_parsed.num_nodes() == N_CNR and cnr_parsed.num_arcs() == len(cnr_model[1])
    assert holds(W.identity_graph(cnr_parsed), cnr_model)
    assert holds(graph_of(W, []), M.csr([])) and holds(graph_of(W, [[]]), M.csr([[]])) and holds(graph_of(W, [[0]]), M.csr([[0]]))


def test_from_csr_refuses_what_bvg_store_refuses(W):
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
            W.store((off, adj), W.default_params())                                   # the yardstick refuses it ...
        with pytest.raises(W.IllegalArgumentException):
            W.ParsedGraph.from_csr(off, adj)                                          # ... and so does from_csr


def test_from_csr_dev(W, cnr_model):
    bad = cnr_model[1].copy(); bad[5] = N_CNR
    off, adj, bad = DeviceBytes(cnr_model[0].tobytes()), DeviceBytes(cnr_model[1].tobytes()), DeviceBytes(bad.tobytes())
    try:
        assert holds(W.ParsedGraph.from_csr_dev(N_CNR, off.ptr, adj.ptr), cnr_model)
        with pytest.raises(W.IllegalArgumentException):
            W.ParsedGraph.from_csr_dev(N_CNR, off.ptr, bad.ptr)
    finally:
        off.free(); adj.free(); bad.free()


# ---- map

@pytest.mark.parametrize("lists, f", [
    ([], []),                                                       # n = 0
    ([[0]], [0]),                                                   # one node with a loop
    ([[0]], [3]),                                                   # ... renamed beyond n
    ([[1, 2], [0], [2]], [-1, -1, -1]),                             # every entry -1: 0 nodes
    ([[1, 2], [3], [0, 3], [1]], [0, 0, 1, 1]),                     # images merge: duplicate arcs and a loop
    ([[1], [2], [0]], [5, 1, 0]),                                   # a value >= n: empty tail nodes
    ([[2], [2], []], [0, 1, -1]),                                   # -1 on a node that is only a target
    ([[1], [0]], [1, 0]),
])
def test_map_hand_cases(W, lists, f):
    with graph_of(W, lists) as g:
        assert holds(W.map_graph(g, f), M.map_graph(*M.csr(lists), f))


def test_map_refusals_leave_out_untouched(W):
    L = W.transform._transform_fns()
    with graph_of(W, [[1], [0], []]) as g:
        src = W.TransformSrc(None, g._h)
        h = C.c_void_p(0x1234)
        short, low = np.array([0, 1], np.int64), np.array([0, -2, 1], np.int64)
        assert L.bvg_transform_map(C.byref(src), short.ctypes.data, 2, C.byref(h)) == W.E_ARG       # wrong length
        assert L.bvg_transform_map(C.byref(src), low.ctypes.data, 3, C.byref(h)) == W.E_ARG         # a value below -1
        assert h.value == 0x1234
        with pytest.raises(W.IllegalArgumentException):
            W.map_graph(g, [0, 1, 2, 3])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_map_random_partial_maps(W, n):
    rng = np.random.default_rng(n)
    lists = random_lists(rng, n, 0.05 if n > 300 else None)
    for trial in range(3):
        f = rng.integers(-1, [n, max(1, n // 3), n + 40][trial], size=n)
        with graph_of(W, lists) as g:
            assert holds(W.map_graph(g, f), M.map_graph(*M.csr(lists), f)), (n, trial)


def test_map_and_filter_dev(W):
    rng = np.random.default_rng(3)
    lists = random_lists(rng, 200, 0.1)
    f = rng.integers(-1, 150, size=200)
    L = W.transform._transform_fns()
    d = DeviceBytes(f.astype(np.int64).tobytes())
    try:
        with graph_of(W, lists) as g:
            h = C.c_void_p()
            assert L.bvg_transform_map_dev(C.byref(W.TransformSrc(None, g._h)), d.ptr, 200, C.byref(h)) == 0
            assert holds(W.ParsedGraph(h), M.map_graph(*M.csr(lists), f))
            cls = DeviceBytes((f % 3).astype(np.int64).tobytes())
            assert L.bvg_transform_filter_dev(C.byref(W.TransformSrc(None, g._h)), W.TRANSFORM_SAME_CLASS, cls.ptr, 200, C.byref(h)) == 0
            cls.free()
            assert holds(W.ParsedGraph(h), M.filter_arcs(*M.csr(lists), "SAME_CLASS", f % 3))
    finally:
        d.free()


def test_map_cnr_by_a_permutation_and_back(W, cnr, cnr_model, cnr_perm):
    perm, inv = cnr_perm
    want = M.map_graph(*cnr_model, perm)
    with W.map_graph(cnr, perm) as mapped:
        off, adj = mapped.csr()
        assert M.same((off, adj), want)
        assert holds(W.map_graph(mapped, inv), cnr_model)            # every list identical to the fixture


def test_store_of_a_mapped_cnr_decodes_to_the_model(W, cnr_parsed, cnr_model, cnr_perm):
    want = M.map_graph(*cnr_model, cnr_perm[0])
    with W.map_graph(cnr_parsed, cnr_perm[0]) as mapped:
        graph, offsets = mapped.store()
    p = W.default_params(nodes=N_CNR, arcs=len(want[1]))
    g = W.BVGraph.from_memory(p, graph, offsets)
    try:
        deg, succ = g.decode_range(0, N_CNR)
    finally:
        g.close()
    assert np.array_equal(deg, np.diff(want[0])) and np.array_equal(succ, want[1])


# ---- filter

@pytest.mark.parametrize("kind", ["NO_LOOPS", "SAME_CLASS", "DIFFERENT_CLASS"])
def test_filter_cnr_and_loops_only(W, cnr, cnr_model, kind):
    rng = np.random.default_rng(17)
    for src, model, n in ((cnr, cnr_model, N_CNR), (None, M.csr([[x] for x in range(300)]), 300)):
        cls = None if kind == "NO_LOOPS" else rng.integers(0, 4, size=n)
        g = src if src is not None else W.ParsedGraph.from_csr(*model)
        try:
            assert holds(W.filter_arcs(g, kind, cls), M.filter_arcs(*model, kind, cls))
        finally:
            if src is None:
                g.close()


def test_filter_refusals(W):
    with graph_of(W, [[1], [0], []]) as g:
        with pytest.raises(W.IllegalArgumentException):
            W.filter_arcs(g, "SAME_CLASS", [0, 1])                   # class_len mismatch
        with pytest.raises(W.IllegalArgumentException):
            W.filter_arcs(g, "DIFFERENT_CLASS")                      # no classes at all
        with pytest.raises(W.IllegalArgumentException):
            W.filter_arcs(g, "NO_LOOPS", [0, 1, 2])                  # classes with NO_LOOPS


# ---- transpose / symmetrize / simplify

def test_transpose_and_symmetrize_are_what_bvgraph_returns(W, cnr, cnr_parsed, cnr_model):
    toff, tsucc = cnr.transpose()
    soff, ssucc = cnr.symmetrize()
    for src in (cnr, cnr_parsed):                                    # a BVGraph source and a ParsedGraph source: the same contents
        assert holds(W.transpose_graph(src), (toff, tsucc))
        assert holds(W.symmetrize_graph(src), (soff, ssucc))
    assert M.same(M.transpose(*cnr_model), (toff, tsucc)) and M.same(M.symmetrize(*cnr_model), (soff, ssucc))


def test_simplified_graph_is_symmetric_and_loopless(W, cnr, cnr_model):
    with W.simplify_graph(cnr) as s:
        off, adj = s.csr()
        assert M.same((off, adj), M.symmetrize(*cnr_model, drop_loops=True))
        src, dst = M.arcs_of(off, adj)
        assert not np.any(src == dst)
        assert holds(W.transpose_graph(s), (off, adj))


def test_transpose_small(W):
    for lists in ([], [[]], [[0]], [[1, 2], [1], [0]], [[], [], [0, 1, 2]]):
        with graph_of(W, lists) as g:
            assert holds(W.transpose_graph(g), M.transpose(*M.csr(lists)))
            assert holds(W.symmetrize_graph(g), M.symmetrize(*M.csr(lists)))
            assert holds(W.simplify_graph(g), M.symmetrize(*M.csr(lists), drop_loops=True))


# ---- union

def test_union(W):
    rng = np.random.default_rng(23)
    small, big = random_lists(rng, 70, 0.1), random_lists(rng, 300, 0.03)
    for la, lb in ((small, big), (big, small), (big, []), ([], big), (big, big), ([], []), (small, [[0]] * 70)):
        a, b = M.csr(la), M.csr(lb)
        with graph_of(W, la) as ga, graph_of(W, lb) as gb:
            assert holds(W.union(ga, gb), M.union(a, b))
            assert holds(W.union(ga, gb, drop_loops=True), M.union(a, b, drop_loops=True))
    with graph_of(W, big) as g:
        assert holds(W.union(g, g), M.csr(big))                      # with itself (one handle, twice)


def test_union_of_cnr_and_its_transpose_is_symmetrize(W, cnr):
    soff, ssucc = cnr.symmetrize()
    with W.transpose_graph(cnr) as t:
        assert holds(W.union(cnr, t), (soff, ssucc))


# ---- permutations

def both_orders(W, lists):
    off, adj = M.csr(lists)
    with W.ParsedGraph.from_csr(off, adj) as g:
        for gray, call in ((False, W.lexicographical_permutation), (True, W.gray_code_permutation)):
            got, want = call(g), M.permutation_of_csr(off, adj, gray)
            assert sorted(got.tolist()) == list(range(len(lists))), "not a bijection"
            assert np.array_equal(got, want), ("gray" if gray else "lex", np.flatnonzero(got != want)[:8])
    return True


@pytest.mark.parametrize("gray", [False, True])
def test_permutation_of_cnr(W, cnr, cnr_model, gray):
    got = (W.gray_code_permutation if gray else W.lexicographical_permutation)(cnr)
    assert np.array_equal(np.sort(got), np.arange(N_CNR))
    want = M.permutation_of_csr(*cnr_model, gray)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_permutation_all_lists_empty(W):
    assert both_orders(W, [[] for _ in range(1000)])
    assert both_orders(W, [])


def test_permutation_equal_long_lists(W):
    """512 identical lists of 2 000 successors and one that differs only in its last element, among empty ones."""
    same = list(range(3, 2003))
    lists = [[] for _ in range(2100)]
    for x in range(40, 40 + 513):
        lists[x] = same
    lists[300] = same[:-1] + [2050]
    assert both_orders(W, lists)


def test_permutation_prefixes_at_even_and_odd_lengths(W):
    """Every prefix of one list, so that for every length a list ends where another continues: inside the head key, at its edge and behind
    it, at even and at odd positions (where the Gray order flips); each prefix twice, for the tie rule."""
    rng = np.random.default_rng(31)
    n = 2000
    base = np.sort(rng.choice(n, size=40, replace=False))
    lists = [[] for _ in range(n)]
    nodes = rng.permutation(n)[:82]
    for j in range(41):
        lists[nodes[2 * j]] = base[:j]; lists[nodes[2 * j + 1]] = base[:j]
    assert both_orders(W, lists)
    assert both_orders(W, [[1, 3], [1, 3, 5], [1, 3, 5, 7], [1], [], [1, 3, 5], [1, 3], [], [1]])


@pytest.mark.parametrize("at", [0, 1, 2, 63, 64, 65, 1300])
def test_permutation_first_difference_at(W, at):
    n = 3000
    common = list(range(10, 10 + at))
    lists = [[] for _ in range(n)]
    lists[7] = common + [2000, 2500]
    lists[1500] = common + [2001, 2400]
    lists[2999] = common + [2001]
    lists[8] = common + [2000, 2500]
    lists[0] = common
    assert both_orders(W, lists)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 257])
def test_permutation_random_graphs(W, n):
    rng = np.random.default_rng(100 + n)
    for dens in (0.0, 0.1, 0.5, 0.9):
        lists = random_lists(rng, n, dens)
        for x in range(0, n, 5):                                     # equal lists, far apart
            lists[x] = lists[(x * 7 + 3) % n]
        assert both_orders(W, lists)


def test_random_permutation(W, cnr_parsed):
    with graph_of(W, [[]] * 1000) as g:
        a, b, c = W.random_permutation(g, 5), W.random_permutation(g, 5), W.random_permutation(g, 6)
        assert sorted(a.tolist()) == list(range(1000)) and np.array_equal(a, b) and not np.array_equal(a, c)
        assert np.array_equal(a, M.random_permutation(1000, 5))
        assert np.array_equal(W.random_permutation(g, -1), M.random_permutation(1000, -1))
    big = W.random_permutation(cnr_parsed, 42)
    assert np.array_equal(np.sort(big), np.arange(N_CNR))
    assert np.array_equal(big[:2000], M.random_permutation(N_CNR, 42)[:2000])


def test_permutation_dev(W):
    rng = np.random.default_rng(8)
    lists = random_lists(rng, 300, 0.2)
    out = DeviceBytes(bytes(300 * 8))
    try:
        with graph_of(W, lists) as g:
            W.permutation_dev(g, W.PERM_GRAY, out.ptr)
        assert np.array_equal(out.get().view(np.int64), M.permutation_of_csr(*M.csr(lists), True))
    finally:
        out.free()


# ---- chain

def test_chain_lex_map_simplify_store(W, tools):
    """map_graph(g, lex) -> simplify_graph -> store: every step takes the resident result of the one before."""
    rng = np.random.default_rng(77)
    lists = random_lists(rng, 500, 0.03)
    model = M.csr(lists)
    want = M.symmetrize(*M.map_graph(*model, M.permutation_of_csr(*model, False)), drop_loops=True)
    with graph_of(W, lists) as g:
        with W.map_graph(g, W.lexicographical_permutation(g)) as mapped, W.simplify_graph(mapped) as simple:
            graph, offsets = simple.store()
            assert M.same(simple.csr(), want)
    ref = tools.store(M.lists_of(*want), W.default_params())
    assert np.array_equal(offsets, ref.offsets) and graph.tobytes() == ref.graph.tobytes()


def test_remove_dangling(W):
    lists = [[1], [], [0, 3], [], [4], []]
    model = M.csr(lists)
    with graph_of(W, lists) as g:
        assert holds(W.remove_dangling(g), M.map_graph(*model, M.remove_dangling_map(model[0])))


def test_transform_main_round_trip(W, tmp_path):
    """The command line: lexPerm, then mapOffline by that file, read back."""
    rng = np.random.default_rng(1)
    lists = random_lists(rng, 120, 0.1)
    model = M.csr(lists)
    src = str(tmp_path / "src")
    with graph_of(W, lists) as g:
        W.write_bvgraph(src, g)
    assert W.transform_main(["lexPerm", src, str(tmp_path / "perm")]) == 0
    perm = W.load_longs(str(tmp_path / "perm"))
    assert np.array_equal(perm, M.permutation_of_csr(*model, False))
    assert W.transform_main(["mapOffline", src, str(tmp_path / "dst"), str(tmp_path / "perm")]) == 0
    assert W.transform_main(["-d", "ASCIIGraph", "simplifyOffline", src, str(tmp_path / "simple"), "1000", str(tmp_path)]) == 0   # batchSize, tempDir: ignored
    want = M.map_graph(*model, perm)
    g2 = W.BVGraph.load(str(tmp_path / "dst"))
    try:
        deg, succ = g2.decode_range(0, g2.num_nodes())
    finally:
        g2.close()
    assert np.array_equal(deg, np.diff(want[0])) and np.array_equal(succ, want[1])
    with W.load_ascii_graph(str(tmp_path / "simple")) as s:
        assert M.same(s.csr(), M.symmetrize(*model, drop_loops=True))
