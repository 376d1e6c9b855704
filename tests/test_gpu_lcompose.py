"""GPU: the labelled graph product on the device (bvg_lcompose), list for list and label for label against the model (tests/lcompose_model.py):
the smallest graphs, the reference's own case under every semiring and from a label stream on disk, unequal node counts, rows built to sit
exactly at, one below and one above each tier's limit (the shapes of tests/test_gpu_compose.py, among them the one that puts every lane of a
row's owner on ONE value slot), every tier forced, tier 2 in batches of one row, a prefix of cnr-2000, the range refusal and what tells a
clamped sum from a wrapped one, determinism, chaining, the files, and the refusals."""
import numpy as np
import pytest

import compose_model as CM
import labelled_model as LM
import lcompose_model as LC
from conftest import CNR  # noqa: F401
from test_gpu_compose import boundary_bounds, boundary_rows, expected_rows, product_graphs, shape_rows

pytestmark = pytest.mark.gpu

GAMMA, FIXED = LC.GAMMA, LC.FIXED
PREFIX = 5000
REFERENCE_ROWS = [[(1, 2), (2, 10), (3, 1)], [(2, 4)], [], [(2, 1)]]          # TransformTest.testLabelledCompose
REFERENCE_LABELS = {LC.MIN_PLUS: 2, LC.MAX_PLUS: 6, LC.MAX_MIN: 2, LC.MIN_MAX: 1, LC.PLUS_TIMES: 9}


def lgraph(W, g, kind=GAMMA, width=0):
    return W.LabelledGraph.from_csr(g[0], g[1], g[2], kind, width)


def same(got, want, what=""):
    off, adj, lab = got
    assert len(off) == len(want[0]), what + ": node counts differ"
    assert np.array_equal(np.asarray(off).astype(np.int64), want[0]), what + ": offsets differ"
    assert np.array_equal(adj, want[1]), what + ": successors differ"
    assert np.array_equal(np.asarray(lab).astype(np.int64), want[2]), what + ": labels differ"
    return True


def check(W, a, b, semiring, kind=GAMMA, width=0, out_width=None, what=""):
    """The device's answer to a o b is the model's: the same graph, or the same refusal with the same count and first arc.  -> the report."""
    want = LC.compose(a, b, semiring, kind, width if out_width is None else out_width)
    with lgraph(W, a, kind, width) as ga, lgraph(W, b, kind, width) as gb:
        if want[0] == "range":
            with pytest.raises(W.IllegalArgumentException) as e:
                W.compose_labelled(ga, gb, semiring, out_width=out_width)
            assert (e.value.out_of_range, e.value.first_arc) == want[1:], what
            assert e.value.report["out_of_range"] == want[1] and "(%d, %d)" % want[2] in str(e.value)
            return e.value.report
        g, rep = W.compose_labelled(ga, gb, semiring, out_width=out_width, report=True)
        with g:
            assert (g.kind, g.width) == (kind, (width if out_width is None else out_width) if kind == FIXED else 0)
            assert g.num_nodes() == len(want[1][0]) - 1 and g.num_arcs() == len(want[1][1]) == rep["arcs"]
            assert same(g.csr(), want[1], what)
        assert rep["out_of_range"] == 0 and (rep["first_row"], rep["first_successor"]) == (-1, -1)
        return rep


def limits(W):
    one = LC.from_rows([[(0, 1)]])
    with lgraph(W, one) as g:
        r, rep = W.compose_labelled(g, g, "MIN_PLUS", report=True)
        r.close()
    assert rep["limit"][0] >= 1 and rep["limit"][1] > rep["limit"][0]
    return rep["limit"]


def labelled_products(rows):
    """product_graphs(rows) with labels: g0's arcs 1..3, g1's arcs all different (1 + the arc's index), so that the lists a row unites differ in
    their labels; small enough for every semiring's result over a few thousand products to stay a GammaCodedIntLabel."""
    g0, g1 = product_graphs(rows)
    a = LC.make(g0[0], g0[1], np.arange(len(g0[1])) % 3 + 1)
    b = LC.make(g1[0], g1[1], np.arange(len(g1[1])) + 1)
    return a, b


# ---- the smallest graphs, the reference's case

@pytest.mark.parametrize("semiring", LC.SEMIRINGS)
def test_smallest_graphs(W, semiring):
    empty = LC.from_rows([])
    check(W, empty, empty, semiring, what="0 nodes")
    check(W, LC.from_rows([[]]), LC.from_rows([[]]), semiring, what="1 node, no arcs")
    check(W, LC.from_rows([[(0, 3)]]), LC.from_rows([[(0, 3)]]), semiring, what="a loop")
    check(W, LC.from_rows([[(0, 3)]]), LC.from_rows([[]]), semiring)
    check(W, LC.from_rows([[], [], []]), LC.from_rows([[(1, 1), (2, 2)], [(0, 3)], [(2, 4)]]), semiring)


@pytest.mark.parametrize("name", sorted(LC.NAMES))
def test_the_references_case_under_every_semiring(W, name):
    g = LC.from_rows(REFERENCE_ROWS)
    with lgraph(W, g) as lg, W.compose_labelled(lg, lg, name) as by_name, W.compose_labelled(lg, lg, LC.NAMES[name]) as by_number:
        want = LC.from_rows([[(2, REFERENCE_LABELS[LC.NAMES[name]])], [], [], []])
        assert same(by_name.csr(), want, name) and same(by_number.csr(), want, name)
    check(W, g, g, LC.NAMES[name])


@pytest.mark.parametrize("kind, width", [(GAMMA, 0), (FIXED, 5)])
def test_the_references_case_from_label_streams_on_disk(W, tools, tmp_path, kind, width):
    g = LC.from_rows(REFERENCE_ROWS)
    base = str(tmp_path / "ref")
    tools.store((g[0], g[1])).write(base + "-underlying")
    tools.store_labels(kind, width, g[2].astype(np.int32), g[0].astype(np.uint64)).write(base, "ref-underlying")
    bs = W.BitStreamArcLabelledImmutableGraph.load(base)
    try:
        with W.compose_labelled(bs, bs, "MIN_PLUS") as r:                      # a BitStreamArcLabelledImmutableGraph source, converted once
            assert (r.kind, r.width) == (kind, width)
            assert same(r.csr(), LC.from_rows([[(2, 2)], [], [], []]))
    finally:
        bs.close(); bs.g.close()
    out = str(tmp_path / "out")
    assert W.labelled_compose_main([base, base, out, "PLUS_TIMES"] + (["--width", "7"] if kind == FIXED else [])) == 0
    back = W.BitStreamArcLabelledImmutableGraph.load(out)
    try:
        with W.LabelledGraph.from_graph(back) as lb:
            assert (lb.kind, lb.width) == (kind, 7 if kind == FIXED else 0)
            assert same(lb.csr(), LC.from_rows([[(2, 9)], [], [], []]))
    finally:
        back.close(); back.g.close()


# ---- unequal node counts: the guard y < n1

@pytest.mark.parametrize("n0, n1", [(50, 1), (50, 7), (7, 50), (300, 64), (64, 300), (3, 0), (0, 3)])
def test_unequal_node_counts(W, n0, n1):
    rng = np.random.default_rng(n0 * 1000 + n1)
    a = LC.from_rows([[(int(y), int(rng.integers(0, 100))) for y in np.flatnonzero(rng.random(n0) < 0.3)] for _ in range(n0)])
    b = LC.from_rows([[(int(z), int(rng.integers(0, 100))) for z in np.flatnonzero(rng.random(n1) < 0.5)] for _ in range(n1)])
    if n0 > n1:
        assert len(a[1]) and int(a[1].max()) >= n1                             # successors g1 does not have
    for s in (LC.MIN_PLUS, LC.PLUS_TIMES):
        check(W, a, b, s)


# ---- rows at the tiers' limits

@pytest.mark.parametrize("semiring", LC.SEMIRINGS)
@pytest.mark.parametrize("shape", ["one_list", "uneven_lists", "same_key", "stride"])
def test_rows_at_the_tier_limits(W, shape, semiring):
    lim = limits(W)
    rng = np.random.default_rng(3)
    ubs = boundary_bounds(lim)
    a, b = labelled_products([shape_rows(shape, ub, rng) for ub in ubs])
    assert CM.bounds(LC.underlying(a), LC.underlying(b))[:len(ubs)].tolist() == ubs   # the rows have exactly these bounds
    if shape == "same_key":                                                    # ub products onto the one key, their labels all different
        lists = [b[2][b[0][y]:b[0][y + 1]].tolist() for y in a[1][a[0][5]:a[0][6]]]
        assert len(lists) == ubs[5] and len(set(map(tuple, lists))) == ubs[5]
    rep = check(W, a, b, semiring, what=shape)
    assert rep["rows"] == expected_rows(ubs, lim) == [2, 3, 1]
    assert rep["products"] == sum(ubs) and rep["batches"] == 1


# ---- forced tiers, batches

@pytest.mark.parametrize("tier", [0, 1, 2])
def test_forced_tiers_give_the_same_graph(W, monkeypatch, tier):
    lim = limits(W)
    a, b = labelled_products(boundary_rows(lim))
    ub = CM.bounds(LC.underlying(a), LC.underlying(b))
    monkeypatch.setenv("BVG_COMPOSE_TIER", str(tier))
    rep = check(W, a, b, LC.MIN_PLUS, what="boundary rows, tier %d" % tier)
    assert rep["rows"] == expected_rows(ub.tolist(), lim, tier)
    rng = np.random.default_rng(3)
    ubs = boundary_bounds(lim)
    a, b = labelled_products([shape_rows("same_key", u, rng) for u in ubs])
    for s in LC.SEMIRINGS:                                                     # every lane of the owner on one value slot, in this tier's memory
        rep = check(W, a, b, s, what="same key, tier %d, semiring %d" % (tier, s))
        assert rep["rows"] == expected_rows(ubs, lim, tier)


def test_tier2_in_batches_of_one_row(W, monkeypatch):
    rng = np.random.default_rng(9)
    rows = [[np.sort(rng.choice(5000, size=100, replace=False)).astype(np.int64)] for _ in range(10)] + [[]]   # ten rows of bound 100, one of 0
    a, b = labelled_products(rows)
    monkeypatch.setenv("BVG_COMPOSE_TIER", "2")
    monkeypatch.setenv("BVG_COMPOSE_WS", str(2 * 128 * 16))                    # one row's table: 2 pow2ceil(100) slots of 16 bytes
    for s in (LC.MIN_PLUS, LC.MAX_PLUS):                                       # values cleared to all-ones, and to zero
        rep = check(W, a, b, s)
        assert rep["rows"] == [0, 0, 10] and rep["batches"] == 10
    monkeypatch.setenv("BVG_COMPOSE_WS", "1")                                  # below any table: every row a batch and a workspace of its own
    assert check(W, a, b, LC.PLUS_TIMES)["batches"] == 10
    monkeypatch.delenv("BVG_COMPOSE_WS")
    assert check(W, a, b, LC.MIN_PLUS)["batches"] == 1


# ---- a real structure

@pytest.fixture(scope="module")
def prefix_labelled(cnr_csr):
    deg, succ = cnr_csr
    off, adj = CM.prefix(np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ, PREFIX)
    src = np.repeat(np.arange(PREFIX, dtype=np.int64), np.diff(off))
    return LC.make(off, adj, (src * 31 + adj) % 97)


def test_cnr_prefix(W, prefix_labelled):
    g = prefix_labelled
    assert len(g[1]) > 10000
    for s in (LC.MIN_PLUS, LC.PLUS_TIMES):
        rep = check(W, g, g, s, what="cnr prefix, semiring %d" % s)
        assert rep["products"] == int(CM.bounds(LC.underlying(g), LC.underlying(g)).sum())
    with lgraph(W, g) as lg, W.compose_labelled(lg, lg, "MAX_MIN") as sq, sq.underlying() as u, lg.underlying() as ul, W.compose(ul, ul) as want:
        off, adj = u.csr()
        woff, wadj = want.csr()
        assert np.array_equal(off, woff) and np.array_equal(adj, wadj)         # underlying(a o b) = underlying(a) o underlying(b), on the device


# ---- range

def path(l0, l1):
    """0 -> 1 labelled l0, 1 -> 2 labelled l1: composed with itself, the one arc (0, 2)."""
    return LC.from_rows([[(1, l0)], [(2, l1)], []])


def test_range_of_a_fixed_width_result(W):
    rep = check(W, path(255, 0), path(255, 0), LC.MIN_PLUS, FIXED, 8)          # 255 + 0 fits 8 bits
    assert rep["arcs"] == 1
    with lgraph(W, path(255, 1), FIXED, 8) as g:
        with pytest.raises(W.IllegalArgumentException) as e:
            W.compose_labelled(g, g, "MIN_PLUS")
        assert e.value.out_of_range == 1 and e.value.first_arc == (0, 2) and e.value.report["arcs"] == 1
        with W.compose_labelled(g, g, "MIN_PLUS", out_width=9) as r:           # ... and 256 fits 9
            assert (r.kind, r.width) == (FIXED, 9) and r.csr()[2].tolist() == [256]
    check(W, path(255, 1), path(255, 1), LC.MIN_PLUS, FIXED, 8)                 # the model's refusal is the device's
    check(W, path(255, 1), path(255, 1), LC.MIN_PLUS, FIXED, 8, out_width=9)
    check(W, path(3, 3), path(3, 3), LC.MAX_MIN, FIXED, 2, out_width=0)         # width 0 holds the label 0 alone: refused
    check(W, path(0, 3), path(0, 3), LC.MAX_MIN, FIXED, 2, out_width=0)


def test_range_of_a_gamma_result(W):
    top = (1 << 31) - 1
    with lgraph(W, path(top, top)) as g:
        with pytest.raises(W.IllegalArgumentException) as e:
            W.compose_labelled(g, g, "MIN_PLUS")
        assert e.value.out_of_range == 1 and e.value.first_arc == (0, 2)
        with pytest.raises(W.IllegalArgumentException):                        # a GammaCodedIntLabel has no width to choose
            W.compose_labelled(g, g, "MIN_MAX", out_width=31)
    check(W, path(top, top), path(top, top), LC.MIN_MAX)                        # max(top, top) is in range
    check(W, path(top, 0), path(top, 0), LC.MAX_PLUS)
    check(W, path(top, 1), path(top, 1), LC.MAX_PLUS)


def test_the_report_names_the_smallest_refused_arc(W):
    g = LC.from_rows([[(2, 1)], [(2, 200)], [(3, 100)], [(0, 200)]])
    # 1 -> 2 -> 3 and 2 -> 3 -> 0 reach 300, 0 -> 2 -> 3 and 3 -> 0 -> 2 stay below 256
    assert LC.compose(g, g, LC.MAX_PLUS, FIXED, 8) == ("range", 2, (1, 3))
    check(W, g, g, LC.MAX_PLUS, FIXED, 8)


def test_plus_times_is_clamped_not_wrapped(W):
    """16 paths of 2^30 * 2^30 onto one key: an unclamped 64-bit sum is 2^64 = 0, a valid label."""
    big = 1 << 30
    g = LC.from_rows([[(y, big) for y in range(1, 17)]] + [[(17, big)]] * 16 + [[]])
    assert LC.compose_rows(g, g, LC.PLUS_TIMES)[0] == [(17, 1 << 64)]
    assert LC.compose(g, g, LC.PLUS_TIMES) == ("range", 1, (0, 17))
    check(W, g, g, LC.PLUS_TIMES)
    small = LC.from_rows([[(y, 1 << 13) for y in range(1, 17)]] + [[(17, 1 << 13)]] * 16 + [[]])   # 16 * 2^26 = 2^30: exact
    assert check(W, small, small, LC.PLUS_TIMES)["arcs"] == 1


# ---- determinism, chaining, files

def test_deterministic_chains_and_files(W, tmp_path):
    g = LM.random_graph(np.random.default_rng(12), 400, 0.04, heavy=True, lab_max=(1 << 10) - 1)
    g = LC.make(*g)
    status, want = LC.compose(g, g, LC.MIN_PLUS, FIXED, 11)
    assert status == "ok"
    with lgraph(W, g, FIXED, 10) as lg:
        with W.compose_labelled(lg, lg, "MIN_PLUS", out_width=11) as r1, W.compose_labelled(lg, lg, "MIN_PLUS", out_width=11) as r2:
            c1, c2 = r1.csr(), r2.csr()
            assert all(np.array_equal(p, q) for p, q in zip(c1, c2)) and same(c1, want)
            with W.transpose_labelled(r1) as t:                                # the result is a source like any other
                assert (t.kind, t.width) == (FIXED, 11)
                assert LM.equal(LM.make(*t.csr()), LM.transpose(LM.make(*want)))
            base = str(tmp_path / "sq")
            r1.write(base)
        bs = W.BitStreamArcLabelledImmutableGraph.load(base)
        try:
            with W.LabelledGraph.from_graph(bs) as back:
                assert (back.kind, back.width) == (FIXED, 11) and same(back.csr(), want)
        finally:
            bs.close(); bs.g.close()


# ---- refusals

def test_differing_label_classes_are_refused(W):
    g = path(1, 1)
    with lgraph(W, g, GAMMA) as a, lgraph(W, g, FIXED, 4) as b, lgraph(W, g, FIXED, 5) as c:
        for p, q in [(a, b), (b, a), (b, c)]:
            with pytest.raises(W.IllegalArgumentException):
                W.compose_labelled(p, q, "MIN_PLUS")
        W.compose_labelled(b, b, "MIN_PLUS").close()
        b.close()
        with pytest.raises(W.IllegalArgumentException):
            W.compose_labelled(b, c, "MIN_PLUS")                               # a closed source


def test_result_above_the_limit_is_refused_with_its_size(W, monkeypatch, prefix_labelled):
    g = prefix_labelled
    want = CM.compose(LC.underlying(g), LC.underlying(g))
    arcs, products = len(want[1]), int(CM.bounds(LC.underlying(g), LC.underlying(g)).sum())
    with lgraph(W, g) as lg:
        monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", "1000")
        with pytest.raises(W.UnsupportedOperationException) as e:
            W.compose_labelled(lg, lg, "MIN_PLUS")
        assert e.value.report["arcs"] == arcs and e.value.report["products"] == products and sum(e.value.report["rows"]) > 0
        monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", str(arcs))                   # the limit itself passes
        W.compose_labelled(lg, lg, "MIN_PLUS").close()
        monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", str(arcs - 1))
        with pytest.raises(W.UnsupportedOperationException):
            W.compose_labelled(lg, lg, "MIN_PLUS")
