"""GPU: the graph product on the device (bvg_compose), list for list against the model (tests/compose_model.py) unless said otherwise:
the smallest graphs, unequal node counts (the guard that keeps a successor a smaller g1 does not have from being used as an index), rows
built to sit exactly at, one below and one above each tier's limit, every tier forced, tier 2 in batches of one row, cnr-2000, the
algebraic identities with the existing transforms as yardsticks, and the refusals."""
import numpy as np
import pytest

import compose_model as CM
import transform_model as M
from conftest import CNR

pytestmark = pytest.mark.gpu

N_CNR = 325557
PREFIX = 20000


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
def prefix_model(cnr_model):
    return CM.prefix(*cnr_model, PREFIX)


@pytest.fixture(scope="module")
def prefix(W, prefix_model):
    g = W.ParsedGraph.from_csr(*prefix_model)
    yield g
    g.close()


@pytest.fixture(scope="module")
def prefix_square(prefix_model):
    return CM.cached("prefix_square", lambda: CM.compose(prefix_model, prefix_model))


def graph_of(W, lists):
    return W.ParsedGraph.from_csr(*M.csr(lists))


def same(got, want, what=""):
    off, adj = got
    assert len(off) == len(want[0]), what + ": node counts differ"
    assert np.array_equal(np.asarray(off).astype(np.int64), np.asarray(want[0]).astype(np.int64)), what + ": offsets differ"
    assert np.array_equal(adj, want[1]), what + ": successors differ"
    return True


def holds(g, want, what=""):
    """The resident graph holds the model's lists (and closes)."""
    with g:
        off, adj = g.csr()
        assert g.num_nodes() == len(want[0]) - 1 and g.num_arcs() == len(adj) == int(off[-1])
        return same((off, adj), want, what)


def limits(W):
    with graph_of(W, [[0]]) as g:
        r, rep = W.compose(g, g, report=True)
        r.close()
    assert rep["limit"][0] >= 1 and rep["limit"][1] > rep["limit"][0]
    return rep["limit"]


def padded_csr(lists, n):
    """The CSR of `lists` as a graph of n >= len(lists) nodes: the tail nodes have no successors."""
    off = np.zeros(n + 1, dtype=np.int64)
    lens = np.array([len(l) for l in lists], dtype=np.int64)
    off[1:len(lists) + 1] = np.cumsum(lens)
    off[len(lists) + 1:] = off[len(lists)]
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if int(off[-1]) else np.empty(0, np.int64)
    return off, adj


def product_graphs(rows):
    """rows[r] = the lists of g1 that row r of g0 unites.  -> (g0, g1) as CSRs: g0 has len(rows) nodes, node r pointing at the nodes of
    g1 that hold its lists; g1 has as many nodes as its lists and their targets need."""
    g0, g1 = [], []
    for lists in rows:
        g0.append(np.arange(len(g1), len(g1) + len(lists), dtype=np.int64))
        g1.extend(lists)
    top = max([int(l[-1]) + 1 for l in g1 if len(l)] + [len(g1), 1])
    return padded_csr(g0, max(len(g0), len(g1))), padded_csr(g1, top)          # (a graph's successors are nodes of its own)


def shape_rows(shape, ub, rng, s=6):
    """The lists of one row whose bound is exactly ub."""
    if shape == "one_list":
        return [np.arange(2, ub + 2, dtype=np.int64)]
    if shape == "uneven_lists":                                                # 65 disjoint lists, some empty, ub keys together
        cuts = np.sort(rng.integers(0, ub + 1, size=64))
        cuts[10], cuts[31], cuts[32] = cuts[11], cuts[30], cuts[30]            # repeated cuts: empty lists
        edges = np.concatenate([[0], np.sort(cuts), [ub]])
        return [np.arange(edges[i], edges[i + 1], dtype=np.int64) * 3 + 1 for i in range(65)]
    if shape == "same_key":                                                    # ub lists of the same single successor
        return [np.array([5], dtype=np.int64)] * ub
    assert shape == "stride"
    return [np.arange(ub, dtype=np.int64) << s]


def boundary_bounds(lim):
    return [lim[0] - 1, lim[0], lim[0] + 1, lim[1] - 1, lim[1], lim[1] + 1]


def expected_rows(ubs, lim, forced=None):
    rows = [0, 0, 0]
    for u in ubs:
        if u:
            t = 0 if u <= lim[0] else 1 if u <= lim[1] else 2
            rows[max(t, forced) if forced is not None else t] += 1
    return rows


def boundary_rows(lim, shapes=("one_list", "uneven_lists", "same_key", "stride")):
    rng = np.random.default_rng(5)
    rows = []
    for shape in shapes:
        for ub in boundary_bounds(lim):
            rows.append(shape_rows(shape, ub, rng))
    rows.append([])                                                            # a row without successors among them
    return rows


# ---- the smallest graphs

@pytest.mark.parametrize("la, lb", [
    ([], []),                                                                  # 0 nodes
    ([[]], [[]]),                                                              # 1 node without arcs
    ([[0]], [[0]]),                                                            # ... with a loop
    ([[0]], [[]]), ([[]], [[0]]),
    ([[1], [2], []], [[1], [2], []]),                                          # the path 0 -> 1 -> 2
    ([[], [], []], [[1, 2], [0], [2]]),                                        # only empty lists on the left
    ([[1, 2], [0], [2]], [[], [], []]),                                        # ... on the right
    ([[0, 1, 2]] * 3, [[0, 1, 2]] * 3),
])
def test_smallest_graphs(W, la, lb):
    with graph_of(W, la) as a, graph_of(W, lb) as b:
        g, rep = W.compose(a, b, report=True)
        assert holds(g, M.csr(CM.compose_sets(la, lb)))
        assert rep["products"] == int(CM.bounds(M.csr(la), M.csr(lb)).sum()) and rep["arcs"] == sum(len(l) for l in CM.compose_sets(la, lb))


# ---- unequal node counts: the guard y < n1

@pytest.mark.parametrize("n0, n1", [(50, 1), (50, 7), (7, 50), (1, 50), (300, 64), (64, 300), (3, 0), (0, 3)])
def test_unequal_node_counts(W, n0, n1):
    rng = np.random.default_rng(n0 * 1000 + n1)
    la = [np.flatnonzero(rng.random(n0) < 0.3) for _ in range(n0)]             # successors over all of [0, n0): most of them >= n1 when n1 is small
    lb = [np.flatnonzero(rng.random(n1) < 0.5) for _ in range(n1)]
    if n0 > n1:
        assert any(len(l) and l[-1] >= n1 for l in la)
    with graph_of(W, la) as a, graph_of(W, lb) as b:
        assert holds(W.compose(a, b), M.csr(CM.compose_sets(la, lb)))


# ---- rows at the tiers' limits

@pytest.mark.parametrize("shape", ["one_list", "uneven_lists", "same_key", "stride", "stride_max"])
def test_rows_at_the_tier_limits(W, shape):
    lim = limits(W)
    rng = np.random.default_rng(3)
    rows, ubs = [], boundary_bounds(lim)
    for ub in ubs:
        if shape == "stride_max":                                              # the largest stride that keeps the graph under 2^22 nodes
            s = max(s for s in range(6, 22) if ((ub - 1) << s) + 1 < (1 << 22))
            rows.append(shape_rows("stride", ub, rng, s))
        else:
            rows.append(shape_rows(shape, ub, rng))
    g0, g1 = product_graphs(rows)
    assert CM.bounds(g0, g1)[:len(ubs)].tolist() == ubs                         # the rows have exactly these bounds
    want = CM.compose(g0, g1)
    with W.ParsedGraph.from_csr(*g0) as a, W.ParsedGraph.from_csr(*g1) as b:
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want, shape)
    assert rep["rows"] == expected_rows(ubs, lim) == [2, 3, 1]
    assert rep["products"] == sum(ubs) and rep["arcs"] == len(want[1])
    assert rep["batches"] == 1


def test_every_shape_mixed_in_one_call(W):
    lim = limits(W)
    rows = boundary_rows(lim)
    g0, g1 = product_graphs(rows)
    ub = CM.bounds(g0, g1)
    want = CM.compose(g0, g1)
    with W.ParsedGraph.from_csr(*g0) as a, W.ParsedGraph.from_csr(*g1) as b:
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want)
    assert rep["rows"] == expected_rows(ub.tolist(), lim) and rep["products"] == int(ub.sum()) and rep["arcs"] == len(want[1])


# ---- forced tiers, batches

@pytest.mark.parametrize("tier", [0, 1, 2])
def test_forced_tiers_give_the_same_graph(W, monkeypatch, prefix, prefix_model, prefix_square, tier):
    lim = limits(W)
    g0, g1 = product_graphs(boundary_rows(lim))
    ub = CM.bounds(g0, g1)
    want = CM.compose(g0, g1)
    monkeypatch.setenv("BVG_COMPOSE_TIER", str(tier))
    with W.ParsedGraph.from_csr(*g0) as a, W.ParsedGraph.from_csr(*g1) as b:
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want, "boundary rows, tier %d" % tier)
    assert rep["rows"] == expected_rows(ub.tolist(), lim, tier)
    g, rep = W.compose(prefix, prefix, report=True)
    assert holds(g, prefix_square, "cnr prefix, tier %d" % tier)
    pub = CM.bounds(prefix_model, prefix_model)
    assert rep["rows"] == expected_rows(pub.tolist(), lim, tier) and sum(rep["rows"]) == int(np.sum(pub > 0))
    if tier == 2:
        assert rep["rows"][2] == int(np.sum(pub > 0)) and rep["rows"][:2] == [0, 0]


def test_tier2_in_batches_of_one_row(W, monkeypatch):
    rng = np.random.default_rng(9)
    rows = [[np.sort(rng.choice(5000, size=100, replace=False)).astype(np.int64)] for _ in range(10)] + [[]]   # ten rows of bound 100, one of 0
    g0, g1 = product_graphs(rows)
    want = CM.compose(g0, g1)
    monkeypatch.setenv("BVG_COMPOSE_TIER", "2")
    monkeypatch.setenv("BVG_COMPOSE_WS", str(2 * 128 * 8))                     # one row's table: 2 pow2ceil(100) slots of 8 bytes
    with W.ParsedGraph.from_csr(*g0) as a, W.ParsedGraph.from_csr(*g1) as b:
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want)
        assert rep["rows"] == [0, 0, 10] and rep["batches"] == 10
        monkeypatch.setenv("BVG_COMPOSE_WS", "1")                              # below any table: every row a batch and a workspace of its own
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want) and rep["batches"] == 10
        monkeypatch.delenv("BVG_COMPOSE_WS")
        g, rep = W.compose(a, b, report=True)
        assert holds(g, want) and rep["batches"] == 1


# ---- cnr-2000

def test_cnr_prefix(W, prefix, prefix_model, prefix_square):
    g, rep = W.compose(prefix, prefix, report=True)
    assert holds(g, prefix_square)
    assert rep["products"] == 1563905 and rep["arcs"] == 923888
    assert int(np.diff(prefix_square[0]).max()) == 1192 and int(CM.bounds(prefix_model, prefix_model).max()) == 4617


def test_cnr_squared(W, cnr, cnr_model):
    want = CM.cached("cnr_square", lambda: CM.compose(cnr_model, cnr_model))
    g, rep = W.compose(cnr, cnr, report=True)                                  # a BVGraph source, and the same handle twice
    with g:
        off, adj = g.csr()
        assert g.num_nodes() == N_CNR and g.num_arcs() == 34174066
    assert same((off, adj), want, "cnr o cnr")
    deg = np.diff(off.astype(np.int64))
    assert rep["products"] == 96065788 and rep["arcs"] == 34174066 and int(np.sum(deg > 0)) == 241644 and int(deg.max()) == 15723
    assert sum(rep["rows"]) == int(np.sum(CM.bounds(cnr_model, cnr_model) > 0))
    with W.ParsedGraph.from_csr(*cnr_model) as parsed:                         # a ParsedGraph source, and one of each
        g2 = W.compose(parsed, cnr)
        with g2:
            off2, adj2 = g2.csr()
        assert np.array_equal(off2, off) and np.array_equal(adj2, adj)


# ---- identities, with no model

def test_identity_graph_is_neutral(W, prefix, prefix_model):
    loops = (np.arange(PREFIX + 1, dtype=np.int64), np.arange(PREFIX, dtype=np.int64))
    with W.ParsedGraph.from_csr(*loops) as ident:
        assert holds(W.compose(prefix, ident), prefix_model, "g o I")
        assert holds(W.compose(ident, prefix), prefix_model, "I o g")


def test_associative_and_transpose_reverses(W, prefix):
    with W.filter_arcs(prefix, "NO_LOOPS") as b, W.compose(prefix, b) as ab, W.compose(b, prefix) as bc:
        with W.compose(ab, prefix) as left, W.compose(prefix, bc) as right:
            assert same(left.csr(), right.csr(), "(a o b) o c = a o (b o c)")
        with W.transpose_graph(ab) as t_ab, W.transpose_graph(prefix) as ta, W.transpose_graph(b) as tb, W.compose(tb, ta) as rev:
            assert same(t_ab.csr(), rev.csr(), "transpose(a o b) = transpose(b) o transpose(a)")


def test_result_can_be_stored(W, prefix, prefix_square):
    with W.compose(prefix, prefix) as sq:
        graph, offsets = sq.store()
    g = W.BVGraph.from_memory(W.default_params(nodes=PREFIX, arcs=len(prefix_square[1])), graph, offsets)
    try:
        deg, succ = g.decode_range(0, PREFIX)
    finally:
        g.close()
    assert np.array_equal(deg, np.diff(prefix_square[0])) and np.array_equal(succ, prefix_square[1])


# ---- refusals

def test_result_above_the_limit_is_refused_with_its_size(W, monkeypatch, prefix):
    monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", "1000")
    with pytest.raises(W.UnsupportedOperationException) as e:
        W.compose(prefix, prefix)
    assert e.value.report["arcs"] == 923888 and e.value.report["products"] == 1563905
    monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", "923888")                       # the limit itself passes
    W.compose(prefix, prefix).close()
    monkeypatch.setenv("BVG_COMPOSE_MAX_ARCS", "923887")
    with pytest.raises(W.UnsupportedOperationException):
        W.compose(prefix, prefix)


def test_closed_and_shard_handles_are_refused(W, cnr, prefix):
    g = graph_of(W, [[0]])
    g.close()
    with pytest.raises(W.IllegalArgumentException):
        W.compose(g, prefix)
    with pytest.raises(W.IllegalArgumentException):
        W.compose(prefix, g)
    shard = cnr.copy()
    try:
        shard.set_node_base(5)                                                 # a shard's handle: its targets leave its node range
        with pytest.raises(W.IllegalArgumentException):
            W.compose(shard, prefix)
        with pytest.raises(W.IllegalArgumentException):
            W.compose(prefix, shard)
    finally:
        shard.close()
