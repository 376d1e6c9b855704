"""CPU: the numpy model of the graph product (tests/compose_model.py) against Python sets on small random graphs of unequal node counts,
and the figures of cnr-2000 that the device tests and DESIGN.md 7k quote."""
import numpy as np

import compose_model as CM
import transform_model as M


def random_lists(rng, n, targets, dens):
    return [np.flatnonzero(rng.random(targets) < dens) for _ in range(n)]


def test_model_against_sets_on_unequal_node_counts():
    rng = np.random.default_rng(11)
    for trial in range(120):
        n0, n1 = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        dens = [0.0, 0.05, 0.3, 0.7][trial % 4]
        # g0's successors range over max(n0, n1) nodes when it is the larger graph: arcs into [n1, n0) must contribute nothing
        la, lb = random_lists(rng, n0, n0, dens), random_lists(rng, n1, n1, dens)
        want = CM.compose_sets(la, lb)
        off, adj = CM.compose(M.csr(la), M.csr(lb), chunk=7)
        assert [l.tolist() for l in M.lists_of(off, adj)] == want, (trial, n0, n1)
        ub = CM.bounds(M.csr(la), M.csr(lb))
        assert ub.tolist() == [sum(len(lb[y]) for y in la[x] if y < n1) if x < n0 else 0 for x in range(max(n0, n1))], (trial, n0, n1)


def cnr_model(cnr_csr):
    deg, succ = cnr_csr
    return np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ


def test_cnr_figures(cnr_csr):
    g = cnr_model(cnr_csr)
    assert len(g[1]) == 3216152
    ub = CM.bounds(g, g)
    assert int(ub.sum()) == 96065788
    assert [int(np.sum(ub > t)) for t in (64, 1024, 8192)] == [139701, 28413, 31]
    off, adj = CM.cached("cnr_square", lambda: CM.compose(g, g))
    deg = np.diff(off)
    assert len(adj) == int(off[-1]) == 34174066
    assert int(np.sum(deg > 0)) == 241644
    assert int(deg.max()) == 15723 and int(ub[int(deg.argmax())]) == 18480       # the longest row (node 31980) and its products
    assert int(ub.max()) == 34537 and int(deg[int(ub.argmax())]) == 2554         # the largest bound belongs to another row (node 181662)
    assert np.all(deg <= ub)
    t = M.transpose(*g)
    assert int(CM.bounds(t, g).sum()) == 169085946                              # cnr^T o cnr: g0 = the transpose
    assert int(CM.bounds(g, t).sum()) == 15574082986                            # cnr o cnr^T


def test_cnr_prefix_figures(cnr_csr):
    p = CM.prefix(*cnr_model(cnr_csr), 20000)
    assert len(p[0]) == 20001 and len(p[1]) == 134937
    ub = CM.bounds(p, p)
    assert int(ub.sum()) == 1563905 and int(ub.max()) == 4617
    off, adj = CM.cached("prefix_square", lambda: CM.compose(p, p))
    assert len(adj) == 923888 and int(np.diff(off).max()) == 1192
    for x in (0, 1, 777, 19999):                                                # lists sorted, without repeats
        l = adj[off[x]:off[x + 1]]
        assert np.all(np.diff(l) > 0)
