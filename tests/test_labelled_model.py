"""CPU: the model of the labelled transforms (tests/labelled_model.py) against a brute-force restatement over {(x, y): label} dictionaries, on
every pair of a fixed set of small labelled graphs over at most 4 nodes."""
import itertools

import numpy as np
import pytest

import labelled_model as LM

PICK = {LM.KEEP_FIRST: lambda a, b: a, LM.MIN: min, LM.MAX: max}


def _graphs():
    rng = np.random.default_rng(20260)
    out = [(0, {}), (1, {}), (1, {(0, 0): 3}), (4, {}), (4, {(x, y): (x * 4 + y) % 5 for x in range(4) for y in range(4)})]
    for _ in range(11):
        n = int(rng.integers(1, 5))
        out.append((n, {(x, y): int(rng.integers(0, 6)) for x in range(n) for y in range(n) if rng.random() < 0.45}))
    return out


GRAPHS = _graphs()


def brute_union(a, b, strategy):
    (na, da), (nb, db) = a, b
    d = {}
    for k in set(da) | set(db):
        d[k] = PICK[strategy](da[k], db[k]) if k in da and k in db else da.get(k, db.get(k))
    return max(na, nb), d


def brute_transpose(g):
    return g[0], {(y, x): l for (x, y), l in g[1].items()}


def same(model_graph, brute):
    n, d = brute
    return LM.nodes(model_graph) == n and LM.to_dict(model_graph) == d and LM.equal(model_graph, LM.from_dict(n, d))


def test_csr_round_trip_and_order():
    for n, d in GRAPHS:
        g = LM.from_dict(n, d)
        assert LM.to_dict(g) == d and len(g[0]) == n + 1 and int(g[0][-1]) == len(d)
        for x in range(n):
            row = g[1][int(g[0][x]):int(g[0][x + 1])]
            assert np.all(np.diff(row) > 0)                                     # lists sorted by successor, no duplicates
        assert LM.equal(LM.from_csr(*LM.csr(g)), g)


def test_transpose_against_brute_force():
    for n, d in GRAPHS:
        g = LM.from_dict(n, d)
        assert same(LM.transpose(g), brute_transpose((n, d)))
        assert LM.equal(LM.transpose(LM.transpose(g)), g)


@pytest.mark.parametrize("strategy", [LM.KEEP_FIRST, LM.MIN, LM.MAX])
def test_union_against_brute_force_on_every_pair(strategy):
    for a, b in itertools.product(GRAPHS, repeat=2):
        u = LM.union(LM.from_dict(*a), LM.from_dict(*b), strategy)
        assert same(u, brute_union(a, b, strategy)), (a, b)
        common = len(set(a[1]) & set(b[1]))
        assert int(u[0][-1]) == len(a[1]) + len(b[1]) - common


def test_keep_first_is_not_symmetric_min_and_max_are():
    differs = 0
    for a, b in itertools.product(GRAPHS, repeat=2):
        ga, gb = LM.from_dict(*a), LM.from_dict(*b)
        for s in (LM.MIN, LM.MAX):
            assert LM.equal(LM.union(ga, gb, s), LM.union(gb, ga, s))
        ab, ba = LM.to_dict(LM.union(ga, gb)), LM.to_dict(LM.union(gb, ga))
        assert set(ab) == set(ba)
        diff = {k for k in ab if ab[k] != ba[k]}
        assert diff == {k for k in set(a[1]) & set(b[1]) if a[1][k] != b[1][k]}   # exactly the common arcs whose labels differ
        differs += bool(diff)
    assert differs > 0


@pytest.mark.parametrize("strategy", [LM.KEEP_FIRST, LM.MIN, LM.MAX])
def test_symmetrize_is_union_with_transpose(strategy):
    for n, d in GRAPHS:
        g = LM.from_dict(n, d)
        s = LM.symmetrize(g, strategy)
        assert same(s, brute_union((n, d), brute_transpose((n, d)), strategy))
        sd = LM.to_dict(s)
        assert all((y, x) in sd for (x, y) in sd)
        if strategy == LM.KEEP_FIRST:
            assert all(sd[k] == l for k, l in d.items())                        # g's label wherever g has the arc
        else:
            assert all(sd[(x, y)] == sd[(y, x)] for (x, y) in sd)               # label-symmetric


def test_filters_against_brute_force():
    rng = np.random.default_rng(7)
    for n, d in GRAPHS:
        g = LM.from_dict(n, d)
        assert same(LM.filter(g, LM.NO_LOOPS), (n, {k: l for k, l in d.items() if k[0] != k[1]}))
        cls = rng.integers(0, 2, n)
        assert same(LM.filter(g, LM.SAME_CLASS, node_class=cls), (n, {k: l for k, l in d.items() if cls[k[0]] == cls[k[1]]}))
        assert same(LM.filter(g, LM.DIFFERENT_CLASS, node_class=cls), (n, {k: l for k, l in d.items() if cls[k[0]] != cls[k[1]]}))
        for bound in (-1, 0, 2, 3, 6):
            assert same(LM.filter(g, LM.LOWER_BOUND, lower_bound=bound), (n, {k: l for k, l in d.items() if l >= bound}))   # >=: a label equal to the bound stays
    assert LM.to_dict(LM.filter(LM.from_dict(2, {(0, 1): 3, (1, 0): 2}), LM.LOWER_BOUND, lower_bound=3)) == {(0, 1): 3}
