"""CPU: the numpy model of HyperBall (tests/hyperball_model.py) against exact all-pairs breadth-first search, with the criterion of the
reference's own test (HyperBallTest.java:94-126): a term of the neighbourhood function is right when it is within 2 rsd of the exact
value, and it has to be right for at least 9 of 10 seeds."""
import numpy as np
import pytest

import hyperball_model as M

GRAPHS = {
    "clique": lambda: M.clique(100),
    "cycle": lambda: M.cycle(120),
    "line": lambda: M.line(150),
    "out_tree": lambda: M.out_tree(255),
    "random": lambda: M.random_graph(300, 3.0, 2026),
}


def test_hash_and_count_basics():
    for log2m in (4, 8, 12):
        seen = set()
        for v in range(2000):
            j, r = M.hash_node(v, 0, log2m)
            assert 0 <= j < (1 << log2m) and 1 <= r <= 65 - log2m
            seen.add(j)
        assert len(seen) > min(1 << log2m, 2000) // 2
    assert M.hash_node(5, 0, 6) != M.hash_node(5, 1, 6)
    # an empty counter counts 0 (m ln(m / m)); a counter with one register set counts about 1
    for log2m in (4, 6, 8):
        z = np.zeros((1, 1 << log2m), dtype=np.uint8)
        assert M.count(z, log2m)[0] == 0
        z[0, 3] = 1
        assert abs(M.count(z, log2m)[0] - 1) < 0.05


def test_iteration_semantics_on_a_line():
    lists = M.line(6)
    off, succ = M.adjacency(lists)
    hb = M.HyperBallModel(off, succ, 6, seed=3, sum_of_distances=True, harmonic=True)
    hb.init()
    assert hb.nf == [6.0] and hb.iteration == -1 and hb.modified == 6
    r0 = hb.regs.copy()
    hb.iterate()
    assert np.array_equal(hb.regs[5], r0[5]) and np.array_equal(hb.regs[0], np.maximum(r0[0], r0[1]))
    assert hb.modified == 5 and hb.iteration == 0
    hb.run()
    assert hb.modified == 0 and hb.iteration == 5                              # the fifth iteration changes node 0 only, the sixth nothing
    assert np.all(np.diff(hb.nf) >= 0)
    assert hb.sod[5] == 0 and hb.sid[5] == 0 and hb.sod[0] > hb.sod[4] > 0
    assert hb.closeness()[5] == 0 and hb.lin()[5] == 1


@pytest.mark.parametrize("log2m", [4, 5, 6, 8])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_neighbourhood_function_against_exact_bfs(name, log2m):
    lists = GRAPHS[name]()
    exact = M.exact_neighbourhood_function(lists)
    off, succ = M.adjacency(lists)
    rsd = M.relative_standard_deviation(log2m)
    right = np.zeros(len(exact), dtype=int)
    report = []
    for seed in range(10):
        hb = M.HyperBallModel(off, succ, log2m, seed=seed)
        hb.run()
        nf = np.asarray(hb.nf)
        nf = np.concatenate([nf, np.full(max(0, len(exact) - len(nf)), nf[-1])])[:len(exact)]   # (stable: the function stays at its last term)
        ok = np.abs(nf - exact) <= 2 * rsd * exact
        right += ok
        report.append((seed, int(ok.sum()), float(np.max(np.abs(nf - exact) / exact))))
    print(name, log2m, "terms", len(exact), "worst count of right seeds", int(right.min()), report)
    assert right.min() >= 9, (name, log2m, right.tolist())
