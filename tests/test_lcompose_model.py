"""CPU: the model of the labelled product (tests/lcompose_model.py) pinned on the reference's own case (TransformTest.testLabelledCompose) and
on two identities: its structure is the unlabelled product's (tests/compose_model.py), and (+, x) over labels that are all 1 counts, per arc,
the nodes y that join it."""
import numpy as np
import pytest

import compose_model as CM
import lcompose_model as LC

REFERENCE_ARCS = [(0, 1, 2), (0, 2, 10), (0, 3, 1), (1, 2, 4), (3, 2, 1)]


def reference_graph():
    rows = [[] for _ in range(4)]
    for x, y, l in REFERENCE_ARCS:
        rows[x].append((y, l))
    return LC.from_rows(rows)


def random_graph(rng, n, p, lab_max):
    rows = [[(int(y), int(rng.integers(0, lab_max + 1))) for y in np.flatnonzero(rng.random(n) < p)] for _ in range(n)]
    return LC.from_rows(rows)


def test_the_references_own_case():
    g = reference_graph()
    assert LC.compose_rows(g, g, LC.MIN_PLUS) == [[(2, 2)], [], [], []]        # 0 -> 3 -> 2 (1 + 1) beats 0 -> 1 -> 2 (2 + 4)
    status, got = LC.compose(g, g, LC.MIN_PLUS)
    assert status == "ok" and got[0].tolist() == [0, 1, 1, 1, 1] and got[1].tolist() == [2] and got[2].tolist() == [2]


def test_the_five_semirings_on_the_references_case():
    g = reference_graph()
    want = {LC.MIN_PLUS: 2, LC.MAX_PLUS: 6, LC.MAX_MIN: 2, LC.MIN_MAX: 1, LC.PLUS_TIMES: 9}   # the paths 2, 4 and 1, 1
    for s, label in want.items():
        assert LC.compose_rows(g, g, s) == [[(2, label)], [], [], []], s


@pytest.mark.parametrize("na, nb", [(40, 40), (60, 13), (13, 60)])
def test_structure_is_the_unlabelled_product(na, nb):
    rng = np.random.default_rng(na * 100 + nb)
    a = random_graph(rng, na, 0.15, 50)
    b = random_graph(rng, nb, 0.2, 50)
    b = LC.make(b[0], b[1], b[2])
    # a's successors range over [0, na): those >= nb are the ones that contribute nothing
    want = CM.compose(LC.underlying(a), LC.underlying(b))
    for s in LC.SEMIRINGS:
        rows = LC.compose_rows(a, b, s)
        got = LC.from_rows(rows)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), s


def test_plus_times_over_ones_counts_the_joining_nodes():
    rng = np.random.default_rng(4)
    a, b = random_graph(rng, 50, 0.2, 0), random_graph(rng, 50, 0.2, 0)
    a, b = LC.make(a[0], a[1], np.ones(len(a[1]))), LC.make(b[0], b[1], np.ones(len(b[1])))
    succ_a = [set(z for z, _ in r) for r in LC.rows_of(a)]
    pred_b = [set() for _ in range(50)]
    for y, r in enumerate(LC.rows_of(b)):
        for z, _ in r:
            pred_b[z].add(y)
    rows = LC.compose_rows(a, b, LC.PLUS_TIMES)
    assert sum(len(r) for r in rows) > 100
    for x, r in enumerate(rows):
        for z, v in r:
            assert v == len(succ_a[x] & pred_b[z]) >= 1


def test_the_range_rule():
    one = LC.from_rows([[(1, 255)], [(2, 1)], []])
    assert LC.compose(one, one, LC.MIN_PLUS, LC.FIXED, 8) == ("range", 1, (0, 2))
    status, got = LC.compose(one, one, LC.MIN_PLUS, LC.FIXED, 9)
    assert status == "ok" and got[2].tolist() == [256]
    top = (1 << 31) - 1
    g = LC.from_rows([[(1, top)], [(2, top)], []])
    assert LC.compose(g, g, LC.MIN_PLUS, LC.GAMMA)[0] == "range" and LC.compose(g, g, LC.MIN_MAX, LC.GAMMA)[0] == "ok"
    two = LC.from_rows([[(2, 200)], [(2, 200)], [(0, 100), (3, 100)], []])    # 300 on (0, 0), (0, 3), (1, 0), (1, 3) and (2, 2): the smallest is (0, 0)
    assert LC.compose(two, two, LC.MAX_PLUS, LC.FIXED, 8) == ("range", 5, (0, 0))
    assert LC.class_max(LC.FIXED, 0) == 0 and LC.class_max(LC.GAMMA, 0) == top
