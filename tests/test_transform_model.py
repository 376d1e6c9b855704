"""CPU: the model of the transforms (tests/transform_model.py) against the reference's two comparators, written out here position by
position as Transform.java has them, and against itself on the golden text.

The lexicographic comparator of the reference (Transform.java:2017-2032) returns the sign of b - a at the first differing position: the
LARGER successor goes first, whatever its javadoc says.  The key forms of the model state that order; the exhaustive test below is what
pins them to the code."""
import itertools

import numpy as np

import transform_model as M


def java_lex(x, y):
    """Transform.java:2017-2032: -1 stands for the end of a list."""
    i, j = iter(list(x) + [-1]), iter(list(y) + [-1])
    while True:
        a, b = next(i), next(j)
        if a == -1 and b == -1:
            return 0
        if a == -1:
            return -1
        if b == -1:
            return 1
        if a != b:
            t = b - a
            return 0 if t == 0 else -1 if t < 0 else 1


def java_gray(x, y):
    """Transform.java:1946-1975."""
    i, j = iter(list(x) + [-1]), iter(list(y) + [-1])
    parity = False
    while True:
        a, b = next(i), next(j)
        if a == -1 and b == -1:
            return 0
        if a == -1:
            return 1 if parity else -1
        if b == -1:
            return -1 if parity else 1
        if a != b:
            return 1 if parity ^ (a < b) else -1
        parity = not parity


def _sign(a, b):
    return (a > b) - (a < b)


def test_key_forms_are_the_comparators_on_every_pair_of_subsets():
    subsets = [c for r in range(7) for c in itertools.combinations(range(6), r)]
    assert len(subsets) == 64
    for x in subsets:
        for y in subsets:
            assert _sign(M.lex_key(x), M.lex_key(y)) == java_lex(x, y), (x, y)
            assert _sign(M.gray_key(x), M.gray_key(y)) == java_gray(x, y), (x, y)


def test_key_forms_on_random_longer_lists():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        n = int(rng.integers(1, 40))
        x = np.flatnonzero(rng.random(n) < 0.5); y = np.flatnonzero(rng.random(n) < 0.5)
        if rng.random() < 0.3:
            y = x[:int(rng.integers(0, len(x) + 1))]                       # a prefix
        assert _sign(M.lex_key(x), M.lex_key(y)) == java_lex(x, y)
        assert _sign(M.gray_key(x), M.gray_key(y)) == java_gray(x, y)


def test_vectorised_keys_are_the_key_forms():
    rng = np.random.default_rng(9)
    lists = [np.flatnonzero(rng.random(30) < d) for d in rng.random(200)] + [[], [], [3], [3]]
    off, adj = M.csr(lists)
    assert M.keys_of(off, adj, False) == [M.lex_key(l) for l in lists]
    assert M.keys_of(off, adj, True) == [M.gray_key(l) for l in lists]
    assert np.array_equal(M.permutation_of_csr(off, adj, True), M.gray_code_permutation(lists))
    assert np.array_equal(M.permutation_of_csr(off, adj, False), M.lexicographical_permutation(lists))


def test_orders_on_a_hand_case():
    lists = [[], [0], [0, 1], [1], [0, 1], [2]]
    # lex: the empty list, then the larger first successor first; [0] before [0, 1]; the two equal lists by node id
    assert list(np.argsort(M.lexicographical_permutation(lists))) == [0, 5, 3, 1, 2, 4]
    # Gray: position 1 is odd -- [0, 1] continues and so goes BEFORE [0], which ends there
    assert list(np.argsort(M.gray_code_permutation(lists))) == [0, 5, 3, 2, 4, 1]


def test_small_transforms():
    off, adj = M.csr([[1, 2], [1], [0]])
    assert M.same(M.transpose(off, adj), M.csr([[2], [0, 1], [0]]))
    assert M.same(M.filter_arcs(off, adj, "NO_LOOPS"), M.csr([[1, 2], [], [0]]))
    assert M.same(M.filter_arcs(off, adj, "SAME_CLASS", [0, 0, 1]), M.csr([[1], [1], []]))
    assert M.same(M.filter_arcs(off, adj, "DIFFERENT_CLASS", [0, 0, 1]), M.csr([[2], [], [0]]))
    assert M.same(M.map_graph(off, adj, [0, 0, -1]), M.csr([[0]]))                       # merged images, a loop made by merging, a deleted node
    assert M.same(M.map_graph(off, adj, [4, 1, 0]), M.csr([[4], [1], [], [], [0, 1]]))    # a value beyond n: empty nodes in between
    assert M.same(M.map_graph(off, adj, [-1, -1, -1]), M.csr([]))
    assert M.same(M.union((off, adj), M.csr([[], [], [], [3]])), M.csr([[1, 2], [1], [0], [3]]))
    assert M.same(M.symmetrize(off, adj, drop_loops=True), M.csr([[1, 2], [0], [0]]))
    assert list(M.remove_dangling_map(M.csr([[1], [], [0], []])[0])) == [0, -1, 1, -1]


def test_mix64_is_splitmix():
    # SplitMix64 seeded with `seed`: its first outputs are mix64(seed, 0), mix64(seed, 1), ... (published test vector of seed 1234567)
    assert [M.mix64(1234567, i) for i in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    p = M.random_permutation(100, 7)
    assert sorted(p) == list(range(100)) and not np.array_equal(p, M.random_permutation(100, 8))


def test_transpose_twice_and_map_back_are_the_identity_on_the_golden_text(cnr_golden, cnr_csr):
    deg, succ = cnr_csr
    g = (np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ)
    assert M.same(M.transpose(*M.transpose(*g)), g)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(deg)).astype(np.int64)
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    assert M.same(M.map_graph(*M.map_graph(*g, perm), inv), g)
