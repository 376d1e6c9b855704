"""CPU: the EFGraph model (tests/efgraph_model.py) against the format as EFGraph.java states it -- the pinned vector, round trips, the
closed form of a record's length, skip_to against a linear search (EFGraphTest.testSkipFirst), both byte orders."""
import numpy as np
import pytest

import efgraph_model as M


def _er(n, p, seed):
    rng = np.random.default_rng(seed)
    return [np.flatnonzero(rng.random(n) < p).astype(np.int64) for _ in range(n)]


def test_pinned_vector():
    """lists [[1,3], [], [0,1,2,3], [2]], nodes = upperbound = 4, quantum = 2; the first record worked by hand: gamma(2) = 0 1 1, l = 0,
    pointer size 3, two pointers 3 and 6, upper bits 0100101 -> 16 bits."""
    lists = [[1, 3], [], [0, 1, 2, 3], [2]]
    data, off, info = M.store(lists, 4, 1)
    assert list(off) == [0, 16, 21, 43, 54]
    assert data.hex() == "9ea5911156d52800"
    assert M.write_delta_offsets(off).hex() == "945c5724"
    assert (M.lower_bits(3, 4), M.pointer_size(3, 4), M.number_of_pointers(3, 4, 1)) == (0, 3, 2)
    w = M.bytes_to_words(data)[0]
    assert [(w >> i) & 1 for i in range(3)] == [0, 1, 1]                               # gamma(2), LSB first
    assert ((w >> 3) & 7, (w >> 6) & 7) == (3, 6)                                      # the pointers
    assert [(w >> (9 + i)) & 1 for i in range(7)] == [0, 1, 0, 0, 1, 0, 1]             # the upper bits
    assert info == {"bitsforoutdegrees": 3 + 1 + 5 + 3, "bitsforsuccessors": 54 - 12, "arcs": 7}


def whole_word_streams(limit=300):
    """(k, data, offsets) of k empty lists, upper bound k, quantum 256, for every k whose stream is a whole number of words."""
    out = []
    for k in range(1, limit):
        data, off, _ = M.store([[]] * k, k, 8)
        if int(off[-1]) % 64 == 0:
            out.append((k, data, off))
    return out


def test_trailing_word_when_the_length_is_a_multiple_of_64():
    """close() writes the current word always (:408-413): bits / 64 + 1 words, one zero word more when the stream fills its last word."""
    for u in range(1, 200):
        data, off, _ = M.store([[]], u, 8)
        assert len(data) == 8 * (int(off[-1]) // 64 + 1)
    hits = whole_word_streams()
    assert hits, "no stream of a whole number of words in the sweep"
    for _, data, off in hits:
        assert len(data) == int(off[-1]) // 8 + 8 and data[-8:] == bytes(8)


@pytest.mark.parametrize("q", [0, 1, 3, 8])
@pytest.mark.parametrize("ub", ["n", "n+7", "n2", "2^40"])
def test_round_trip_and_closed_form(q, ub):
    n = 150
    lists = M.random_lists(n, 1500, seed=q * 7 + len(ub), degrees=(0, 1, 2, 3, 63, 64, 65, 150))
    U = {"n": n, "n+7": n + 7, "n2": n * n, "2^40": 1 << 40}[ub]
    for order in ("LITTLE_ENDIAN", "BIG_ENDIAN"):
        data, off, info = M.store(lists, U, q, order)
        for x in range(n):
            assert int(off[x + 1] - off[x]) == M.record_bits(len(lists[x]), U, q)
        g = M.Graph(n, U, q, data, off, order)
        for x in range(n):
            assert g.successors(x) == list(lists[x])
    le, be = M.store(lists, U, q, "LITTLE_ENDIAN")[0], M.store(lists, U, q, "BIG_ENDIAN")[0]
    assert be == np.frombuffer(le, "<u8").astype(">u8").tobytes() and (le != be or not any(le))


def _check_skip(lists, U, q, bounds_of):
    n = len(lists)
    data, off, _ = M.store(lists, U, q)
    g = M.Graph(n, U, q, data, off)
    for x in range(n):
        a = lists[x]
        for b in bounds_of(x):
            i = int(np.searchsorted(a, b))
            want = int(a[i]) if i < len(a) else -1
            assert g.skip_to(x, b) == want, (x, b)
            assert g.skip_to(x, b, use_pointers=False) == want, (x, b)


def test_skip_to_every_bound_100_nodes():
    """EFGraphTest.testSkipFirst: Erdos-Renyi, q = 3, every (node, bound)."""
    for p in (0.02, 0.3):
        _check_skip(_er(100, p, 1), 100, 3, lambda x: range(0, 101))


def test_skip_to_every_bound_1000_nodes():
    _check_skip(_er(1000, 0.01, 2), 1000, 3, lambda x: range(0, 1001))


def test_skip_to_large_upper_bounds():
    lists = _er(200, 0.1, 3)
    _check_skip(lists, 200 * 200, 2, lambda x: range(0, 201, 3))
    _check_skip(lists, 1 << 40, 0, lambda x: range(0, 201, 7))
    _check_skip(lists, 207, 1, lambda x: range(0, 208))


def test_sequential_reads_then_skip():
    lists = _er(120, 0.2, 4)
    data, off, _ = M.store(lists, 120, 3)
    g = M.Graph(120, 120, 3, data, off)
    for x in range(120):
        a = lists[x]
        r = g.reader(x)
        got = [r.next() for _ in range(min(3, len(a)))]
        assert got == list(a[:len(got)])
        for b in (0, 30, 60, 119, 120):
            i = max(int(np.searchsorted(a, b)), len(got) - 1 if got else 0)
            want = int(a[i]) if i < len(a) else -1
            if got and b <= got[-1]:
                want = got[-1] if r.last != M.END_OF_LIST else -1
            have = r.skip_to(b)
            assert have == want, (x, b)
            if have == -1:
                break
            got.append(have)


def test_writer_refuses_what_the_reference_refuses():
    with pytest.raises(ValueError):
        M.store([[1, 1]], 4, 1)
    with pytest.raises(ValueError):
        M.store([[5]], 4, 1)
