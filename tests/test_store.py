"""CPU: the tooling encoder (webgraph-big_amd/tools/bvg_store.cpp) is held to the reference's bytes:
re-storing the text golden with the fixture's parameters reproduces cnr-2000.graph / .offsets exactly
(SURVEY section 7 step 3), and store -> oracle decode round-trips (BVGraphTest.testCompression,
test/.../BVGraphTest.java:52-103)."""
import itertools

import numpy as np
import pytest

from conftest import CNR


def test_restore_reproduces_fixture_bytes(W, tools, cnr_golden):
    st = tools.store(cnr_golden, W.default_params(min_interval_length=3))
    assert st.graph.tobytes() == open(CNR + ".graph", "rb").read()
    assert st.offsets_file().tobytes() == open(CNR + ".offsets", "rb").read()
    s = st.stats
    assert (s["copied"], s["intervalised"], s["residual"], s["nodes_with_ref"]) == (2130833, 361894, 723425, 181798)
    assert round(s["tot_ref"] / 325557, 2) == 1.38 and round(s["tot_dist"] / 325557, 2) == 1.74


def _binary_tree(n, out=True):
    lists = [[] for _ in range(n)]
    for i in range(n):
        for c in (2 * i + 1, 2 * i + 2):
            if c < n:
                (lists[i] if out else lists[c]).append(c if out else i)
    return [sorted(l) for l in lists]


@pytest.mark.parametrize("w,r,mi", list(itertools.product([0, 1, 2], [0, 1, 2], [0, 1, 2, 3])))
def test_compression_roundtrip_small_trees(W, tools, oracle, w, r, mi):
    """BVGraphTest.testCompression: complete binary in/out-trees n=1..7 x window x maxRef x minInterval."""
    for n in range(1, 8):
        for out in (True, False):
            lists = _binary_tree(n, out)
            st = tools.store(lists, W.default_params(window_size=w, max_ref_count=r, min_interval_length=mi))
            assert len(st.graph) == (int(st.offsets[-1]) + 7) // 8                       # file length == ceil(bits/8), :68-74
            assert st.stats["copied"] + st.stats["intervalised"] + st.stats["residual"] == sum(map(len, lists))   # :76
            og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
            for x in range(n):
                assert og.successors(x).tolist() == lists[x]
            it = og.node_iterator(0)
            for x in range(n):
                assert it.next() == x and it.successors().tolist() == lists[x]


@pytest.mark.parametrize("kw", [dict(), dict(residual_coding=1), dict(residual_coding=2), dict(residual_coding=7), dict(residual_coding=3, zeta_k=4),
                                dict(outdegree_coding=1, block_coding=1, reference_coding=1, block_count_coding=1, offset_coding=1),
                                dict(reference_coding=2, block_count_coding=5, block_coding=5), dict(zeta_k=1), dict(zeta_k=7),
                                dict(window_size=0, max_ref_count=0, min_interval_length=0), dict(window_size=30, max_ref_count=-1)])
def test_synthetic_roundtrip_all_codings(W, tools, oracle, kw):
    n = 4000
    p = W.default_params(**kw)
    st = tools.synth_store(n, seed=11, params=p, chunk_nodes=1024, threads=3)
    off, adj = tools.synth_adjacency(n, seed=11, chunk_nodes=1024)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    deg, succ = og.decode_range(0, n)
    assert np.array_equal(deg, np.diff(off).astype(np.int32)) and np.array_equal(succ, adj)
    # offsets file round-trip with the chosen offset coding
    ob = st.offsets_file().tobytes()
    assert np.array_equal(oracle.decode_offsets(ob, n, st.params.offset_coding), st.offsets)
    # properties text round-trip
    if kw.get("block_coding") != 5:      # BVGraph declares no BLOCKS_UNARY constant (BVGraph.java:482-485): not expressible in .properties
        p2 = oracle.parse_properties(st.properties_text())
        assert p2.as_dict() == {**st.params.as_dict()}
    else:
        with pytest.raises(oracle.OracleError):
            oracle.parse_properties(st.properties_text())


def test_store_is_thread_count_invariant(W, tools):
    a = tools.synth_store(30000, seed=5, chunk_nodes=4096, threads=1)
    b = tools.synth_store(30000, seed=5, chunk_nodes=4096, threads=7)
    assert a.graph.tobytes() == b.graph.tobytes() and np.array_equal(a.offsets, b.offsets)


def test_hand_built_branch_graphs(W, tools, oracle):
    """One node per decoder branch of BVGraph.java:1003-1064."""
    lists = [
        [],                                   # d = 0
        [5, 9, 13, 20],                       # ref = 0, residuals only
        [5, 9, 13, 20],                       # ref = 1, zero blocks (copy everything)
        [5, 9, 13],                           # ref, odd block count (tail dropped)
        [9, 13, 20],                          # first block 0
        [9, 13, 20, 30, 31, 32, 33, 34],      # copy + interval
        [0, 1, 2, 3, 4, 5, 6],                # interval with negative first left (relative to x = 6)
        [2, 40, 41, 42, 43, 50],              # negative first residual, interval in the middle
        list(range(100, 400)),                # long interval
        [3] + list(range(100, 400)) + [999],  # copy of a long list + extras on both sides
    ]
    for w, r, mi in [(7, 3, 4), (7, 3, 2), (1, 1, 0), (0, 0, 0), (3, 1000, 3)]:
        st = tools.store(lists, W.default_params(window_size=w, max_ref_count=r, min_interval_length=mi))
        og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
        for x, l in enumerate(lists):
            assert og.successors(x).tolist() == l
        deg, succ = og.decode_range(0, len(lists))
        assert succ.tolist() == [v for l in lists for v in l]


# intervalize (BVGraph.java:1595-1618) by hand.  It walks the extras v[0..vl); at i it opens an interval only if v[i] + 1 == v[i + 1], counts
# the run's length j (so j >= 2 whenever j != 0), keeps it if j >= min and otherwise leaves j = that short length; `if (j < min)` then
# makes v[i] -- alone -- a residual and the walk goes on at i + 1.  Hence, for every minimum:
#   [5]           no neighbour: j = 0 < min, residual 5.  Also for min = 1: an interval of one element does not exist.
#   [5, 6]        j = 2: one interval (5, 2) for min 1 and 2; for min 3, 2 < 3 makes 5 a residual, then i = 1 is the last element: 6 too.
#   [5, 7]        5 + 1 != 7: two residuals.
#   [5, 6, 7, 9]  j = 3 at i = 0: interval (5, 3) for min 1, 2, 3 (i jumps to 3); 9 is last: residual.
#   [0, 1, 2, 3]  j = 4: interval (0, 4), no residual; written at node 3 the left extreme is coded as int2nat(0 - 3) = 5.
_INTERVALIZE_BY_HAND = [    # (node, list, min_interval_length, intervals (left, len), residuals)
    (0, [5], 1, [], [5]), (0, [5], 2, [], [5]), (0, [5], 3, [], [5]),
    (0, [5, 6], 1, [(5, 2)], []), (0, [5, 6], 2, [(5, 2)], []), (0, [5, 6], 3, [], [5, 6]),
    (0, [5, 7], 1, [], [5, 7]), (0, [5, 7], 2, [], [5, 7]), (0, [5, 7], 3, [], [5, 7]),
    (0, [5, 6, 7, 9], 1, [(5, 3)], [9]), (0, [5, 6, 7, 9], 2, [(5, 3)], [9]), (0, [5, 6, 7, 9], 3, [(5, 3)], [9]),
    (3, [0, 1, 2, 3], 1, [(0, 4)], []), (3, [0, 1, 2, 3], 2, [(0, 4)], []), (3, [0, 1, 2, 3], 3, [(0, 4)], []),
]

# The records themselves for min_interval_length = 1, window_size = 0 (BVG:2092-2125: gamma outdegree; no reference field without a window;
# gamma interval count; per interval gamma(int2nat(left - node)) then gamma(len - min); residuals zeta_3, the first as int2nat(r - node)).
# gamma(x): with v = x + 1 and b = msb(v), b zeros, a one, the b low bits of v.  zeta_3(x): v = x + 1, h = msb(v) / 3, h zeros, a one, then
# v - 8^h in 3h + 2 bits if v < 2 * 8^h.
#   [5] at node 0:     outdegree gamma(1) = 010 | count gamma(0) = 1 | residual zeta_3(int2nat(5) = 10): v = 11, h = 1: 01, 11 - 8 = 3 in 5 bits 00011
#   [5, 6] at node 0:  outdegree gamma(2) = 011 | count gamma(1) = 010 | left gamma(10): v = 11 = 1011b: 000 1 011 | length gamma(2 - 1) = 010
_RECORD_BITS_BY_HAND = {(5,): "010" "1" "0100011", (5, 6): "011" "010" "0001011" "010"}


@pytest.mark.parametrize("x,l,m,intervals,residuals", _INTERVALIZE_BY_HAND)
def test_intervalize_against_expectations_computed_by_hand(W, tools, x, l, m, intervals, residuals):
    """The device compressor is held to this encoder (tests/test_gpu_store.py), this encoder to the reference's fixture at
    min_interval_length = 3 only: here its intervals are pinned for 1, 2 and 3 to what BVGraph.intervalize does on paper."""
    from bvrecords import PyBits, Record
    n = 10
    lists = [l if y == x else [] for y in range(n)]
    st = tools.store(lists, W.default_params(min_interval_length=m, window_size=0))
    assert (st.stats["intervalised"], st.stats["residual"], st.stats["copied"]) == (sum(ln for _, ln in intervals), len(residuals), 0)
    w = PyBits()
    Record(len(l), intervals=intervals, residuals=residuals).write(w, x, 0, m, 3, len(l))
    want = "1" * x + "".join(map(str, w.bits)) + "1" * (n - 1 - x)                    # (an empty list is gamma(0) = 1)
    assert st.offsets.tolist() == list(range(x + 1)) + [x + len(w) + i for i in range(n - x)]
    got = "".join(map(str, np.unpackbits(st.graph)[:len(want)]))
    assert got == want and len(st.graph) == (len(want) + 7) // 8
    if m == 1 and tuple(l) in _RECORD_BITS_BY_HAND:
        assert got[x:x + len(w)] == _RECORD_BITS_BY_HAND[tuple(l)]
