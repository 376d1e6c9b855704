"""GPU: the wave-wide interval fill of the lean scan kernel (csrc/bvg_scan.hip), on hand-assembled records (tests/bvrecords.py).

A stored list without reference that has intervals (a `d2` root) is decoded in place: its residuals go straight to their places, and right behind the residual phase of
its sub-row all 64 lanes write its intervals, one list after the other, 64 consecutive elements a trip; lane k fetches entry k of the list's interval table, 64 entries a
fetch.  The root is then complete before any level of the sub-row runs, whoever copies from it.

Every group of 13 records holds a root R whose shape goes with the group's kind (the interval lengths on either side of the 64-lane stride, a list that is only intervals,
an interval in front of the first and behind the last residual, two intervals that touch, 63 / 64 / 65 intervals: the entry table is fetched once, once, twice), three
copiers of R in its own sub-row -- one whose mask keeps exactly R's first interval, one that skips exactly it, one that cuts it in the middle --, a chain of depth 3 below
R, a copier of R at distance W (another sub-row or super-row), and three more d2 roots U, V, X with one copier each (four d2 roots in 13 records: three and more share a
sub-row).  13 and 64 are coprime, so over 320 groups every root is the last node of a sub-row, of a super-row and of a block somewhere.
The result is the oracle's: the whole scan, every node of the checked groups alone (then the root lies outside [from, to): its key is 0, it must be filled and add
nothing), and every list out of the materialising form, which shares the code."""
import os
import re

import numpy as np
import pytest

from bvrecords import Record, assemble

pytestmark = pytest.mark.gpu

KNOBS = ("BVG_EMIT", "BVG_DBG", "BVG_NOSKIP", "BVG_SCANK", "BVG_SCAN_POOL", "BVG_SCAN_SCR", "BVG_SCAN_WAVES", "BVG_NO_D2", "BVG_MAT_LEAN", "BVG_DEBUG")
G = 13                    # records per group
KINDS = 8                 # shapes of R
NGROUPS = 320             # 4 160 nodes: a scan of 4 096 nodes and more builds the skip index and validates the blocks (bvg_sched.hip ensure_skip)
W7 = 7
SPAN = 1900               # values of a group lie in [vb, vb + SPAN)
PLACES = int(os.environ.get("BVG_FILLS_PLACES", "2"))   # runs of KINDS groups that are checked node by node (the emulated run, tests/test_emu_interval_fills.py, takes one)
M64 = (1 << 64) - 1


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BVG_EMIT", "1")


def _kept(base, blocks):
    """MaskedLongIterator.java:73-100: blocks alternate keep / skip; behind an even number of blocks the tail is kept."""
    out, pos = [], 0
    for i, b in enumerate(blocks):
        if i % 2 == 0: out += base[pos:pos + b]
        pos += b
    if len(blocks) % 2 == 0: out += base[pos:]
    return out


def _node(lists, ref, blocks, residuals=(), intervals=()):
    x = len(lists)
    kept = _kept(lists[x - ref], blocks) if ref else []
    ivals = [l + k for l, n in intervals for k in range(n)]
    parts = kept + list(residuals) + ivals
    assert len(set(parts)) == len(parts), "the three streams of a record must be disjoint (node %d)" % x
    lists.append(sorted(parts))
    return Record(d=len(parts), ref=ref, blocks=blocks, intervals=sorted(intervals), residuals=sorted(residuals))


def _shape(v0, items):
    """A root's extras from v0 on.  items: ('r', n) n residuals three apart, ('i', len) an interval and a gap behind it, ('t', len) an interval that TOUCHES the next one
    (left2 = left1 + len1 + 1: the gap code is 0)."""
    res, ivs, v = [], [], v0
    for what, n in items:
        if what == "r":
            res += [v + 3 * i for i in range(n)]; v += 3 * n
        else:
            ivs.append((v, n)); v += n + (1 if what == "t" else 3)
    return res, ivs


def _root_items(kind, m):
    """R's shape by kind; m = min_interval_length."""
    return {
        0: [("r", 7), ("i", m), ("r", 6), ("i", 63), ("r", 7), ("i", 64), ("r", 2)],          # below and on the stride; 22 residuals: skip entries, residual tasks
        1: [("r", 2), ("i", 65), ("r", 1), ("i", 128)],                                         # one past the stride, two full trips; 3 residuals: no skip entry
        2: [("r", 9), ("i", 129), ("r", 9), ("i", 200), ("r", 4)],                              # two trips and one element, about 200
        3: [("i", m), ("i", 7)],                                                                # only intervals: no residual at all
        4: [("i", 5), ("r", 10), ("t", 6), ("i", 9), ("r", 10), ("i", m + 1)],                  # an interval in front of the first residual, two that touch, one behind the last
        5: [("r", 1)] + [("i", m)] * 63 + [("r", 2)],                                           # 63 entries
        6: [("r", 18)] + [("i", m)] * 64,                                                       # 64 entries: one fetch, every lane holds one
        7: [("i", m)] * 30 + [("r", 3)] + [("i", m + 2)] * 35,                                  # 65 entries: a second fetch for the last one
    }[kind]


def _group(recs, lists, g, vb, m):
    kind = g % KINDS
    res_r, iv_r = _shape(vb + 10, _root_items(kind, m))
    recs.append(_node(lists, 0, [], res_r, iv_r)); R = lists[-1]      # 0: R
    L = len(R)
    left, ln = iv_r[0]; p0 = R.index(left)
    # 1: keeps EXACTLY R's first interval (skip p0, keep ln, drop the tail); a residual of its own and an interval (stored: 4 copies it)
    recs.append(_node(lists, 1, [0, p0, ln] if p0 else [ln], [vb + 1000], [(vb + 1010, m + 3)]))
    # 2: skips EXACTLY R's first interval (keep p0, skip ln, keep the tail); where the interval has an inner element, a residual of its own lies on it
    recs.append(_node(lists, 2, [p0, ln], [left + 1] if ln >= 3 else [vb + 1100], []))
    # 3: cuts R's LAST interval in the middle (keeps everything up to its middle, drops the rest) + residuals above
    l2, n2 = iv_r[-1]; q0 = R.index(l2)
    recs.append(_node(lists, 3, [q0 + max(1, n2 // 2)], [vb + 1200 + 5 * i for i in range(3)], []))
    # 4: copies 1 (depth 2), 5: copies 4 (depth 3)
    recs.append(_node(lists, 3, [max(1, ln // 2), 1], [vb + 1300], [(vb + 1310, m)]))
    recs.append(_node(lists, 1, [], [vb + 1400, vb + 1404], []))
    # 6: U, one interval between residuals
    res_u, iv_u = _shape(vb + 1450, [("r", 5), ("i", m + 9), ("r", 4)])
    recs.append(_node(lists, 0, [], res_u, iv_u)); U = lists[-1]
    # 7: R a second time, at distance W: a sub-row (or a super-row, or a block) later
    recs.append(_node(lists, 7, [L // 2], [vb + 1500], []))
    # 8: V, two intervals and nothing else for odd g, residuals around them for even g; 9: X, an interval behind the residuals
    res_v, iv_v = _shape(vb + 1520, [("i", m), ("i", 70)] if g % 2 else [("r", 3), ("i", m), ("r", 17), ("i", 70), ("r", 1)])
    recs.append(_node(lists, 0, [], res_v, iv_v)); V = lists[-1]
    res_x, iv_x = _shape(vb + 1700, [("r", 6), ("i", 66)])
    recs.append(_node(lists, 0, [], res_x, iv_x)); X = lists[-1]
    # 10: copies U, 11: copies V (keeps the second interval's first 64 elements and nothing else), 12: copies X (all of it)
    recs.append(_node(lists, 4, [len(U) // 2, 2], [vb + 1800], [(vb + 1810, m)]))
    v1 = V.index(iv_v[1][0])
    recs.append(_node(lists, 3, [0, v1, 64], [], []))
    recs.append(_node(lists, 3, [], [], []))


_cache = {}


def _stream(m):
    if m not in _cache:
        n = NGROUPS * G
        recs, lists = [], []
        for g in range(NGROUPS):
            _group(recs, lists, g, min(g * G, n - SPAN), m)
        gbytes, offs, expect = assemble(recs, min_interval=m, max_ref=4)
        assert [list(l) for l in expect] == lists, "the hand-computed lists disagree with the restated iterators"
        assert 0 <= min(l[0] for l in lists if l) and max(l[-1] for l in lists if l) < n
        _cache[m] = (recs, np.frombuffer(gbytes, dtype=np.uint8), offs, lists)
    return _cache[m]


# (stream's min_interval_length, environment, force_wide)
CASES = {
    "pool1024": (4, {"BVG_SCAN_POOL": "1024"}, False),
    "pool640": (4, {"BVG_SCAN_POOL": "640"}, False),                      # the longest root and its copiers barely share a sub-row
    "min2": (2, {"BVG_SCAN_POOL": "1024"}, False),                       # intervals of two elements
    "wide": (4, {"BVG_SCAN_POOL": "1024"}, True),                        # the 64-bit-id path: ids relative to the block's base
    "waves18": (4, {"BVG_SCAN_POOL": "1024", "BVG_SCAN_WAVES": "18"}, False),   # the 96-VGPR instantiation
    "no_d2": (4, {"BVG_SCAN_POOL": "1024", "BVG_NO_D2": "1"}, False),    # the in-place decode compiled out: a root with intervals is a member of level 0
    "scank0": (4, {"BVG_SCANK": "0"}, False),                            # the control: the lean kernel kept away, the row kernel alone
}


def _open(W, oracle, m, wide):
    recs, graph, offs, lists = _stream(m)
    n = len(recs)
    p = W.default_params(max_ref_count=4, min_interval_length=m).clone(nodes=n, arcs=int(sum(len(l) for l in lists)))
    assert p.window_size == W7 and p.arcs / n > 48.0                  # (bvg_sched.hip lean_geometry: the dense instantiations, which have the in-place decode)
    og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), offs)
    hg = W.BVGraph.from_memory(p, graph, offs)
    if wide: hg.set_tuning(force_wide=True)
    return p, og, hg


@pytest.mark.parametrize("case", sorted(CASES))
def test_interval_fills_against_the_oracle(W, oracle, monkeypatch, capfd, case):
    m, env, wide = CASES[case]
    recs, graph, offs, lists = _stream(m)
    n = len(recs)
    lean = case != "scank0"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_MAT_LEAN", "1")
    p, og, hg = _open(W, oracle, m, wide)
    o = og.scan()
    assert o["arcs"] == p.arcs
    r1 = hg.scan()                                                     # builds the index and validates the blocks
    capfd.readouterr()
    r2 = hg.scan()
    err = capfd.readouterr().err
    for r in (r1, r2):
        assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"])
    if lean:
        assert r2["lean_blocks"] > 0, "the lean scan kernel did not run"
        geo = re.findall(r"scan kernel: pool (\d+) \+ scratch (\d+) elements, window (\d+) dwords, (\d+) wavefronts per CU", err)
        assert geo and int(geo[-1][0]) == int(env["BVG_SCAN_POOL"]), err[-2000:]
        assert int(geo[-1][3]) == (18 if case == "waves18" else 16), geo
    else:
        assert r2["lean_blocks"] == 0
    # node by node: KINDS groups in a row (every shape of R, the copiers that reach back into the group before) at the places of the stream
    for g0 in (1, NGROUPS // 2 + 3)[:PLACES]:
        for y in range(g0 * G, (g0 + KINDS) * G):
            ry, oy = hg.scan(y, y + 1), og.scan(y, y + 1)
            if lean: assert ry["lean_blocks"] > 0, (case, y)
            assert (ry["arcs"], ry["chk"]) == (len(lists[y]), oy["chk"]), (case, y)
    # the materialising form: every list, successor by successor
    odeg, osucc = og.decode_range(0, n)
    assert osucc.tolist() == [v for l in lists for v in l]
    capfd.readouterr()
    deg, succ = hg.decode_range(0, n)
    err = capfd.readouterr().err
    if lean:
        k = re.search(r"scan kernel (\d+) \+ (\d+)/(\d+)/(\d+)/(\d+) LDS-class", [l for l in err.splitlines() if "tiers concurrent" in l][-1])
        assert sum(int(v) for v in k.groups()) > 0, "the materialising call did not run the lean kernel"
    assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc), case
    hg.close()


def _k1(x):
    h = ((x & 0xFFFFFFFF) * 0x9E3779B1 + (x >> 32) * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 15; h = (h * 0x2C1B3C6D) & 0xFFFFFFFF; h ^= h >> 12
    return h | 1


def _moved_stream(gm):
    """The stream of min_interval_length 4 with ONE interval of ONE root moved: group gm (kind 0), R's interval of 63 elements starts one lower.  The element below
    its old left end joins the list, its old last element leaves; both lie in gaps, so the list stays sorted and free of duplicates and every mask keeps its shape."""
    recs, lists = [], []
    n = NGROUPS * G
    for g in range(NGROUPS):
        _group(recs, lists, g, min(g * G, n - SPAN), 4)
    x = gm * G
    r = recs[x]
    k = [i for i, (_, ln) in enumerate(r.intervals) if ln == 63][0]
    left, ln = r.intervals[k]
    r.intervals[k] = (left - 1, ln)
    gbytes, offs, expect = assemble(recs, min_interval=4, max_ref=4)
    return np.frombuffer(gbytes, dtype=np.uint8), offs, [list(l) for l in expect], left - 1, left + ln - 1


def test_a_moved_interval_moves_the_checksum_by_the_linear_term(W, oracle, monkeypatch):
    """The checksum contract (include/bvgraph_hip.h; tests/test_gpu_checksum_integrity.py) on an interval element of a d2 root: moving the interval's left end one down
    swaps the element `gone` for the element `come`.  The root and every copier that keeps the interval move by exactly k1(node) * (come - gone), the copier whose mask
    cuts the interval by k1(node) times the change of the sum of the elements it keeps, every other node not at all."""
    monkeypatch.setenv("BVG_SCAN_POOL", "1024")
    gm = 8 * 11                                                         # a group of kind 0 in the middle of the stream
    _, ga, offa, la = _stream(4)
    gb, offb, lb, come, gone = _moved_stream(gm)
    n = NGROUPS * G
    p = W.default_params(max_ref_count=4).clone(nodes=n, arcs=int(sum(len(l) for l in la)))
    hs = []
    for gr, offs in ((ga, offa), (gb, offb)):
        og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), gr.tobytes(), offs)
        hg = W.BVGraph.from_memory(p, gr, offs)
        o = og.scan(); r1 = hg.scan(); r2 = hg.scan()
        assert (r1["arcs"], r1["chk"]) == (o["arcs"], o["chk"]) and (r2["arcs"], r2["chk"]) == (o["arcs"], o["chk"])
        assert r2["lean_blocks"] > 0, "the lean scan kernel did not run"
        hs.append((og, hg, o))
    (oga, hga, oa), (ogb, hgb, ob) = hs
    movers, total = 0, 0
    for y in range((gm - 1) * G, (gm + 2) * G):
        ra, rb = hga.scan(y, y + 1), hgb.scan(y, y + 1)
        assert ra["lean_blocks"] > 0 and rb["lean_blocks"] > 0
        assert ra["chk"] == oga.scan(y, y + 1)["chk"] and rb["chk"] == ogb.scan(y, y + 1)["chk"]
        assert len(la[y]) == len(lb[y]) == ra["arcs"] == rb["arcs"]
        delta = sum(lb[y]) - sum(la[y])                                 # the linear term: k1 times the change of the sum of the node's successors
        if y != gm * G + 7: assert set(lb[y]) - set(la[y]) <= {come} and set(la[y]) - set(lb[y]) <= {gone}   # (7 cuts the moved interval: its positions hold other elements)
        assert (rb["chk"] - ra["chk"]) & M64 == (_k1(y) * delta) & M64, "node %d" % y
        if delta: movers += 1
        else: assert la[y] == lb[y]
        total += _k1(y) * delta
    assert movers >= 3, "the root and at least two of its copiers hold the moved element"
    assert la[gm * G] != lb[gm * G]
    assert (ob["chk"] - oa["chk"]) & M64 == total & M64
    for _, hg, _ in hs:
        hg.close()
