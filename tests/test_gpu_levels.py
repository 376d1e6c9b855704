"""GPU: the level rule and the liveness rule of the lean scan kernel (csrc/bvg_scan.hip), on hand-assembled records (tests/bvrecords.py).

LEVELS.  A stored list without reference is decoded straight into its place: `direct` (residuals only) or `d2` (residuals around intervals, the intervals filled in by
an extras pass).  Such a chain root is complete before the levels of its sub-row run, so a list that copies from it belongs to level 0, its child to level 1, ...
(BVGraph.java:1062-1090 builds a list from its referenced list, whatever the order).  Where the in-place decode is compiled out (BVG_NO_D2=1, the 85-VGPR instantiation of
sparse graphs) a root with intervals is a member of level 0 itself and its copiers wait for it.

LIVENESS.  A stored list is dropped from the pool once its last referencer has run: every reference of the super-row is known when its lists are built, and those of the
next super-row's first W records are read off their records (from the staged window, or from 12 bytes fetched from memory).  (Not in the 85-VGPR instantiation, which keeps
every stored list of the last W nodes; the materialising form and the LDS classes of the `sparse` case still drop.)

Every group of 13 records holds a root R (alternately direct and d2), a chain c1 -> c2 -> c3 below it with residuals and intervals at every depth, a second child of R
whose first extra lies below / inside / above R's first interval, a copier of R at distance W (a sub-row or a super-row later), a d2 root U whose copiers sit 4 and 6
nodes behind it, and a long direct root F.  13 and 64 are coprime, so over 540 groups every chain meets every sub-row, super-row and block boundary at every phase.
The records of these groups are short (64 of them and the heads of the next W fit the stream window: the next super-row's references are read from the window); the
`long` stream (_long_group) puts six records of 420 residuals between a stored root and its only copier, so that the copier's reference has to be read from memory.
Both ways of filling a d2 root's intervals run: in the `long` stream nothing that is built in a root's sub-row copies from it, so its intervals are filled by the extras
pass of level 0; in the other streams c1 stands right behind a d2 R, and wherever a sub-row holds both (a sub-row boundary cannot fall between them in all 270 such
groups: 13 and 64 are coprime and a sub-row holds several records) the fills run in a pass of their own in front of the levels.
The result is the oracle's: the whole scan, every node of the checked groups alone, and every list out of the materialising form (which shares the level logic)."""
import os
import re

import numpy as np
import pytest

from bvrecords import Record, assemble

pytestmark = pytest.mark.gpu

KNOBS = ("BVG_EMIT", "BVG_DBG", "BVG_NOSKIP", "BVG_SCANK", "BVG_SCAN_POOL", "BVG_SCAN_SCR", "BVG_SCAN_WAVES", "BVG_NO_D2", "BVG_MAT_LEAN", "BVG_DEBUG")
G = 13                    # records per group
W7 = 7                    # window
PLACES = int(os.environ.get("BVG_LEVELS_PLACES", "3"))   # places of the stream that are checked node by node (the emulated run, tests/test_emu_levels.py, takes one)
SCR = 448                 # the scratch area that comes on top of BVG_SCAN_POOL (bvg_sched.hip: scan_scr)


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


def _group(recs, lists, g, vb, NR, NU, NF, nfill):
    """Appends group g (values from vb on).  NR / NU / NF: residuals of R, U and F."""
    kind = g % 4                                                      # 0, 2: R is direct; 1: d2, intervals between its residuals; 3: d2, intervals before and behind them
    res_r = [vb + 10 + 9 * i for i in range(NR)]
    top = res_r[-1]
    iv_r = {0: [], 2: [], 1: [(vb + 10 + 9 * (NR // 3) + 2, 5), (vb + 10 + 9 * (2 * NR // 3) + 2, 6)], 3: [(vb + 2, 5), (top + 20, 4)]}[kind]
    recs.append(_node(lists, 0, [], res_r, iv_r)); R = lists[-1]      # 0: R
    L = len(R)
    # 1: c1 copies R (odd block count: the tail is dropped) + residuals in and above R's range + an interval
    recs.append(_node(lists, 1, [L // 3, max(1, L // 8), L // 3], [vb + 23] + [vb + 700 + 11 * i for i in range(5)], [(vb + 800, 5)]))
    # 2: the second child of R; its first extra lies below / inside / above R's first interval (a direct R has none: the same values)
    left, ln = iv_r[0] if iv_r else (vb + 10 + 9 * (NR // 3) + 2, 5)
    where = (g // 4) % 3
    if where == 0: blocks, first = [], left - 1
    elif where == 2: blocks, first = [], left + ln
    else:
        p0 = R.index(left) if left in R else 0
        blocks, first = ([p0, ln] if left in R else []), left + 2       # the interval's elements are skipped: the child's own residual lies among them
    recs.append(_node(lists, 2, blocks, [first], [(vb + 900, 4)]))
    # 3: c2 copies c1 (depth 2), 4: c3 copies c2 (depth 3), 5: a leaf behind the chain (so c3 is stored)
    recs.append(_node(lists, 2, [len(lists[-2]) // 4, 3], [vb + 14] + [vb + 1000 + 13 * i for i in range(4)], [(vb + 1100, 7)]))
    recs.append(_node(lists, 1, [], [vb + 41] + [vb + 1200 + 7 * i for i in range(3)], [(vb + 1300, 4)]))
    recs.append(_node(lists, 1, [], [], []))
    # 6: U, a d2 root whose copiers sit 4 and 6 nodes behind it
    res_u = [vb + 1400 + 8 * i for i in range(NU)]
    recs.append(_node(lists, 0, [], res_u, [(vb + 1400 + 8 * (NU // 3) + 2, 5)])); U = lists[-1]
    # 7: R is copied a second time, at distance W: a sub-row (or a super-row, or a block) later
    recs.append(_node(lists, 7, [L // 2], [vb + 1700], []))
    # 8: F, a long direct root; 9: a leaf of it
    recs.append(_node(lists, 0, [], [vb + 1800 + 5 * i for i in range(NF)], []))
    recs.append(_node(lists, 1, [], [vb + 2300], []))
    # 10: a stored child of U (level 0 next to R's chain), 11: its leaf, 12: U's last copier
    recs.append(_node(lists, 4, [len(U) // 3, 3], [vb + 1401], [(vb + 2400, 4)]))
    recs.append(_node(lists, 1, [], [], []))
    recs.append(_node(lists, 6, [], [], []))
    for j in range(nfill):                                            # (the sparse stream: short lists, every other one copied by the next)
        recs.append(_node(lists, 0, [], [vb + 2500 + 3 * j, vb + 2501 + 3 * j], []) if j % 2 == 0 else _node(lists, 1, [], [], []))


LONG = 420                # residuals of a long record: 7 bits each (gaps of 8 in zeta_3), so six of them hold more bits than the widest stream window
LONG_PER = 29             # records per long group (coprime with 64)


def _long_group(recs, lists, g, vb):
    """Y, a stored root (d2 for even g, direct for odd g); six LONG records that nobody copies; c, which copies Y at distance W and is copied by two leaves; short
    records without reference.  No stream window holds both Y's record and the head of c's (asserted on the offsets in the test), so c always lies in a later super-row
    than Y, Y's liveness is decided by what the kernel reads of c's record from memory, and no list that is BUILT in Y's sub-row copies from Y: the intervals of a d2 Y are
    filled by the extras pass of level 0, never by the pass in front of the levels.  (That the kernel then takes the 12 fetched bytes rather than giving up and keeping
    every list is not asserted, only argued: it gives up when the scratch area has cut the super-row shorter than the window did, and a super-row here holds at most a
    dozen copy blocks and interval entries against a scratch share of hundreds.)"""
    recs.append(_node(lists, 0, [], [vb + 10 + 9 * i for i in range(20)], [(vb + 10 + 9 * 7 + 2, 5)] if g % 2 == 0 else [])); Y = lists[-1]
    for j in range(6):
        recs.append(_node(lists, 0, [], [vb + 5 + j + 8 * i for i in range(LONG)], []))
    recs.append(_node(lists, 7, [len(Y) // 2, 2], [vb + 3], [(vb + 3400, 4)]))
    recs.append(_node(lists, 1, [], [vb + 1], []))
    recs.append(_node(lists, 2, [3], [], []))
    for j in range(LONG_PER - 10):
        recs.append(_node(lists, 0, [], [vb + 2 + j, vb + 40 + j, vb + 90 + j], []))


STREAMS = {"dense": dict(ngroups=540, NR=60, NU=36, NF=80, nfill=0), "sparse": dict(ngroups=330, NR=6, NU=6, NF=12, nfill=8), "long": dict(ngroups=145)}
_cache = {}


def _stream(name):
    if name not in _cache:
        s = STREAMS[name]
        per = LONG_PER if name == "long" else G + s["nfill"]
        n = s["ngroups"] * per
        recs, lists = [], []
        for g in range(s["ngroups"]):
            if name == "long": _long_group(recs, lists, g, min(g * per, n - 3500))
            else: _group(recs, lists, g, min(g * per, n - 2700), s["NR"], s["NU"], s["NF"], s["nfill"])
        gbytes, offs, expect = assemble(recs, max_ref=4)
        assert [list(l) for l in expect] == lists, "the hand-computed lists disagree with the restated iterators"
        assert 0 <= min(l[0] for l in lists if l) and max(l[-1] for l in lists if l) < n
        _cache[name] = (recs, np.frombuffer(gbytes, dtype=np.uint8), offs, lists, per)
    return _cache[name]


def _stored(recs):
    s = [False] * len(recs)
    for x, r in enumerate(recs):
        if r.ref: s[x - r.ref] = True
    return s


CASES = {
    "dense": ("dense", {}),
    "dense_pool512": ("dense", {"BVG_SCAN_POOL": "512"}),
    "dense_pool1024": ("dense", {"BVG_SCAN_POOL": "1024"}),
    "dense_no_d2": ("dense", {"BVG_NO_D2": "1"}),                         # a root with intervals is a `pure` member of level 0
    "sparse": ("sparse", {}),                                            # the 85-VGPR instantiation: no in-place decode around intervals either
    "sparse_16_waves": ("sparse", {"BVG_SCAN_WAVES": "16"}),             # the 128-VGPR instantiation on short records: the next super-row's references lie in the staged window
    "long": ("long", {}),                                                # the copier's record lies outside the staged window: its reference is read from memory
}


def _scan_geometry(err):
    m = re.findall(r"scan kernel: pool (\d+) \+ scratch (\d+) elements, window (\d+) dwords, (\d+) wavefronts per CU", err)
    assert m, err[-2000:]
    return tuple(int(v) for v in m[-1])


@pytest.mark.parametrize("case", sorted(CASES))
def test_levels_and_liveness_against_the_oracle(W, oracle, monkeypatch, capfd, case):
    name, env = CASES[case]
    recs, graph, offs, lists, per = _stream(name)
    n = len(recs)
    # the boundary cases need sub-rows: the stored lists of any 64 consecutive records -- a super-row holds at most 64 -- exceed the whole area (pool + scratch)
    if "BVG_SCAN_POOL" in env:
        st = _stored(recs)
        dsum = np.concatenate([[0], np.cumsum([r.d if st[x] else 0 for x, r in enumerate(recs)])])
        assert int((dsum[64:] - dsum[:-64]).min()) > int(env["BVG_SCAN_POOL"]) + SCR
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_MAT_LEAN", "1")
    p = W.default_params(max_ref_count=4).clone(nodes=n, arcs=int(sum(len(l) for l in lists)))
    assert p.window_size == W7 and p.min_interval_length == 4
    if name == "sparse":
        assert p.arcs / n <= 16.0                                      # (bvg_sched.hip lean_geometry: 24 wavefronts per CU for such graphs)
    og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), offs)
    hg = W.BVGraph.from_memory(p, graph, offs)
    o = og.scan()
    assert o["arcs"] == p.arcs
    r1 = hg.scan()                                                     # builds the index and validates the blocks
    capfd.readouterr()
    r2 = hg.scan()
    geo = _scan_geometry(capfd.readouterr().err)
    for r in (r1, r2):
        assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"])
    assert r2["lean_blocks"] > 0, "the lean scan kernel did not run"
    if "BVG_SCAN_POOL" in env: assert geo[:2] == (int(env["BVG_SCAN_POOL"]), SCR)
    if case == "sparse": assert geo[3] == 24, geo
    if case == "sparse_16_waves": assert geo[3] == 16, geo
    if name == "long":
        # no window that holds Y's record (it starts at or before it and is geo[2] dwords long) reaches the first 160 bits of c's record, which the kernel wants staged to
        # read a reference from the window: c is in a later super-row than Y, and Y is kept or dropped by the 12 bytes of c's record fetched from memory
        for y in range(0, n, per):
            assert recs[y + 7].ref == 7 and int(offs[y + 7]) + 160 > int(offs[y]) + 32 * geo[2], (y, geo)
    # node by node: four groups in a row (every kind of root, the chains that enter from the group before) at three places of the stream
    ngroups = n // per
    for g0 in (1, ngroups // 2 + 1, ngroups - 5)[:PLACES]:
        for y in range(g0 * per, (g0 + (2 if name == "long" else 4)) * per):
            ry, oy = hg.scan(y, y + 1), og.scan(y, y + 1)
            assert ry["lean_blocks"] > 0, (case, y)
            assert (ry["arcs"], ry["chk"]) == (len(lists[y]), oy["chk"]), (case, y)
    # the materialising form: every list, successor by successor
    odeg, osucc = og.decode_range(0, n)
    assert osucc.tolist() == [v for l in lists for v in l]
    capfd.readouterr()
    deg, succ = hg.decode_range(0, n)
    err = capfd.readouterr().err
    k = re.search(r"scan kernel (\d+) \+ (\d+)/(\d+)/(\d+)/(\d+) LDS-class", [l for l in err.splitlines() if "tiers concurrent" in l][-1])
    assert sum(int(v) for v in k.groups()) > 0, "the materialising call did not run the lean kernel"
    assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc), case
    hg.close()
