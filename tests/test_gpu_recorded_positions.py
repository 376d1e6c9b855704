"""GPU: the recorded positions of the lean scan kernel's extras (csrc/bvg_scan.hip), on hand-assembled records (tests/bvrecords.py).

Where an interval or a residual of a stored list goes in that list depends on the stream alone.  The skip index keeps one 16-bit entry per extra of every list that some
later node of the graph copies from; a block whose flag is clear searches for the positions as before (Z1, a pass per level) and writes them down, a block whose flag is
set places all extras of a sub-row in ONE pass in front of its levels.  Here every case scans four times -- the index build, the recording scan, the recorded scan (the
debug line must say that blocks ran recorded) and a scan with BVG_NO_POS=1 -- and then node by node, against the oracle.

Every group of 17 records (17 and 64 are coprime: over 250 groups every record is the last of a sub-row, of a super-row and of a block somewhere) holds
  0      R, a long root of residuals alone (decoded straight into place: a chain root that no level builds);
  1-3    a chain A <- B <- C below R (depth 1, 2, 3 inside one sub-row) whose members hold 0 / 1 / 2 residuals and 0 / 1 / 2 intervals, the nine pairs rotating with the group;
  4      a leaf that copies C;
  5      P, copied ONLY by record 12, seven records on: from the next sub-row, the next super-row or the next block (then P's entries lie in that block's halo);
  6      U, a root with intervals between its residuals (ref == 0: decoded in place where the instantiation can, else a member with entries for its intervals alone);
  7      a copier of U with many copy blocks (what fills the scratch area);
  8      X, a copier of U whose extras straddle the 64 lanes of a pass: 20 intervals and 38 + g % 12 residuals (58 ... 69 extras; with the few of its neighbours a
         sub-row holds exactly 63, 64 and 65 somewhere, and X's intervals end one pass while its residuals begin the next);
  9      a copier of X (X is stored), 10 a leaf with a reference, 11 a root nobody copies (no entries), 12 the copier of P,
  13-16  Y <- Z: Y holds 30 intervals and nothing else, Z copies it and adds 2 residuals below, between and above them; two leaves."""
import os
import re

import numpy as np
import pytest

from bvrecords import Record, assemble

pytestmark = pytest.mark.gpu

KNOBS = ("BVG_EMIT", "BVG_DBG", "BVG_NOSKIP", "BVG_SCANK", "BVG_SCAN_POOL", "BVG_SCAN_SCR", "BVG_SCAN_STAGE", "BVG_SCAN_WAVES", "BVG_NO_D2", "BVG_NO_POS", "BVG_DEBUG")
G = 17
NGROUPS = 250             # 4 250 nodes: a scan of 4 096 nodes and more builds the skip index and validates the blocks
SPAN = 2600               # values of a group lie in [vb, vb + SPAN)
M = 4                     # min_interval_length
CHECKED = (3, 131)[:int(os.environ.get("BVG_POS_PLACES", "2"))]   # first group of the runs of nine groups that are checked node by node (the emulated run, tests/test_emu_recorded_positions.py, takes one)


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


def _extras(v0, nr, ni, gap=9):
    """nr residuals and ni intervals of M elements from v0 on, alternating, `gap` apart"""
    res, ivs, v = [], [], v0
    for k in range(max(nr, ni)):
        if k < ni: ivs.append((v, M)); v += M + gap
        if k < nr: res.append(v); v += gap
    return res, ivs


def _group(recs, lists, g, vb):
    R_res = [vb + 3 * i for i in range(120)]                                # 0: R occupies vb + {0, 3, ...}: values = 1, 2 (mod 3) below vb + 360 are free
    recs.append(_node(lists, 0, [], R_res))
    free = vb + 1                                                           # free values of residue 1 (mod 3) inside R's span ...
    above = vb + 400                                                        # ... and everything above it
    for j in range(3):                                                      # 1-3: the chain, each member keeps most of the list above it
        nr, ni = divmod((g + 4 * j) % 9, 3)
        res = [free + 3 * (7 * j + i) + 30 for i in range(nr)]              # residuals between the copied elements
        ivs = [(above + 40 * j + 12 * i, M) for i in range(ni)]             # intervals above them
        up = lists[-1]
        recs.append(_node(lists, 1, [len(up) // 3, 2, len(up) // 4, 1], res, ivs))
    recs.append(_node(lists, 1, [5, 3], [vb + 600], []))                    # 4: a leaf below C
    recs.append(_node(lists, 5, [40, 10, 30], [vb + 2, vb + 605], [(vb + 610, M + 1)]))   # 5: P copies R; only record 12 copies P
    u_res, u_ivs = _extras(vb + 700, 12, 3)
    recs.append(_node(lists, 0, [], u_res, u_ivs)); U = lists[-1]           # 6: U
    recs.append(_node(lists, 1, [1, 1] * 9 + [2], [vb + 690], [(vb + 900, M)]))           # 7: 19 copy blocks
    nx = 38 + g % 12                                                        # 8: X
    x_res = [vb + 2 + 3 * i for i in range(1, nx + 1)]                      # (residue 2 (mod 3): between R's elements; X keeps all of U)
    x_ivs = [(vb + 1000 + 9 * i, M) for i in range(20)]
    recs.append(_node(lists, 2, [], x_res, x_ivs)); X = lists[-1]
    recs.append(_node(lists, 1, [len(X) // 2, 7], [vb + 1300], []))         # 9: copies X
    recs.append(_node(lists, 4, [3], [vb + 1310, vb + 1313], [(vb + 1320, M)]))   # 10: a leaf that copies U
    recs.append(_node(lists, 0, [], [vb + 1400 + 5 * i for i in range(9)], [(vb + 1460, 6)]))   # 11: a root nobody copies
    recs.append(_node(lists, 7, [4, 2, 20], [vb + 1500], []))               # 12: the only copier of P
    recs.append(_node(lists, 0, [], [], [(vb + 1600 + 11 * i, M + i % 3) for i in range(30)])); Y = lists[-1]   # 13: Y, thirty intervals
    recs.append(_node(lists, 1, [], [vb + 1590, vb + 1600 + 11 * 15 - 2, vb + 2000][:2 + g % 2], []))      # 14: Z copies all of Y: residuals below / between (/ above) its elements
    recs.append(_node(lists, 1, [len(Y) // 2], [], [(vb + 2100, M)]))       # 15: a leaf below Z
    recs.append(_node(lists, 2, [0, 10], [vb + 2200], []))                  # 16: a leaf that copies Z


_cache = {}


def _stream():
    if not _cache:
        n = NGROUPS * G
        recs, lists = [], []
        for g in range(NGROUPS):
            _group(recs, lists, g, min(g * G, n - SPAN))
        gbytes, offs, expect = assemble(recs, min_interval=M, max_ref=4)
        assert [list(l) for l in expect] == lists, "the hand-computed lists disagree with the restated iterators"
        assert 0 <= min(l[0] for l in lists if l) and max(l[-1] for l in lists if l) < n
        _cache[0] = (recs, np.frombuffer(gbytes, dtype=np.uint8), offs, lists)
    return _cache[0]


_oracle = {}


def _open(W, oracle, wide=False, no_index=False):
    recs, graph, offs, lists = _stream()
    n = len(recs)
    p = W.default_params(max_ref_count=4, min_interval_length=M).clone(nodes=n, arcs=int(sum(len(l) for l in lists)))
    assert p.window_size == 7 and p.arcs / n > 48.0                     # (bvg_sched.hip lean_geometry: the dense instantiations unless BVG_SCAN_WAVES says otherwise)
    if not _oracle:                                                     # the reference answers, computed once and shared by every case
        og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), offs)
        _oracle["all"] = og.scan()
        _oracle["node"] = {y: og.scan(y, y + 1) for g0 in CHECKED for y in range(g0 * G, (g0 + 9) * G)}
    hg = W.BVGraph.from_memory(p, graph, offs)
    if wide or no_index: hg.set_tuning(force_wide=wide, no_index=no_index)
    return hg, n, lists


def _same(r, o):
    return (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"])


def _positions(err):
    """(blocks that ran recorded, blocks that were recording) of the last scan, from its debug line"""
    m = re.findall(r"positions: (\d+) blocks recorded, (\d+) recording", err)
    assert m, err[-2000:]
    return int(m[-1][0]), int(m[-1][1])


def _nodes(hg, lists, places=CHECKED):
    for g0 in places:
        for y in range(g0 * G, (g0 + 9) * G):
            ry, oy = hg.scan(y, y + 1), _oracle["node"][y]
            assert ry["lean_blocks"] > 0, y
            assert (ry["arcs"], ry["chk"]) == (len(lists[y]), oy["chk"]), y


# (environment, force_wide)
CASES = {
    "pool1024": ({"BVG_SCAN_POOL": "1024"}, False),
    "pool640": ({"BVG_SCAN_POOL": "640"}, False),                                          # X and the lists around it barely share a sub-row
    "scr_small": ({"BVG_SCAN_POOL": "1024", "BVG_SCAN_SCR": "16", "BVG_SCAN_STAGE": "384"}, False),                 # super-rows cut short by the scratch area: lists stored that nobody copies
    "no_d2": ({"BVG_SCAN_POOL": "1024", "BVG_NO_D2": "1"}, False),                         # U and Y are members of level 0, with entries for their intervals
    "waves24": ({"BVG_SCAN_POOL": "1024", "BVG_SCAN_WAVES": "24"}, False),                 # the 85-VGPR instantiation: no in-place decode around intervals either
    "waves18": ({"BVG_SCAN_POOL": "1024", "BVG_SCAN_WAVES": "18"}, False),                 # the 96-VGPR instantiation
    "wide": ({"BVG_SCAN_POOL": "1024"}, True),                                             # the 64-bit-id path: ids relative to the block's base, an index of its own width
}


def _super_rows(err):
    return int(re.findall(r"scan kernel rows: (\d+) super-rows", err)[-1])


@pytest.mark.parametrize("case", sorted(CASES))
def test_recording_recorded_and_searched_scans_equal_the_oracle(W, oracle, monkeypatch, capfd, case):
    env, wide = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_DBG", "64")
    hg, n, lists = _open(W, oracle, wide=wide)
    o = _oracle["all"]
    assert _same(hg.scan(), o)                                          # builds the index (the checking kernels) and counts the entries
    capfd.readouterr()
    r_rec = hg.scan()                                                   # every block searches for its positions and writes them down
    e_rec = capfd.readouterr().err
    r_use = hg.scan()                                                   # ... and reads them back
    e_use = capfd.readouterr().err
    assert _same(r_rec, o) and _same(r_use, o), case
    assert r_use["lean_blocks"] > 0
    # (a block that overflows the pool of tier 0 leaves for an LDS class on the next scan and records there: the counts need not add up to lean_blocks)
    used, recording = _positions(e_rec)
    assert used == 0 and 0 < recording <= r_rec["lean_blocks"], e_rec[-1500:]
    used, recording = _positions(e_use)
    assert used > 0 and used >= 4 * recording and used + recording <= r_use["lean_blocks"], e_use[-1500:]   # (the test cannot pass on the old path alone)
    geo = re.findall(r"scan kernel: pool (\d+) \+ scratch (\d+) elements, window (\d+) dwords, (\d+) wavefronts per CU", e_use)
    assert geo and int(geo[-1][0]) == int(env["BVG_SCAN_POOL"]) and ("BVG_SCAN_WAVES" not in env or int(geo[-1][3]) == int(env["BVG_SCAN_WAVES"])), geo
    if case == "scr_small":                                             # the scratch area did cut super-rows short: more of them than with the default area and the same window
        monkeypatch.setenv("BVG_SCAN_SCR", "448")
        assert _same(hg.scan(), o)
        e_big = capfd.readouterr().err
        assert _super_rows(e_use) > _super_rows(e_big), (e_use[-600:], e_big[-600:])
        monkeypatch.setenv("BVG_SCAN_SCR", "16")
    _nodes(hg, lists)
    monkeypatch.setenv("BVG_NO_POS", "1")
    r_old = hg.scan()
    e_old = capfd.readouterr().err
    assert _same(r_old, o) and r_old["lean_blocks"] > 0 and _positions(e_old) == (0, 0), e_old[-1500:]
    _nodes(hg, lists, CHECKED[:1])
    hg.close()
    # the recording scan itself, node by node: a second handle whose blocks are recorded by the one-node scans that touch them first
    monkeypatch.delenv("BVG_NO_POS")
    hb, _, _ = _open(W, oracle, wide=wide)
    assert _same(hb.scan(), o)
    capfd.readouterr()
    _nodes(hb, lists)
    seen = re.findall(r"positions: (\d+) blocks recorded, (\d+) recording", capfd.readouterr().err)
    assert any(int(b) for a, b in seen) and any(int(a) for a, b in seen), seen[:8]
    hb.close()


def test_node_by_node_scans_record_their_blocks(W, oracle, monkeypatch, capfd):
    """A scan of one node decodes its whole block: the first one that touches a block records it, the others read its entries."""
    monkeypatch.setenv("BVG_SCAN_POOL", "1024"); monkeypatch.setenv("BVG_DEBUG", "1")
    hg, n, lists = _open(W, oracle)
    assert _same(hg.scan(), _oracle["all"])
    capfd.readouterr()
    _nodes(hg, lists)
    err = capfd.readouterr().err
    seen = re.findall(r"positions: (\d+) blocks recorded, (\d+) recording", err)
    assert any(int(b) for a, b in seen) and any(int(a) for a, b in seen), seen[:8]
    assert _same(hg.scan(), _oracle["all"])
    hg.close()


def test_entries_do_not_depend_on_the_geometry(W, oracle, monkeypatch, capfd):
    """Recorded under one pool, read under another: the two cut the sub-rows differently, the entries are addressed by node order alone."""
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_SCAN_POOL", "1024")
    hg, n, lists = _open(W, oracle)
    o = _oracle["all"]
    assert _same(hg.scan(), o) and _same(hg.scan(), o)                  # the build, the recording scan
    monkeypatch.setenv("BVG_SCAN_POOL", "640")
    capfd.readouterr()
    r = hg.scan()
    err = capfd.readouterr().err
    assert _same(r, o) and _positions(err)[0] > 0, err[-1500:]
    assert "pool 640" in err
    _nodes(hg, lists)
    monkeypatch.setenv("BVG_SCAN_POOL", "1024"); monkeypatch.setenv("BVG_NO_D2", "1")   # an instantiation that needs U's and Y's entries too: it records them first
    capfd.readouterr()
    r1 = hg.scan(); e1 = capfd.readouterr().err
    r2 = hg.scan(); e2 = capfd.readouterr().err
    assert _same(r1, o) and _same(r2, o)
    assert _positions(e1)[0] == 0 and _positions(e1)[1] > 0 and _positions(e2)[0] > 0, (e1[-800:], e2[-800:])
    hg.close()


def test_handles_that_share_the_index(W, oracle, monkeypatch, capfd):
    """A copy() flyweight reads what its origin recorded; a marks-only handle (no_index = 2) has no entries and keeps the searches."""
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_SCAN_POOL", "1024")
    hg, n, lists = _open(W, oracle)
    o = _oracle["all"]
    assert _same(hg.scan(), o) and _same(hg.scan(), o)
    fl = hg.copy()
    capfd.readouterr()
    r = fl.scan()
    err = capfd.readouterr().err
    assert _same(r, o) and _positions(err)[0] > 0 and _positions(err)[1] == 0, err[-1500:]
    _nodes(fl, lists, CHECKED[:1])
    fl.close(); hg.close()
    mg, _, _ = _open(W, oracle, no_index=2)
    for _ in range(3):
        capfd.readouterr()
        r = mg.scan()
        assert _same(r, o)
    assert r["lean_blocks"] > 0 and _positions(capfd.readouterr().err) == (0, 0)
    _nodes(mg, lists, CHECKED[:1])
    mg.close()


def test_entries_recorded_under_a_large_scratch_area_serve_a_small_one(W, oracle, monkeypatch, capfd):
    """The other direction of `scr_small`: recorded with full super-rows, read with super-rows cut short.  A list that was a leaf in the recording scan (nobody of its
    block copies from it) may be stored in the reading one (the peek at the next super-row unknown): its entries were never written, read 0xFFFF, and it keeps Z1."""
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_DBG", "64"); monkeypatch.setenv("BVG_SCAN_POOL", "1024")
    monkeypatch.setenv("BVG_SCAN_SCR", "1024"); monkeypatch.setenv("BVG_SCAN_STAGE", "1024")
    hg, n, lists = _open(W, oracle)
    o = _oracle["all"]
    assert _same(hg.scan(), o) and _same(hg.scan(), o)                  # the build, the recording scan
    e_big = capfd.readouterr().err
    for scr, stage in (("16", "1024"), ("16", "128"), ("448", "128"), ("64", "256")):
        monkeypatch.setenv("BVG_SCAN_SCR", scr); monkeypatch.setenv("BVG_SCAN_STAGE", stage)
        r = hg.scan()
        err = capfd.readouterr().err
        assert _same(r, o) and _positions(err)[0] > 0 and _positions(err)[1] == 0, (scr, stage, err[-1500:])
        assert _super_rows(err) > _super_rows(e_big), (scr, stage)
    _nodes(hg, lists)
    hg.close()


def test_a_loaded_index_records_on_its_first_scan(W, oracle, monkeypatch, capfd, tmp_path):
    """The entries are not in basename.bvgidx: loading counts them again, the first scan of the loaded index records, the second reads them back."""
    monkeypatch.setenv("BVG_DEBUG", "1"); monkeypatch.setenv("BVG_SCAN_POOL", "1024")
    hg, n, lists = _open(W, oracle)
    o = _oracle["all"]
    assert _same(hg.scan(), o)
    path = hg.save_index(str(tmp_path / "recorded.bvgidx"))
    hg.close()
    hl, _, _ = _open(W, oracle)
    hl.load_index(path)
    capfd.readouterr()
    r1 = hl.scan(); e1 = capfd.readouterr().err
    r2 = hl.scan(); e2 = capfd.readouterr().err
    assert _same(r1, o) and _same(r2, o) and r1["lean_blocks"] > 0
    assert "residual skip index:" not in e1, "the loaded index was rebuilt"
    assert _positions(e1)[0] == 0 and _positions(e1)[1] > 0 and _positions(e2)[0] > 0 and _positions(e2)[1] == 0, (e1[-800:], e2[-800:])
    _nodes(hl, lists, CHECKED[:1])
    hl.close()
