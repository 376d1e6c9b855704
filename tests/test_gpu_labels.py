"""The arc-label decoder (csrc/bvg_labels.hip: four label classes, three kernels, five decode entry points, a file loader) against the plain
model of tests/labels_model.py, bit for bit, by the one rule of tests/label_cases.py: the device returns 0 exactly when the model decodes,
and then the arrays are equal; otherwise the open or the decode returns the documented error and nothing is handed out.

  * every width of every class (gamma; FixedWidthIntLabel and FixedWidthIntListLabel 0..32; FixedWidthLongListLabel 0..64) over graphs of
    1, 255, 256, 257 and 513 nodes and four value patterns; node and arc counts on both sides of each level of the shared prefix sum;
  * streams that end on the last bit of the file, for nbytes = 0, 1, 15 (mod 16), every start alignment, and the empty stream;
  * every range with both ends in {0, 1, 255, 256, 257, n - 1, n} through the host calls, the list calls and the _dev call, and a handle
    whose workspace grows (large, small, larger);
  * the capacity contract, the argument errors, the wrong entry point for the handle's kind;
  * every defect of label_cases: truncations, bit flips, degrees off by one, offsets swapped or past the file, an all-zero stream, and
    hand-assembled codes no label class writes.  A gamma-coded label or list length of 2^31 or more is REFUSED (BVG_E_EOF): the reference's
    readGamma() would wrap it to a negative int (the CPU oracle does), and a negative label handed on silently is worse than an error;
  * BitStreamArcLabelledImmutableGraph.load for all four classes and the ways a label graph on disk can be wrong.

No case is skipped or exempted; what is checked by other means than equal values is named in tests/label_cases.py.  Every defect case ran
on the host emulator (tests/test_emu.py) before it was sent to a GPU.

The _dev test runs in a fresh child process (this file as a script) that imports torch BEFORE the product library, like
tests/test_gpu_device_buffers.py; on the emulated library, whose device memory is host memory, the buffers are numpy arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import label_cases as LC
import labels_model as M
from label_cases import FIXED, GAMMA, LIST, LONG_LIST

pytestmark = pytest.mark.gpu

KINDS = (GAMMA, FIXED, LIST, LONG_LIST)
_ids = lambda k: LC.KIND_NAMES[k] if k in LC.KIND_NAMES else str(k)


def range_graph(kind, n=513):
    width = {GAMMA: 0, FIXED: 19, LIST: 9, LONG_LIST: 53}[kind]
    rng = np.random.default_rng([5, kind, n])
    return LC.make("%s-ranges-n%d" % (LC.KIND_NAMES[kind], n), kind, width, LC.degrees(n, rng, big=300), "random", rng, lead=5)


def all_ranges(n):
    ends = sorted({0, 1, 255, 256, 257, n - 1, n})
    return [(a, b) for a in ends for b in ends if a <= b]


@pytest.mark.parametrize("pattern", LC.PATTERNS)
@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_parameter_space(W, kind, pattern):
    cases = 0
    for case in LC.sweep_cases(kind, pattern):
        assert LC.check_parity(W, case) == ["ok"], case
        cases += 1
    assert cases == len(LC.widths(kind)) * len(LC.SIZES)


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_counts_around_the_levels_of_the_prefix_sum(W, kind):
    """label_cases.SCAN_BOUNDARIES: 1024 | 1025 and 65536 | 65537 nodes (scalar classes) or arcs (list classes).  The 65537-node graphs are the one
    place where these tests leave `a few thousand nodes`: the second level of the scan starts there and nowhere below."""
    for case in LC.scan_cases(kind):
        assert LC.check_parity(W, case) == ["ok"], case


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_end_of_stream(W, kind):
    """peek_global loads nine bytes from the position's byte, clamped to the last 16 bytes of the padded copy: the last run of these streams ends on the
    last bit of the file, is read alone and with the rest, and ends in a label of all ones."""
    starts, mods = set(), set()
    for case in LC.end_of_stream_cases(kind):
        seen = LC.check_parity(W, case, ranges=[(0, case.n), (case.n - 1, case.n), (case.n - 2, case.n)])
        if "empty-stream-with-arcs" in case.name:
            want = "ok" if kind == FIXED and case.width == 0 else "overrun"     # labels of no bits can be read from no bytes
            assert seen == [want, "ok", want], (case, seen)
        else:
            assert seen == ["ok"] * 3, (case, seen)
        if case.stream:
            mods.add(len(case.stream) % 16)
            starts.update(int(o) % 8 for o, d in zip(case.offsets[:-1], case.deg) if d > 0)
    assert mods == {0, 1, 15} and starts == set(range(8)), (mods, starts)


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_ranges_on_one_handle(W, kind):
    """Every (from, to) around the 256-thread block on the 513-node graph, through the host entry point of the class, on ONE handle; first large, small,
    larger, so that the workspace of the scalar calls (d_cum: to - from + 1 words) grows while it is in use."""
    case = range_graph(kind)
    seen = LC.check_parity(W, case, ranges=[(1, 257), (255, 256), (0, 513)] + all_ranges(case.n))
    assert seen == ["ok"] * len(seen) and len(seen) == 3 + 28


@pytest.mark.parametrize("kind", (GAMMA, FIXED), ids=_ids)
def test_workspace_reuse_across_scan_sizes(W, kind):
    """d_tmp holds one word per 1024 nodes (+ 1): ranges of 1000, 1 and 2500 nodes on one handle, then back down."""
    rng = np.random.default_rng([6, kind])
    case = LC.make("%s-reuse" % LC.KIND_NAMES[kind], kind, 7 if kind == FIXED else 0, LC.degrees(2500, rng, big=300), "random", rng)
    seen = LC.check_parity(W, case, ranges=[(0, 1000), (5, 6), (0, 2500), (1024, 1025), (1, 2499), (2500, 2500)])
    assert seen == ["ok"] * 6


def _call(W, h, case, frm, to, deg, out, cap, need, loff=None):
    """The host entry point of the case's class with raw pointers (None = NULL)."""
    L = W.lib()
    p = lambda a: None if a is None else a.ctypes.data
    if case.kind in (GAMMA, FIXED):
        return L.bvg_labels_decode_range(h, frm, to, p(deg), p(out), cap, None if need is None else C.byref(need))
    fn = L.bvg_labels_decode_range_lists if case.kind == LIST else L.bvg_labels_decode_range_lists64
    return fn(h, frm, to, p(deg), p(loff), p(out), cap, None if need is None else C.byref(need))


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_capacity_contract(W, kind):
    """cap = total - 1 and a NULL buffer: BVG_E_CAPACITY, *n set, the scalar output untouched, list_off filled for the list calls (so that the caller can
    size the values and call again)."""
    case = range_graph(kind)
    dt = np.int64 if kind == LONG_LIST else np.int32
    r, h = LC.open_case(W, case)
    assert r == 0
    try:
        for frm, to in ((0, case.n), (170, 172), (240, 256)):
            model = M.decode(kind, case.width, case.stream, case.offsets, frm, to, case.deg[frm:to])
            assert model.ok and model.total > 1
            deg = np.ascontiguousarray(case.deg[frm:to]); arcs = int(deg.sum())
            for out, cap in ((LC._filled(model.total, dt), model.total - 1), (None, model.total), (None, 0), (LC._filled(model.total, dt), 0)):
                need = C.c_uint64(0)
                loff = np.full(arcs + 1, LC.SENT64, dtype=np.uint64)
                assert _call(W, h, case, frm, to, deg, out, cap, need, loff) == W.E_CAPACITY and need.value == model.total, (frm, to, cap)
                assert out is None or LC._is_sentinel(out), "E_CAPACITY wrote into the output"
                if kind in (LIST, LONG_LIST):
                    assert np.array_equal(loff, model.list_off), "list_off is filled either way"
            # n may be NULL
            out = LC._filled(model.total, dt); loff = np.zeros(arcs + 1, dtype=np.uint64)
            assert _call(W, h, case, frm, to, deg, out, model.total, None, loff) == 0
            assert np.array_equal(out[:model.total], model.labels if model.labels is not None else model.values) and LC._is_sentinel(out[model.total:])
    finally:
        W.lib().bvg_labels_close(h)


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_argument_errors(W, kind):
    case = range_graph(kind)
    n = case.n
    dt = np.int64 if kind == LONG_LIST else np.int32
    r, h = LC.open_case(W, case)
    assert r == 0
    try:
        arcs = int(case.deg.sum())
        for what, frm, to, deg in (("from < 0", -1, 5, case.deg), ("to > nodes", 0, n + 1, case.deg), ("to < from", 7, 6, case.deg), ("null outdeg", 0, n, None),
                                   ("negative outdegree", 0, n, np.where(np.arange(n) == 300, -1, case.deg).astype(np.int32)),
                                   ("negative outdegree at the end", 0, n, np.where(np.arange(n) == n - 1, -7, case.deg).astype(np.int32))):
            out, loff, need = LC._filled(arcs + 8, dt), np.full(arcs + 9, LC.SENT64, dtype=np.uint64), C.c_uint64(0)
            assert _call(W, h, case, frm, to, deg, out, arcs + 8, need, loff) == W.E_ARG, what
            assert LC._is_sentinel(out), what
        if kind in (LIST, LONG_LIST):
            assert _call(W, h, case, 0, n, case.deg, LC._filled(8, dt), 8, C.c_uint64(0), None) == W.E_ARG          # no list_off
        need = C.c_uint64(9)
        assert _call(W, h, case, 5, 5, None, None, 0, need, np.zeros(1, np.uint64)) == 0 and need.value == 0          # an empty range needs no outdegrees
    finally:
        W.lib().bvg_labels_close(h)
    assert _call(W, None, case, 0, 1, case.deg, LC._filled(8, dt), 8, C.c_uint64(0), np.zeros(9, np.uint64)) == W.E_ARG   # no handle


def test_wrong_entry_point_for_the_kind(W):
    L = W.lib()
    for kind in KINDS:
        case = range_graph(kind)
        r, h = LC.open_case(W, case)
        assert r == 0
        try:
            arcs = int(case.deg.sum())
            for name, fn, dt, lists in (("host", L.bvg_labels_decode_range, np.int32, False), ("dev", L.bvg_labels_decode_range_dev, np.int32, False),
                                        ("lists", L.bvg_labels_decode_range_lists, np.int32, True), ("lists64", L.bvg_labels_decode_range_lists64, np.int64, True)):
                right = {GAMMA: ("host", "dev"), FIXED: ("host", "dev"), LIST: ("lists",), LONG_LIST: ("lists64",)}[kind]
                if name in right:
                    continue
                out, loff, need = LC._filled(arcs, dt), np.full(arcs + 1, LC.SENT64, dtype=np.uint64), C.c_uint64(0)
                if name == "dev" and not _device_memory_is_host_memory(W):
                    continue                                                   # (device pointers: the child process of test_dev_entry_point asks this)
                args = (h, 0, case.n, case.deg.ctypes.data) + ((loff.ctypes.data,) if lists else ()) + (out.ctypes.data, arcs, C.byref(need))
                assert fn(*args) == W.E_UNSUPPORTED, (LC.KIND_NAMES[kind], name)
                assert LC._is_sentinel(out), (LC.KIND_NAMES[kind], name)
        finally:
            L.bvg_labels_close(h)
    st = np.zeros(4, np.uint8); lo = np.zeros(2, np.uint64); h = C.c_void_p()
    assert L.bvg_labels_open_mem(5, 8, 1, st.ctypes.data, 4, lo.ctypes.data, 0, C.byref(h)) == W.E_UNSUPPORTED and not h.value
    for kind, width in ((FIXED, 33), (FIXED, -1), (LIST, 33), (LONG_LIST, 65)):
        assert L.bvg_labels_open_mem(kind, width, 1, st.ctypes.data, 4, lo.ctypes.data, 0, C.byref(h)) == W.E_ARG and not h.value


FLIPS_PER_BASE = 12


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_status_parity_on_every_defect(W, kind):
    """Every defect generator of label_cases on every base stream of the class, and FLIPS_PER_BASE seeded single-bit flips; then every range of three
    nodes around the longest node of the damaged stream."""
    tally = {}
    for base in LC.defect_bases(kind):
        assert LC.check_parity(W, base) == ["ok"]
        rng = np.random.default_rng([7, kind, base.width])
        x = int(np.argmax(base.deg))
        for name in LC.defect_names(base) + ["flip"] * FLIPS_PER_BASE:
            case = LC.apply_defect(base, name, rng)
            seen = LC.check_parity(W, case, ranges=[(0, case.n), (x - 1, x + 2), (x, x + 1), (0, x), (x + 1, case.n)])
            for s in ([seen] if isinstance(seen, str) else seen):
                tally[s] = tally.get(s, 0) + 1
    # the bases refuse in every way there is (labels of width 0 alone cannot overrun or come up short: the fixed_int bases have other widths too)
    for s in ("ok", "open:past_file", "open:non_monotone", "overrun", "short"):
        assert tally.get(s), (s, tally)


def test_hand_assembled_codes(W):
    """Codes no label class writes.  The gamma_range decision, pinned: 2^31 - 1 decodes; 2^31, 2^32 - 1 and a list length of 2^31 or more are refused."""
    want = {"gamma-2^31-1-decodes": "ok", "gamma-2^31-refused": "gamma_range", "gamma-2^32-1-refused": "gamma_range", "gamma-2^32-refused": "gamma_range",
            "gamma-2^63-refused": "gamma_range", "gamma-2^64-2-refused": "gamma_range", "gamma-64-zeros-then-a-code": "gamma_range",
            "gamma-70-zeros-run-too-short": "overrun", "gamma-200-zeros": "overrun"}
    pinned = 0
    for case in LC.hand_cases():
        seen = LC.check_parity(W, case, ranges=[(0, case.n)] + [(x, x + 1) for x in range(case.n)])
        if case.name in want:
            assert seen[0] == want[case.name] and seen[1:] == ["ok", want[case.name], "ok"], (case, seen); pinned += 1
        elif case.name.endswith("len-2^31-1-no-elements") or case.name.endswith("len-2^31-2-one-element"):
            assert seen[0] == "overrun", (case, seen); pinned += 1
        elif case.name.endswith("w0-len-2^31-1-decodes"):
            assert seen[0] == "ok", (case, seen); pinned += 1
        else:
            assert "len-2^" in case.name and seen[0] == "gamma_range", (case, seen); pinned += 1
    assert pinned == 9 + 4 * 5 + 2 * 2


# ---- files ----
def _graph_on_disk(tools, tmp_path, n=300):
    rng = np.random.default_rng(8)
    deg = LC.degrees(n, rng, big=120)
    lists = [sorted(int(v) for v in rng.choice(n, size=d, replace=False)) for d in deg]
    st = tools.store(lists)
    st.write(str(tmp_path / "under"))
    arc_off = np.zeros(n + 1, dtype=np.uint64); arc_off[1:] = np.cumsum(deg)
    return deg, np.concatenate([np.array(l, dtype=np.int64) for l in lists]), arc_off, rng


def _stored_labels(tools, kind, width, arc_off, rng):
    """(StoredLabels by the tooling writer, the same stream as a Case for the model)"""
    deg = [int(d) for d in np.diff(arc_off.astype(np.int64))]
    case = LC.make("file-%s" % LC.KIND_NAMES[kind], kind, width, deg, "random", rng)
    model = M.decode(kind, width, case.stream, case.offsets, 0, case.n, case.deg)
    if kind in (GAMMA, FIXED):
        sl = tools.store_labels(kind, width, model.labels, arc_off)
    elif kind == LIST:
        sl = tools.store_label_lists(width, model.list_off, model.values, arc_off)
    else:
        sl = tools.store_label_long_lists(width, model.list_off, model.values, arc_off)
    assert sl.stream.tobytes() == case.stream and np.array_equal(sl.offsets, case.offsets)      # two writers, one stream
    return sl, model


@pytest.mark.parametrize("kind,width", [(GAMMA, 0), (FIXED, 23), (LIST, 11), (LONG_LIST, 47)], ids=lambda v: str(v))
def test_labelled_graphs_from_files(W, tools, tmp_path, kind, width):
    """BitStreamArcLabelledImmutableGraph.load for every class: .labeloffsets through bvg_labels_open, .properties with a relative and an absolute
    underlyinggraph, the class named with the standard package."""
    deg, succ, arc_off, rng = _graph_on_disk(tools, tmp_path)
    sl, model = _stored_labels(tools, kind, width, arc_off, rng)
    n = len(deg)
    for variant, under in (("relative", "under"), ("absolute", str(tmp_path / "under")), ("standard-package", "under")):
        base = str(tmp_path / ("lab-" + variant))
        sl.write(base, under)
        assert sl.spec().startswith("it.unimi.dsi.big.webgraph.labelling.")
        if variant == "standard-package":
            with open(base + ".properties", "w") as f:
                f.write("labelspec=%s\nunderlyinggraph=%s\n" % (sl.spec().replace("it.unimi.dsi.big.webgraph.", "it.unimi.dsi.webgraph."), under))
        lg = W.BitStreamArcLabelledImmutableGraph.load(base)
        try:
            if kind in (GAMMA, FIXED):
                d, s, lab = lg.decode_range(0, n)
                assert np.array_equal(lab, model.labels), variant
                a, b = int(arc_off[100]), int(arc_off[102])
                assert np.array_equal(lg.decode_range(100, 102)[2], model.labels[a:b]), variant
            else:
                d, s, lo, lv = lg.decode_range_lists(0, n)
                assert lv.dtype == (np.int64 if kind == LONG_LIST else np.int32)
                assert np.array_equal(lo, model.list_off) and np.array_equal(lv, model.values), variant
            assert np.array_equal(d, deg) and np.array_equal(s, succ), variant
        finally:
            lg.close(); lg.g.close()


def test_label_files_that_are_wrong(W, tools, tmp_path):
    deg, succ, arc_off, rng = _graph_on_disk(tools, tmp_path)
    sl, model = _stored_labels(tools, FIXED, 9, arc_off, rng)
    n, L = len(deg), W.lib()

    def status(base):
        h = C.c_void_p(); buf = C.create_string_buffer(4096)
        r = L.bvg_labels_open(os.fsencode(base), n, 0, C.byref(h), buf, len(buf))
        assert (r == 0) == bool(h.value)
        if h.value:
            L.bvg_labels_close(h)
        return r

    good = str(tmp_path / "good"); sl.write(good, "under")
    assert status(good) == 0
    # no labelspec
    base = str(tmp_path / "nospec"); sl.write(base, "under")
    with open(base + ".properties", "w") as f:
        f.write("graphclass = it.unimi.dsi.big.webgraph.labelling.BitStreamArcLabelledImmutableGraph\nunderlyinggraph = under\n")
    assert status(base) == W.E_IO
    with pytest.raises(W.IOException):
        W.BitStreamArcLabelledImmutableGraph.load(base)
    # a user's label class
    base = str(tmp_path / "userclass"); sl.write(base, "under")
    with open(base + ".properties", "w") as f:
        f.write("underlyinggraph = under\nlabelspec = org.example.MyOwnLabel(FOO,9)\n")
    assert status(base) == W.E_UNSUPPORTED
    with pytest.raises(W.UnsupportedOperationException):
        W.BitStreamArcLabelledImmutableGraph.load(base)
    # .labeloffsets with fewer than nodes + 1 entries: the status bvg_decode_offsets gives for those bytes
    full = tools.encode_offsets(sl.offsets, 2).tobytes()
    for cut in (len(full) // 2, len(full) - 1, 0):
        base = str(tmp_path / ("shortoffsets%d" % cut)); sl.write(base, "under")
        with open(base + ".labeloffsets", "wb") as f:
            f.write(full[:cut])
        buf = np.frombuffer(full[:cut], dtype=np.uint8); out = np.zeros(n + 1, dtype=np.uint64)
        want = L.bvg_decode_offsets(buf.ctypes.data if len(buf) else None, len(buf), n, 2, out.ctypes.data)
        assert want != 0 and status(base) == want, (cut, want)
    # no .labels / no .labeloffsets / no .properties
    for ext in (".labels", ".labeloffsets", ".properties"):
        base = str(tmp_path / ("missing" + ext[1:])); sl.write(base, "under")
        os.remove(base + ext)
        assert status(base) == W.E_IO, ext
    # a .labels file that is shorter than its offsets say
    base = str(tmp_path / "shortlabels"); sl.write(base, "under")
    with open(base + ".labels", "wb") as f:
        f.write(sl.stream.tobytes()[:-9])
    assert status(base) == W.E_EOF


# ---- bvg_labels_decode_range_dev ----
def _device_memory_is_host_memory(W):
    return hasattr(W.lib(), "emu_fail_next_mallocs")                            # the emulated library (tests/emu)


class TorchMemory:
    def __init__(self, torch):
        self.torch = torch

    def put(self, a):
        t = self.torch.from_numpy(a.copy()).cuda()
        self.torch.cuda.synchronize()
        return t

    def ptr(self, t):
        return t.data_ptr()

    def get(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()


def _dev_entry_point(W, mem):
    """bvg_labels_decode_range_dev with `mem`'s buffers: every range on one handle (large, small, larger first), the capacity contract with the guard
    behind the capacity, the refusals, the list kinds."""
    L = W.lib()
    for kind in (GAMMA, FIXED):
        case = range_graph(kind)
        seen = LC.check_parity(W, case, ranges=[(1, 257), (255, 256), (0, 513)] + all_ranges(case.n), mem=mem, what="dev")
        assert seen == ["ok"] * len(seen)
        refused = [LC.check_parity(W, LC.apply_defect(case, name), mem=mem, what="dev")[0] for name in ("deg+1-longest", "deg-1-first", "trunc9-clamped", "all_zero")]
        assert refused[:2] == ["overrun", "short"], refused
        r, h = LC.open_case(W, case)
        assert r == 0
        total = int(case.deg.sum())
        d_deg = mem.put(case.deg)
        for cap, null in ((total - 1, False), (total, True), (0, False)):
            d_out = mem.put(LC._filled(total, np.int32)); need = C.c_uint64(0)
            assert L.bvg_labels_decode_range_dev(h, 0, case.n, mem.ptr(d_deg), None if null else mem.ptr(d_out), cap, C.byref(need)) == W.E_CAPACITY and need.value == total
            assert LC._is_sentinel(mem.get(d_out)), "E_CAPACITY wrote labels"
        need = C.c_uint64(0)
        assert L.bvg_labels_decode_range_dev(h, -1, 3, mem.ptr(d_deg), None, 0, C.byref(need)) == W.E_ARG
        assert L.bvg_labels_decode_range_dev(h, 0, case.n + 1, mem.ptr(d_deg), None, 0, C.byref(need)) == W.E_ARG
        assert L.bvg_labels_decode_range_dev(h, 3, 2, mem.ptr(d_deg), None, 0, C.byref(need)) == W.E_ARG
        assert L.bvg_labels_decode_range_dev(h, 0, case.n, None, None, 0, C.byref(need)) == W.E_ARG
        L.bvg_labels_close(h)
    for kind in (LIST, LONG_LIST):
        case = range_graph(kind)
        r, h = LC.open_case(W, case)
        assert r == 0
        d_deg = mem.put(case.deg); d_out = mem.put(LC._filled(8, np.int32)); need = C.c_uint64(0)
        assert L.bvg_labels_decode_range_dev(h, 0, case.n, mem.ptr(d_deg), mem.ptr(d_out), 8, C.byref(need)) == W.E_UNSUPPORTED
        assert LC._is_sentinel(mem.get(d_out))
        L.bvg_labels_close(h)


def test_dev_entry_point(W):
    if _device_memory_is_host_memory(W):
        _dev_entry_point(W, LC.HostMemory())
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "dev"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "dev ok" in r.stdout, "child failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-6000:])


if __name__ == "__main__":
    import torch                                                    # (first: see the module docstring)
    assert torch.cuda.is_available(), "bvg_labels_decode_range_dev needs torch on a GPU"
    from conftest import ROOT                                       # noqa: F401  (the repository on sys.path, BVG_TEST_KNOBS)
    import webgraph_big_amd as W
    assert sys.argv[1] == "dev"
    _dev_entry_point(W, TorchMemory(torch))
    print("dev ok")
