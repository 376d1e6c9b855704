"""Shapes, value patterns and defects of arc-label streams, and the one rule they are checked by: shared by tests/test_gpu_labels.py (the
sweep) and tests/test_gpu_labels_fuzz.py (seeded draws).  The streams are written here, bit by bit, by a writer of this file's own (not
the tooling's: tests/test_labels_model.py holds the two against each other), so that codes the label classes never write -- gamma codes
of 2^31 and more, runs of zeros, lengths without elements -- are assembled the same way as the well-formed ones.

THE RULE (check_parity): the device returns 0 exactly when the model (tests/labels_model.py) decodes, and then the arrays are equal.
Otherwise the open returns BVG_E_EOF (last offset behind the stream) or BVG_E_IO (offsets not non-decreasing), or the decode returns
BVG_E_EOF, the scalar output and the list values stay at their sentinel, and list_off holds what the model says the refusal leaves.
No stream is left out.  One class of streams is checked by other means than equal values: list streams that decode to more than
labels_model.VALUES_LIMIT (2^22) elements (only elements of width 0 can: hand_cases() has one, a single list of 2^31 - 1 elements) are
asked for with a small capacity: BVG_E_CAPACITY, *n_values and list_off are compared, the values are never built.

The boundaries of launch_exclusive_scan (csrc/bvg_kernels.hip: kScanTile = 1024 elements per workgroup, scan_partials_serial carries over
64 partial sums at a time), named SCAN_BOUNDARIES: 1024 | 1025 elements (one workgroup | two) and 65536 | 65537 (64 partial sums, one
pass of the wavefront | 65, a second pass with a carry).  The scalar decode scans the outdegrees of the nodes, the list decode the
outdegrees and then the lengths of the arcs' lists: scan_cases() puts node counts (scalar classes) and arc counts (list classes) on both
sides of each."""
import ctypes as C

import numpy as np

import labels_model as M

GAMMA, FIXED, LIST, LONG_LIST = M.GAMMA, M.FIXED, M.LIST, M.LONG_LIST
KIND_NAMES = {GAMMA: "gamma", FIXED: "fixed_int", LIST: "int_list", LONG_LIST: "long_list"}
PATTERNS = ("zero", "ones", "alternating", "random")
SIZES = (1, 255, 256, 257, 513)                         # around the 256-thread block of the label kernels
SCAN_BOUNDARIES = (1024, 1025, 65536, 65537)
TRUNCATIONS = (1, 2, 8, 9, 16, 17)
GAMMA_MAX = (1 << 31) - 1                               # the largest value readGamma() returns

SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 64


def widths(kind):
    return (0,) if kind == GAMMA else range(33) if kind in (FIXED, LIST) else range(65)


class Writer:
    def __init__(self):
        self.parts, self.n = [], 0

    def raw(self, s):
        self.parts.append(s); self.n += len(s)

    def bits(self, v, w):
        if w:
            self.raw(format(v & ((1 << w) - 1), "0%db" % w))

    def gamma(self, x):
        self.raw("0" * ((x + 1).bit_length() - 1) + format(x + 1, "b"))

    def bytes(self):
        s = "".join(self.parts)
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


class Case:
    """A label stream with the offsets and outdegrees it is to be read with."""

    def __init__(self, name, kind, width, stream, offsets, deg):
        self.name, self.kind, self.width, self.stream = name, kind, width, bytes(stream)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.deg = np.ascontiguousarray(deg, dtype=np.int32)
        self.n = len(self.deg)

    def but(self, name, **kw):
        c = Case(self.name + "/" + name, self.kind, self.width, kw.get("stream", self.stream), kw.get("offsets", self.offsets), kw.get("deg", self.deg))
        return c

    def __repr__(self):
        return "Case(%s: %s width %d, %d nodes, %d bytes)" % (self.name, KIND_NAMES[self.kind], self.width, self.n, len(self.stream))


def build(name, kind, width, deg, payload, lead=0):
    """payload: one value per arc (scalar classes) or one list per arc; `lead` bits of ones lie before the first run."""
    w = Writer()
    w.raw("1" * lead)
    offsets, a = [lead], 0
    for d in deg:
        for item in payload[a:a + d]:
            if kind == GAMMA:
                w.gamma(item)
            elif kind == FIXED:
                w.bits(item, width)
            else:
                w.gamma(len(item))
                for v in item:
                    w.bits(v, width)
        a += d
        offsets.append(w.n)
    assert a == len(payload)
    return Case(name, kind, width, w.bytes(), offsets, deg)


# ---- shapes ----
def degrees(n, rng, big=300, top=4):
    """Outdegrees below `top`; empty runs at the start, in the middle and at the end; one node of `big` arcs."""
    if n == 1:
        return [2]
    deg = rng.integers(0, top, size=n)
    deg[0] = deg[-1] = 0
    deg[n // 2:n // 2 + 3] = 0
    if n >= 16 and big:
        deg[n // 3] = big
    return [int(d) for d in deg]


def pattern_values(pattern, width, count, rng):
    mask = (1 << width) - 1
    if pattern == "zero":
        return [0] * count
    if pattern == "ones":
        return [mask] * count
    if pattern == "alternating":
        return [(0xAAAAAAAAAAAAAAAA, 0x5555555555555555)[i & 1] & mask for i in range(count)]
    return [int(v) & mask for v in np.frombuffer(rng.bytes(8 * count), dtype=np.uint64)]


def gamma_values(pattern, count, rng):
    if pattern == "zero":
        return [0] * count
    if pattern == "ones":
        return [GAMMA_MAX] * count
    if pattern == "alternating":
        return [(1, GAMMA_MAX - 1)[i & 1] for i in range(count)]
    vals = [int(v) - 1 for v in rng.geometric(0.02, size=count)]
    for i in range(0, count, 7):
        vals[i] = (0, 1, GAMMA_MAX - 1, GAMMA_MAX, int(rng.integers(0, 1 << 31)))[(i // 7) % 5]
    return vals


def list_lengths(mode, arcs, rng, long_at=None):
    """mode: "zero" (every list empty), "one", "mixed" (0..5, empty lists at the start, in the middle and at the end, one long list)."""
    if mode == "zero":
        return [0] * arcs
    if mode == "one":
        return [1] * arcs
    lens = [int(v) for v in rng.integers(0, 6, size=arcs)]
    if arcs:
        lens[0] = lens[-1] = lens[arcs // 2] = 0
    if long_at is not None and arcs > 4:
        lens[long_at % arcs] = 200
    return lens


def make(name, kind, width, deg, pattern, rng, lens_mode="mixed", lead=0):
    arcs = sum(deg)
    if kind == GAMMA:
        payload = gamma_values(pattern, arcs, rng)
    elif kind == FIXED:
        payload = pattern_values(pattern, width, arcs, rng)
    else:
        lens = list_lengths(lens_mode, arcs, rng, long_at=arcs // 5)
        flat = pattern_values(pattern, width, sum(lens), rng)
        payload, k = [], 0
        for n in lens:
            payload.append(flat[k:k + n]); k += n
    return build(name, kind, width, deg, payload, lead=lead)


LENS_MODE_OF_SIZE = {1: "mixed", 255: "one", 256: "zero", 257: "mixed", 513: "mixed"}


def sweep_cases(kind, pattern, seed=1):
    """Every width of the class over SIZES, one value pattern."""
    for width in widths(kind):
        for n in SIZES:
            rng = np.random.default_rng([seed, kind, width, n])
            yield make("%s-w%d-n%d-%s" % (KIND_NAMES[kind], width, n, pattern), kind, width, degrees(n, rng, big=300 if n == 513 else 0), pattern, rng,
                       lens_mode=LENS_MODE_OF_SIZE[n], lead=(width + n) % 8)


def scan_cases(kind, seed=2):
    """Node counts (scalar classes) or arc counts (list classes) on both sides of each of SCAN_BOUNDARIES."""
    for count in SCAN_BOUNDARIES:
        rng = np.random.default_rng([seed, kind, count])
        width = {GAMMA: 0, FIXED: 11, LIST: 5, LONG_LIST: 37}[kind]
        if kind in (GAMMA, FIXED):
            deg = [int(d) for d in rng.integers(0, 3, size=count)]
            yield make("%s-scan-nodes%d" % (KIND_NAMES[kind], count), kind, width, deg, "random", rng)
        else:
            deg = [0, count // 3, 0, 1, count - count // 3 - 6, 5, 0]
            c = make("%s-scan-arcs%d" % (KIND_NAMES[kind], count), kind, width, deg, "random", rng, lens_mode="mixed")
            assert int(c.deg.sum()) == count
            yield c


END_WIDTHS = {GAMMA: (0,), FIXED: (0, 1, 2, 7, 8, 9, 31, 32), LIST: (0, 1, 7, 8, 31, 32), LONG_LIST: (0, 1, 33, 63, 64)}


def end_of_stream_cases(kind, seed=3):
    """Streams whose last run ends on the last bit of the file, for nbytes = 0, 1, 15 (mod 16) and for every number 0..7 of leading bits
    (so the first run starts at every alignment).  The last node takes as many more arcs as it needs for the stream to end on a byte; a
    fixed width that shares a factor with 8 cannot end every alignment on a byte: those (width, lead) pairs do not exist and are left out.
    The last label is all ones, so the last bit of the file is a one wherever the class allows it."""
    for width in END_WIDTHS[kind]:
        for mod in (0, 1, 15):
            for lead in range(8):
                rng = np.random.default_rng([seed, kind, width, mod, lead])
                deg = degrees(40, rng, big=0, top=3)
                deg[-1] = 1
                arcs = sum(deg)
                done = None
                if kind == GAMMA:
                    head, fill, last = gamma_values("random", arcs - 1, rng), 0, GAMMA_MAX
                elif kind == FIXED:
                    head, fill, last = pattern_values("random", width, arcs - 1, rng), 1, (1 << width) - 1
                else:
                    head, fill, last = [pattern_values("random", width, int(n), rng) for n in rng.integers(0, 4, size=arcs - 1)], [], [(1 << width) - 1] * 2
                for extra in range(8):
                    d2 = deg[:-1] + [1 + extra]
                    payload = head + [fill] * extra + [last]
                    c = build("x", kind, width, d2, payload, lead=lead)
                    if int(c.offsets[-1]) % 8 == 0:
                        done = (d2, payload)
                        break
                if done is None:
                    continue
                nbytes = int(c.offsets[-1]) // 8
                more = (mod - nbytes) % 16                                      # whole bytes of leading ones
                c = build("%s-w%d-end-mod%d-lead%d" % (KIND_NAMES[kind], width, mod, lead), kind, width, done[0], done[1], lead=lead + 8 * more)
                assert int(c.offsets[-1]) == 8 * len(c.stream) and len(c.stream) % 16 == mod
                yield c
    # the empty stream: nothing to read, and something asked of it
    for width in END_WIDTHS[kind]:
        yield Case("%s-w%d-empty-stream" % (KIND_NAMES[kind], width), kind, width, b"", [0] * 6, [0] * 5)
        yield Case("%s-w%d-empty-stream-with-arcs" % (KIND_NAMES[kind], width), kind, width, b"", [0] * 6, [0, 2, 0, 1, 0])


# ---- defects ----
def _first_last_longest(deg):
    nz = np.flatnonzero(deg > 0)
    return (("first", int(nz[0])), ("last", int(nz[-1])), ("longest", int(np.argmax(deg)))) if len(nz) else ()


def defect_names(case):
    names = ["trunc%d-%s" % (k, how) for k in TRUNCATIONS for how in ("as_is", "clamped")]
    names += ["deg%+d-%s" % (s, w) for s in (1, -1) for w in ("first", "last", "longest")]
    return names + ["swapped_offsets", "last_offset_plus_64", "all_zero"]


def apply_defect(case, name, rng=None):
    """The case with one defect; "flip" takes its bit from rng."""
    if name.startswith("trunc"):
        k, how = int(name[5:].split("-")[0]), name.split("-")[1]
        s = case.stream[:max(len(case.stream) - k, 0)]
        offsets = np.minimum(case.offsets, np.uint64(8 * len(s))) if how == "clamped" else case.offsets
        return case.but(name, stream=s, offsets=offsets)
    if name.startswith("deg"):
        where = dict(_first_last_longest(case.deg)).get(name.rsplit("-", 1)[1], 0)      # (a graph without arcs: node 0)
        deg = case.deg.copy()
        deg[where] = max(int(deg[where]) + int(name[3:5]), 0)
        return case.but(name, deg=deg)
    if name == "swapped_offsets":
        o = case.offsets.copy()
        i = np.flatnonzero(o[1:] > o[:-1])
        if len(i):
            j = int(i[len(i) // 2]); o[j], o[j + 1] = o[j + 1], o[j]
        return case.but(name, offsets=o)
    if name == "last_offset_plus_64":
        o = case.offsets.copy(); o[-1] += np.uint64(64)
        return case.but(name, offsets=o)
    if name == "all_zero":
        return case.but(name, stream=bytes(len(case.stream)))
    if name == "flip":
        s = bytearray(case.stream)
        bit = int(rng.integers(0, max(8 * len(s), 1)))
        if s:
            s[bit >> 3] ^= 0x80 >> (bit & 7)
        return case.but("flip%d" % bit, stream=bytes(s))
    raise KeyError(name)


def defect_bases(kind, seed=4):
    """The well-formed streams the defects are applied to: 300 nodes, a few widths of each class."""
    for width in {GAMMA: (0,), FIXED: (0, 1, 13, 32), LIST: (0, 5, 32), LONG_LIST: (0, 17, 64)}[kind]:
        rng = np.random.default_rng([seed, kind, width])
        yield make("%s-w%d-base" % (KIND_NAMES[kind], width), kind, width, degrees(300, rng, big=120), "random", rng, lead=3)


def hand_cases():
    """Codes the label classes never write.  (name, case); what each must do follows from the model, the names say what is expected."""
    def gamma_raw(x):
        w = Writer(); w.gamma(x); return "".join(w.parts)
    out = []
    for name, code in (("gamma-2^31-1-decodes", gamma_raw(GAMMA_MAX)), ("gamma-2^31-refused", gamma_raw(1 << 31)), ("gamma-2^32-1-refused", gamma_raw((1 << 32) - 1)),
                       ("gamma-2^32-refused", gamma_raw(1 << 32)), ("gamma-2^63-refused", gamma_raw(1 << 63)), ("gamma-2^64-2-refused", gamma_raw((1 << 64) - 2)),
                       ("gamma-64-zeros-then-a-code", "0" * 64 + "1" + "1" * 64), ("gamma-70-zeros-run-too-short", "0" * 70 + "1" + "1" * 20),
                       ("gamma-200-zeros", "0" * 200)):
        # a well-formed node on either side: gamma(5) | the code | gamma(7), gamma(0)
        w = Writer(); w.raw("11"); offs = [2]
        w.gamma(5); offs.append(w.n); w.raw(code); offs.append(w.n); w.gamma(7); w.gamma(0); offs.append(w.n)
        out.append(Case(name, GAMMA, 0, w.bytes(), offs, [1, 1, 2]))
    for kind, width in ((LIST, 32), (LIST, 1), (LONG_LIST, 64), (LONG_LIST, 3)):
        for name, n in (("len-2^31-1-no-elements", GAMMA_MAX), ("len-2^31", 1 << 31), ("len-2^32-1", (1 << 32) - 1), ("len-2^40", 1 << 40)):
            w = Writer(); offs = [0]
            w.gamma(2); w.bits(1, width); w.bits(2, width); offs.append(w.n)
            w.gamma(1); w.bits(3, width); w.raw(gamma_raw(n)); w.gamma(1); w.bits(1, width); offs.append(w.n)
            w.gamma(0); offs.append(w.n)
            out.append(Case("%s-w%d-%s" % (KIND_NAMES[kind], width, name), kind, width, w.bytes() + b"\xff" * 24, offs, [1, 3, 1]))
        # a length that fits an int, whose elements would end far behind the file (len * width: up to 2^37 bits)
        w = Writer(); w.gamma(1); w.bits(1, width); w.gamma(GAMMA_MAX - 1); w.bits(1, width)
        out.append(Case("%s-w%d-len-2^31-2-one-element" % (KIND_NAMES[kind], width), kind, width, w.bytes(), [0, w.n], [2]))
    for kind in (LIST, LONG_LIST):
        # elements of width 0: the length alone is the list.  2^31 - 1 elements decode (too many to build: see the module docstring) ...
        w = Writer(); w.gamma(3); w.gamma(GAMMA_MAX); w.gamma(0)
        out.append(Case("%s-w0-len-2^31-1-decodes" % KIND_NAMES[kind], kind, 0, w.bytes(), [0, w.n], [3]))
        w = Writer(); w.gamma(3); w.gamma(1 << 31); w.gamma(0)                   # ... and 2^31 do not
        out.append(Case("%s-w0-len-2^31-refused" % KIND_NAMES[kind], kind, 0, w.bytes(), [0, w.n], [3]))
    return out


# ---- the device side ----
def open_case(W, case):
    """(status, handle)"""
    st = np.frombuffer(case.stream, dtype=np.uint8)
    h = C.c_void_p()
    r = W.lib().bvg_labels_open_mem(case.kind, case.width, case.n, st.ctypes.data if len(st) else None, len(st), case.offsets.ctypes.data, 0, C.byref(h))
    assert (r == 0) == bool(h.value), "a handle is returned exactly with status 0"
    return r, h


def _filled(n, dtype):
    return np.full(n + GUARD, SENT64 if np.dtype(dtype).itemsize == 8 else SENT32, dtype=dtype)


def _is_sentinel(a):
    return bool((a == (SENT64 if a.dtype.itemsize == 8 else SENT32)).all())


class HostMemory:
    """The `device` buffers of bvg_labels_decode_range_dev where device memory is host memory (the emulated library)."""

    def put(self, a):
        return a.copy()

    def ptr(self, a):
        return a.ctypes.data

    def get(self, a):
        return a


def decode_on_device(W, h, case, frm, to, model, mem=None, what=""):
    """One decode call on an open handle, checked against what the model made of the same range (THE RULE of the module docstring).
    mem: None for the host entry points, or the memory for bvg_labels_decode_range_dev (scalar classes)."""
    L = W.lib()
    deg = np.ascontiguousarray(case.deg[frm:to])
    need = C.c_uint64(123)
    if case.kind in (GAMMA, FIXED):
        total = int(deg.sum())
        out = _filled(total, np.int32)
        if mem is None:
            r = L.bvg_labels_decode_range(h, frm, to, deg.ctypes.data if len(deg) else None, out.ctypes.data, total, C.byref(need))
        else:
            d_deg, d_out = mem.put(deg if len(deg) else np.zeros(1, np.int32)), mem.put(out)
            r = L.bvg_labels_decode_range_dev(h, frm, to, mem.ptr(d_deg), mem.ptr(d_out), total, C.byref(need))
            got = mem.get(d_out)
            out = got if r == 0 else np.concatenate([out[:total], got[total:]])      # (the device call may leave labels of a refused range behind: device scratch)
        if not model.ok:
            assert r == W.E_EOF, (what, case, frm, to, model, r)
            assert _is_sentinel(out), (what, case, frm, to, "a refused decode wrote labels")
            return
        assert r == 0 and need.value == total == model.total, (what, case, frm, to, r, need.value, total)
        assert np.array_equal(out[:total], model.labels), (what, case, frm, to, "first difference at arc %d" % int(np.argmax(out[:total] != model.labels)))
        assert _is_sentinel(out[total:]), (what, case, frm, to, "written behind the capacity")
        return
    fn, dt = (L.bvg_labels_decode_range_lists, np.int32) if case.kind == LIST else (L.bvg_labels_decode_range_lists64, np.int64)
    arcs = int(deg.sum())
    loff = np.full(arcs + 1 + GUARD, SENT64, dtype=np.uint64)
    cap = model.total if model.ok and model.values is not None else 16
    vals = _filled(cap, dt)
    r = fn(h, frm, to, deg.ctypes.data if len(deg) else None, loff.ctypes.data, vals.ctypes.data, cap, C.byref(need))
    assert _is_sentinel(loff[arcs + 1:]), (what, case, frm, to, "list_off written behind arcs + 1")
    if not model.ok:
        assert r == W.E_EOF, (what, case, frm, to, model, r)
        assert _is_sentinel(vals), (what, case, frm, to, "a refused decode wrote values")
        assert np.array_equal(loff[:arcs + 1], model.list_off), (what, case, frm, to, "list_off of a refused decode")
        return
    assert np.array_equal(loff[:arcs + 1], model.list_off), (what, case, frm, to, "list_off")
    if model.values is None:                                                    # more elements than anyone builds: sized, not decoded
        assert r == W.E_CAPACITY and need.value == model.total and _is_sentinel(vals), (what, case, frm, to, r, need.value)
        return
    assert r == 0 and need.value == model.total, (what, case, frm, to, r, need.value, model.total)
    assert np.array_equal(vals[:cap], model.values), (what, case, frm, to, "first difference at element %d" % int(np.argmax(vals[:cap] != model.values)))
    assert _is_sentinel(vals[cap:]), (what, case, frm, to, "written behind the capacity")


def check_parity(W, case, ranges=None, mem=None, what=""):
    """THE RULE on one case, over the whole graph or over `ranges`.  Returns what happened: "open:<reason>", or a list with "ok" or the
    defect's name per range."""
    reason = M.check_offsets(len(case.stream), case.offsets)
    r, h = open_case(W, case)
    if reason is not None:
        assert r == (W.E_EOF if reason == "past_file" else W.E_IO), (what, case, reason, r)
        return "open:" + reason
    assert r == 0, (what, case, r)
    seen = []
    try:
        for frm, to in (ranges or [(0, case.n)]):
            model = M.decode(case.kind, case.width, case.stream, case.offsets, frm, to, case.deg[frm:to])
            decode_on_device(W, h, case, frm, to, model, mem=mem, what=what)
            seen.append("ok" if model.ok else model.name)
    finally:
        W.lib().bvg_labels_close(h)
    return seen
