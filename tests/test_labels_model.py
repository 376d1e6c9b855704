"""The plain model of the arc-label decode (tests/labels_model.py) against the CPU oracle (oracle.labels_decode*), without a GPU: the hand-written
streams of tests/test_labels.py, and every stream tests/test_gpu_labels.py and tests/test_gpu_labels_fuzz.py send to the device (a cut of the width
sweep; all end-of-stream, defect and hand-assembled cases).

Where the two legitimately differ: ONLY in "gamma_range".  The oracle, like the reference's readGamma(), wraps a gamma-coded value of 2^31 or more
to int32 (and goes on to read a list of that many elements, to whatever end); the model names it a defect, and the device refuses it.  Wherever the
model says anything else, the oracle says the same: it decodes the model's arrays, or it fails.  The stream writer of label_cases is held against
the tooling's here as well."""
import numpy as np
import pytest

import label_cases as LC
import labels_model as M
from label_cases import FIXED, GAMMA, LIST, LONG_LIST

KINDS = (GAMMA, FIXED, LIST, LONG_LIST)


def oracle_decode(oracle, case, frm, to):
    """("ok", arrays...) or ("error", code)"""
    deg = case.deg[frm:to]
    try:
        if case.kind in (GAMMA, FIXED):
            return "ok", oracle.labels_decode(case.kind, case.width, case.stream, case.offsets, frm, to, deg)
        fn = oracle.labels_decode_lists if case.kind == LIST else oracle.labels_decode_long_lists
        return ("ok",) + tuple(fn(case.width, case.stream, case.offsets, frm, to, deg))
    except oracle.OracleError as e:
        return "error", e.code


def agree(oracle, case, ranges=None):
    """The model's outcome per range, after holding the oracle against it."""
    seen = []
    if M.check_offsets(len(case.stream), case.offsets) is not None:
        return "open:" + M.check_offsets(len(case.stream), case.offsets)       # (the oracle takes offsets as they come: the open is the product's check)
    for frm, to in (ranges or [(0, case.n)]):
        m = M.decode(case.kind, case.width, case.stream, case.offsets, frm, to, case.deg[frm:to])
        seen.append("ok" if m.ok else m.name)
        if m.ok and m.list_off is not None and m.values is None:
            continue                                                           # (2^22 elements and more: nobody builds them, the oracle included)
        if not m.ok and m.name == "gamma_range":
            if case.kind in (LIST, LONG_LIST) and case.width == 0:
                continue                                                       # (the oracle would count to 2^31 and beyond, one element of no bits at a time)
            o = oracle_decode(oracle, case, frm, to)                           # the one legitimate difference: the oracle may well decode, wrapped
            if case.kind == GAMMA and o[0] == "ok" and m.node == to - 1 and case.deg[m.node] == 1:
                assert (o[1] < 0).any(), (case, "the oracle wraps, so some label is negative")
            continue
        o = oracle_decode(oracle, case, frm, to)
        if m.ok:
            assert o[0] == "ok", (case, frm, to, o)
            if case.kind in (GAMMA, FIXED):
                assert np.array_equal(o[1], m.labels), (case, frm, to)
            else:
                assert np.array_equal(o[1], m.list_off) and np.array_equal(o[2], m.values) and o[2].dtype == m.values.dtype, (case, frm, to)
        else:
            assert o[0] == "error", (case, frm, to, m)
    return seen


def test_model_reads_handwritten_label_streams():
    # gamma(0)=1 gamma(1)=010 | node 1 empty | gamma(5)=00110 gamma(1000)=0000000001 111101001 gamma(7)=0001000
    stream = bytes.fromhex("a3003e9100")
    lo, deg = [0, 4, 4, 35], [2, 0, 3]
    assert M.decode(GAMMA, 0, stream, lo, 0, 3, deg).labels.tolist() == [0, 1, 5, 1000, 7]
    assert M.decode(GAMMA, 0, stream, lo, 2, 3, deg[2:]).labels.tolist() == [5, 1000, 7]
    assert M.decode(GAMMA, 0, stream, lo, 1, 2, deg[1:2]).labels.tolist() == []
    stream = bytes.fromhex("00001017e801c0")                                   # FixedWidthIntLabel(FOO,10)
    lo = [0, 20, 20, 50]
    assert M.decode(FIXED, 10, stream, lo, 0, 3, deg).labels.tolist() == [0, 1, 5, 1000, 7]
    bad = M.decode(FIXED, 10, stream, lo, 0, 3, [2, 1, 3])
    assert not bad.ok and (bad.name, bad.node) == ("overrun", 1)
    short = M.decode(FIXED, 10, stream, lo, 0, 3, [2, 0, 2])
    assert not short.ok and (short.name, short.node) == ("short", 2)
    # lists: gamma(2) 3 1 | gamma(0) | gamma(1) 2, elements of 2 bits: 011 11 01 | 1 | 010 10
    stream = bytes([0b01111011, 0b01010000])
    m = M.decode(LIST, 2, stream, [0, 8, 13], 0, 2, [2, 1])
    assert m.list_off.tolist() == [0, 2, 2, 3] and m.values.tolist() == [3, 1, 2]
    m = M.decode(LONG_LIST, 2, stream, [0, 8, 13], 1, 2, [1])
    assert m.list_off.tolist() == [0, 1] and m.values.tolist() == [2] and m.values.dtype == np.int64
    # int32 / int64 wrap at the end only
    assert M.decode(FIXED, 32, b"\xff\xff\xff\xfe", [0, 32], 0, 1, [1]).labels.tolist() == [-2]
    assert M.decode(LONG_LIST, 64, b"\x40" + b"\xff" * 8, [0, 67], 0, 1, [1]).values.tolist() == [(1 << 59) - 1]
    assert M.decode(LONG_LIST, 64, b"\x5f" + b"\xff" * 8, [0, 67], 0, 1, [1]).values.tolist() == [-1]
    assert M.check_offsets(1, [0, 9]) == "past_file" and M.check_offsets(2, [0, 9, 8]) == "non_monotone" and M.check_offsets(1, [0, 20, 9]) == "past_file"
    assert M.check_offsets(0, [0, 0]) is None


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: LC.KIND_NAMES[k])
def test_model_and_oracle_on_the_sweep(oracle, kind):
    """A cut of test_gpu_labels.py::test_parameter_space (every fourth width and the widest, two patterns), the smaller scan boundaries, the ranges."""
    ws = sorted(set(list(LC.widths(kind))[::4]) | {max(LC.widths(kind))})
    for pattern in ("ones", "random"):
        for case in LC.sweep_cases(kind, pattern):
            if case.width in ws:
                assert agree(oracle, case) == ["ok"], case
    for case in LC.scan_cases(kind):
        if case.n <= 2000:
            assert agree(oracle, case) == ["ok"], case


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: LC.KIND_NAMES[k])
def test_model_and_oracle_at_the_end_of_the_stream(oracle, kind):
    count = 0
    for case in LC.end_of_stream_cases(kind):
        seen = agree(oracle, case, ranges=[(0, case.n), (case.n - 1, case.n)])
        assert seen[1] == "ok" and (seen[0] == "ok" or "with-arcs" in case.name), (case, seen)
        count += 1
    assert count >= 24


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: LC.KIND_NAMES[k])
def test_model_and_oracle_on_every_defect(oracle, kind):
    tally = {}
    for base in LC.defect_bases(kind):
        rng = np.random.default_rng([7, kind, base.width])                     # (the flips of test_gpu_labels.py::test_status_parity_on_every_defect)
        x = int(np.argmax(base.deg))
        for name in LC.defect_names(base) + ["flip"] * 12:
            case = LC.apply_defect(base, name, rng)
            seen = agree(oracle, case, ranges=[(0, case.n), (x - 1, x + 2), (x, x + 1)])
            for s in ([seen] if isinstance(seen, str) else seen):
                tally[s] = tally.get(s, 0) + 1
    for s in ("ok", "open:past_file", "open:non_monotone", "overrun", "short"):
        assert tally.get(s), (s, tally)


def test_model_and_oracle_on_hand_assembled_codes(oracle):
    seen = {case.name: agree(oracle, case)[0] for case in LC.hand_cases()}
    assert seen["gamma-2^31-1-decodes"] == "ok" and seen["gamma-2^31-refused"] == seen["gamma-2^32-1-refused"] == "gamma_range"
    # what the oracle makes of the two the issue of the device's refusal started from: it wraps
    for name, wrapped in (("gamma-2^31-refused", -(1 << 31)), ("gamma-2^32-1-refused", -1)):
        case = [c for c in LC.hand_cases() if c.name == name][0]
        assert oracle_decode(oracle, case, 0, 3)[1].tolist() == [5, wrapped, 7, 0]


def test_fuzz_draws_are_comparable_and_varied(oracle):
    """The first 400 draws of tests/test_gpu_labels_fuzz.py at its default seed: none is of the class that is sized instead of compared, every outcome
    occurs, and the oracle agrees with the model on each."""
    from test_gpu_labels_fuzz import DEFAULT_SEED, draw
    tally = {}
    for c in range(400):
        what, case, ranges = draw(np.random.default_rng([DEFAULT_SEED, c]))
        if M.check_offsets(len(case.stream), case.offsets) is None:
            for frm, to in ranges:
                m = M.decode(case.kind, case.width, case.stream, case.offsets, frm, to, case.deg[frm:to])
                assert not (m.ok and m.list_off is not None and m.values is None), (what, "more than 2^22 elements")
        seen = agree(oracle, case, ranges)
        for s in ([seen] if isinstance(seen, str) else seen):
            tally[s] = tally.get(s, 0) + 1
    for s in ("ok", "open:past_file", "open:non_monotone", "overrun", "short", "gamma_range"):
        assert tally.get(s), (s, tally)


def test_the_writer_of_the_cases_writes_what_the_tooling_writes(tools):
    for kind, width in ((GAMMA, 0), (FIXED, 0), (FIXED, 13), (FIXED, 32), (LIST, 0), (LIST, 7), (LIST, 32), (LONG_LIST, 33), (LONG_LIST, 64)):
        rng = np.random.default_rng([9, kind, width])
        case = LC.make("w", kind, width, LC.degrees(257, rng, big=90), "random", rng)
        m = M.decode(kind, width, case.stream, case.offsets, 0, case.n, case.deg)
        arc_off = np.zeros(case.n + 1, dtype=np.uint64); arc_off[1:] = np.cumsum(case.deg)
        if kind in (GAMMA, FIXED):
            sl = tools.store_labels(kind, width, m.labels, arc_off)
        elif kind == LIST:
            sl = tools.store_label_lists(width, m.list_off, m.values, arc_off)
        else:
            sl = tools.store_label_long_lists(width, m.list_off, m.values, arc_off)
        assert sl.stream.tobytes() == case.stream and np.array_equal(sl.offsets, case.offsets), (kind, width)
        assert sl.spec() == "it.unimi.dsi.big.webgraph.labelling." + {GAMMA: "GammaCodedIntLabel(FOO)", FIXED: "FixedWidthIntLabel(FOO,%d)", LIST: "FixedWidthIntListLabel(FOO,%d)",
                                                                      LONG_LIST: "FixedWidthLongListLabel(FOO,%d)"}[kind].replace("%d", str(width))
