"""CPU: bvg_lcompose is declared in include/bvgraph_hip.h with its semirings and its report, exported by the library cross-compiled for gfx950
and bound by the ctypes mirror in a group of its own; the ABI version stays 4; the argument checks and the command line's refusals need no
device."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)


def test_header_declares_the_entry_point():
    text = header()
    assert re.search(r"\bint\s+bvg_lcompose\s*\(\s*const bvg_lgraph\*\s*g0,\s*const bvg_lgraph\*\s*g1,\s*int semiring,\s*int out_width,\s*"
                     r"bvg_lcompose_report\*\s*report,\s*bvg_lgraph\*\*\s*out\)", text)
    for name, value in [("MIN_PLUS", 0), ("MAX_PLUS", 1), ("MAX_MIN", 2), ("MIN_MAX", 3), ("PLUS_TIMES", 4)]:
        assert re.search(r"\bBVG_SEMIRING_%s\s*=\s*%d\b" % (name, value), text), name
    m = re.search(r"typedef struct bvg_lcompose_report \{(.*?)\} bvg_lcompose_report;", text, flags=re.S)
    assert m
    fields = re.findall(r"\b(u?int64_t)\s+(\w+)(\[\d+\])?;", m.group(1))
    assert [(t, n, d) for t, n, d in fields] == [("uint64_t", "products", ""), ("uint64_t", "arcs", ""), ("uint64_t", "rows", "[3]"), ("uint64_t", "limit", "[2]"),
                                                 ("uint64_t", "batches", ""), ("uint64_t", "out_of_range", ""), ("int64_t", "first_row", ""),
                                                 ("int64_t", "first_successor", "")]
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays
    assert "Not built: compose with a LabelSemiring" not in open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read()


def test_library_exports_and_mirror_binds_it(W):
    lib = C.CDLL(W.build())
    assert hasattr(lib, "bvg_lcompose")
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.lcompose_signatures()
    assert sorted(sigs) == ["bvg_lcompose"]
    assert W.labelled._lcompose_fns().bvg_lcompose.argtypes == sigs["bvg_lcompose"]
    assert "bvg_lcompose" not in W._abi.labelled_signatures() and "bvg_lcompose" not in W._abi.compose_signatures()
    R = W._abi.LComposeReport
    assert C.sizeof(R) == 88                                                   # as the header states it
    assert (R.products.offset, R.arcs.offset, R.rows.offset, R.limit.offset, R.batches.offset) == (0, 8, 16, 40, 56)   # bvg_compose_report's fields first
    assert (R.out_of_range.offset, R.first_row.offset, R.first_successor.offset) == (64, 72, 80)
    assert (W.SEMIRING_MIN_PLUS, W.SEMIRING_MAX_PLUS, W.SEMIRING_MAX_MIN, W.SEMIRING_MIN_MAX, W.SEMIRING_PLUS_TIMES) == (0, 1, 2, 3, 4)


def test_argument_checks_need_no_device(W):
    """Every refusal that is decided before a handle is looked at: the handles here are made-up addresses."""
    L = W.labelled._lcompose_fns()
    fake = C.c_void_p(0x1000)
    h = C.c_void_p(0x1234)
    rep = W._abi.LComposeReport()
    out = C.byref(h)
    assert L.bvg_lcompose(fake, fake, 0, -1, None, None) == W.E_ARG                            # no out
    assert L.bvg_lcompose(fake, fake, 0, -1, C.byref(rep), None) == W.E_ARG
    assert L.bvg_lcompose(None, fake, 0, -1, C.byref(rep), out) == W.E_ARG                     # a NULL source
    assert L.bvg_lcompose(fake, None, 0, -1, None, out) == W.E_ARG
    assert L.bvg_lcompose(None, None, 4, 31, None, out) == W.E_ARG
    for semiring in (-1, 5):
        assert L.bvg_lcompose(fake, fake, semiring, -1, C.byref(rep), out) == W.E_ARG
    for width in (-2, 32):
        assert L.bvg_lcompose(fake, fake, 0, width, C.byref(rep), out) == W.E_ARG
    assert h.value == 0x1234                                                                   # nothing was written
    assert bytes(rep) == bytes(88)


def test_python_surface(W):
    for name in ("compose_labelled", "labelled_compose_main", "SEMIRING_MIN_PLUS", "SEMIRING_PLUS_TIMES"):
        assert hasattr(W, name), name
    with pytest.raises(W.IllegalArgumentException):
        W.compose_labelled([[0]], [[0]], "MIN_PLUS")                                           # neither a LabelledGraph nor a BitStreamArcLabelledImmutableGraph
    for bad in ("min_plus", "PLUS", 5, -1, None, True):                                        # decided before the sources are looked at
        with pytest.raises(W.IllegalArgumentException, match="unknown semiring"):
            W.compose_labelled(None, None, bad)
    for bad in (-1, 32, "8"):
        with pytest.raises(W.IllegalArgumentException, match="out_width"):
            W.compose_labelled(None, None, "MIN_PLUS", out_width=bad)


def test_command_line_refusals(W, capsys):
    for argv in ([], ["a"], ["a", "b", "c"], ["a", "b", "c", "MIN_PLUS", "e"], ["--width", "9", "a", "b", "c"]):
        assert W.labelled_compose_main(argv) == 1, argv
        assert "I need 4 arguments rather than %d." % len([v for v in argv if v not in ("--width", "9")]) in capsys.readouterr().err, argv
    assert W.labelled_compose_main(["a", "b", "c", "TIMES_PLUS"]) == 1                         # before anything is opened
    assert "unknown semiring" in capsys.readouterr().err
    with pytest.raises(W.IOException):
        W.labelled_compose_main(["/nonexistent/none", "/nonexistent/none", "/nonexistent/out", "MIN_PLUS"])
    # the answers of the unlabelled command lines are unchanged
    assert W.compose_main(["a", "b", "c", "semiring"]) == 1
    assert "labelled graphs are not built" in capsys.readouterr().err
    assert W.transform_main(["compose", "a", "b", "c"]) == 1


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        g = W.LabelledGraph.from_csr([0, 1], [0], [3], W.LABEL_GAMMA_INT)
        W.compose_labelled(g, g, "MIN_PLUS")
