"""CPU: bvg_compose is declared in include/bvgraph_hip.h, exported by the library cross-compiled for gfx950 and bound by the ctypes mirror;
the ABI version stays 4; the argument checks and the command line's refusals need no device."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+bvg_compose\s*\(\s*const bvg_transform_src\*\s*g0,\s*const bvg_transform_src\*\s*g1,\s*bvg_compose_report\*\s*report,\s*bvg_text\*\*\s*out\)", text)
    assert re.search(r"typedef struct bvg_compose_report \{", text)
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_it(W):
    lib = C.CDLL(W.build())
    assert hasattr(lib, "bvg_compose")
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.compose_signatures()
    assert sorted(sigs) == ["bvg_compose"]
    assert W.transform._compose_fns().bvg_compose.argtypes == sigs["bvg_compose"]
    assert C.sizeof(W.ComposeReport) == 64
    assert (W.ComposeReport.products.offset, W.ComposeReport.arcs.offset, W.ComposeReport.rows.offset, W.ComposeReport.limit.offset, W.ComposeReport.batches.offset) == (0, 8, 16, 40, 56)
    assert "bvg_compose" not in W._abi.transform_signatures()


def test_argument_checks_need_no_device(W):
    """Every refusal that is decided before a handle is looked at: the handles here are made-up addresses."""
    L = W.transform._compose_fns()
    S = W.TransformSrc
    fake, both, neither = S(None, 0x1000), S(0x1000, 0x2000), S(None, None)
    h = C.c_void_p(0x1234)
    rep = W.ComposeReport()
    out = C.byref(h)
    assert L.bvg_compose(C.byref(fake), C.byref(fake), None, None) == W.E_ARG                 # no out
    assert L.bvg_compose(C.byref(fake), C.byref(fake), C.byref(rep), None) == W.E_ARG
    for bad in (both, neither):                                                                # both or neither member of a source set
        assert L.bvg_compose(C.byref(bad), C.byref(fake), None, out) == W.E_ARG
        assert L.bvg_compose(C.byref(fake), C.byref(bad), C.byref(rep), out) == W.E_ARG
        assert L.bvg_compose(C.byref(bad), C.byref(bad), None, out) == W.E_ARG
    assert L.bvg_compose(None, C.byref(fake), None, out) == W.E_ARG                           # a NULL source
    assert L.bvg_compose(C.byref(fake), None, None, out) == W.E_ARG
    assert L.bvg_compose(None, None, None, out) == W.E_ARG
    assert h.value == 0x1234                                                                   # nothing was written
    assert rep.products == 0 and rep.arcs == 0


def test_python_surface(W):
    assert hasattr(W, "compose") and hasattr(W, "compose_main") and hasattr(W, "ComposeReport")
    with pytest.raises(W.IllegalArgumentException):
        W.compose([[0]], [[0]])                                                                # neither a BVGraph nor a ParsedGraph


def test_command_line_refusals(W, capsys):
    for argv in ([], ["a"], ["a", "b"], ["a", "b", "c", "d", "e"], ["-d", "ASCIIGraph", "a", "b"]):
        assert W.compose_main(argv) == 1, argv
        assert "I need 3 arguments rather than %d." % len([v for v in argv if v not in ("-d", "ASCIIGraph")]) in capsys.readouterr().err, argv
    assert W.compose_main(["a", "b", "c", "semiring"]) == 1
    assert "labelled graphs are not built" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        W.compose_main(["-s", "NoSuchGraph", "a", "b", "c"])
    with pytest.raises(W.IOException):
        W.compose_main(["-s", "ASCIIGraph", "/nonexistent/none", "/nonexistent/none", "/nonexistent/out"])
    # Transform.main's own answer to `compose` is unchanged: 1, before anything is opened
    assert W.transform_main(["compose", "a", "b", "c"]) == 1
    assert "compose" in capsys.readouterr().err


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        g = W.ParsedGraph.from_csr([0, 1], [0])
        W.compose(g, g)
