"""CPU: the arc-labelled entry points (bvg_lgraph_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for gfx950
and bound by the ctypes mirror; the ABI version stays 4; the argument checks and the command line's refusals need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = sorted(["bvg_lgraph_from_csr", "bvg_lgraph_from_csr_dev", "bvg_lgraph_from_labelled", "bvg_lgraph_close", "bvg_lgraph_info", "bvg_lgraph_get",
                "bvg_lgraph_get_dev", "bvg_lgraph_underlying", "bvg_lgraph_transpose", "bvg_lgraph_union", "bvg_lgraph_symmetrize", "bvg_lgraph_filter",
                "bvg_lgraph_store_labels", "bvg_lgraph_store_labels_dev"])
GAMMA, FIXED, LIST, LONG_LIST = 1, 2, 3, 4


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_lgraph_[a-z_0-9]*)\s*\(", text))) == NAMES
    for name, value in (("LMERGE_KEEP_FIRST", 0), ("LMERGE_MIN", 1), ("LMERGE_MAX", 2), ("LFILTER_NO_LOOPS", 0), ("LFILTER_SAME_CLASS", 1),
                        ("LFILTER_DIFFERENT_CLASS", 2), ("LFILTER_LOWER_BOUND", 3), ("LABEL_GAMMA_INT", 1), ("LABEL_FIXED_INT", 2)):
        assert re.search(r"\bBVG_%s = %d\b" % (name, value), text), name
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays
    # the new family took no name of the families the other ABI tests pin
    assert not [n for n in NAMES if n.startswith(("bvg_transform_", "bvg_text_", "bvg_labels_"))]


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.labelled_signatures()
    assert sorted(sigs) == NAMES
    L = W.labelled._labelled_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert (W.LMERGE_KEEP_FIRST, W.LMERGE_MIN, W.LMERGE_MAX) == (0, 1, 2)
    assert (W.LFILTER_NO_LOOPS, W.LFILTER_SAME_CLASS, W.LFILTER_DIFFERENT_CLASS, W.LFILTER_LOWER_BOUND) == (0, 1, 2, 3)
    assert (W.LFILTER_NO_LOOPS, W.LFILTER_SAME_CLASS, W.LFILTER_DIFFERENT_CLASS) == (W.TRANSFORM_NO_LOOPS, W.TRANSFORM_SAME_CLASS, W.TRANSFORM_DIFFERENT_CLASS)


def test_argument_checks_need_no_device(W):
    """Every refusal that is decided before a handle is looked at: the handles here are made-up addresses."""
    L = W.labelled._labelled_fns()
    fake = 0x1000
    h = C.c_void_p(0x1234)
    out = C.byref(h)
    a = np.zeros(4, dtype=np.int64); lab = np.zeros(4, dtype=np.int32); off = np.zeros(2, dtype=np.uint64)
    # no out
    assert L.bvg_lgraph_from_csr(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, GAMMA, 0, 0, None) == W.E_ARG
    assert L.bvg_lgraph_from_csr_dev(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, GAMMA, 0, 0, None) == W.E_ARG
    assert L.bvg_lgraph_from_labelled(fake, fake, None) == W.E_ARG
    assert L.bvg_lgraph_underlying(fake, None) == W.E_ARG
    assert L.bvg_lgraph_transpose(fake, None) == W.E_ARG
    assert L.bvg_lgraph_union(fake, fake, 0, None) == W.E_ARG
    assert L.bvg_lgraph_symmetrize(fake, 0, None) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, 0, None, 0, 0, None) == W.E_ARG
    assert L.bvg_lgraph_store_labels(fake, None, None, None) == W.E_ARG
    assert L.bvg_lgraph_store_labels_dev(fake, None, 0, None, None) == W.E_ARG
    # NULL sources
    assert L.bvg_lgraph_from_labelled(None, fake, out) == W.E_ARG and L.bvg_lgraph_from_labelled(fake, None, out) == W.E_ARG
    assert L.bvg_lgraph_info(None, None, None, None, None) == W.E_ARG
    assert L.bvg_lgraph_get(None, None, 0, None, 0, None, 0) == W.E_ARG and L.bvg_lgraph_get_dev(None, None, 0, None, 0, None, 0) == W.E_ARG
    assert L.bvg_lgraph_underlying(None, out) == W.E_ARG
    assert L.bvg_lgraph_transpose(None, out) == W.E_ARG
    assert L.bvg_lgraph_union(None, fake, 0, out) == W.E_ARG and L.bvg_lgraph_union(fake, None, 0, out) == W.E_ARG
    assert L.bvg_lgraph_symmetrize(None, 0, out) == W.E_ARG
    assert L.bvg_lgraph_filter(None, 0, None, 0, 0, out) == W.E_ARG
    nb = C.c_uint64(77)
    assert L.bvg_lgraph_store_labels(None, out, C.byref(nb), out) == W.E_ARG and L.bvg_lgraph_store_labels_dev(None, None, 0, C.byref(nb), None) == W.E_ARG
    assert L.bvg_lgraph_from_csr(1, None, a.ctypes.data, lab.ctypes.data, GAMMA, 0, 0, out) == W.E_ARG
    L.bvg_lgraph_close(None)                                                     # closing nothing is allowed
    # unknown strategy, filter kind or label kind
    for s in (-1, 3, 99):
        assert L.bvg_lgraph_union(fake, fake, s, out) == W.E_ARG and L.bvg_lgraph_symmetrize(fake, s, out) == W.E_ARG
    for k in (-1, 4):
        assert L.bvg_lgraph_filter(fake, k, None, 0, 0, out) == W.E_ARG
    for k in (0, 5, -1):
        assert L.bvg_lgraph_from_csr(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, k, 0, 0, out) == W.E_ARG
        assert L.bvg_lgraph_from_csr_dev(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, k, 0, 0, out) == W.E_ARG
    # width 32 (FixedWidthIntLabel.java:41-42 stops at 31), a negative width; a list kind
    assert L.bvg_lgraph_from_csr(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, FIXED, 32, 0, out) == W.E_ARG
    assert L.bvg_lgraph_from_csr(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, FIXED, -1, 0, out) == W.E_ARG
    for k in (LIST, LONG_LIST):
        assert L.bvg_lgraph_from_csr(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, k, 8, 0, out) == W.E_UNSUPPORTED
        assert L.bvg_lgraph_from_csr_dev(1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, k, 8, 0, out) == W.E_UNSUPPORTED
    # lower_bound with a filter that takes none; classes with a filter that takes none; negative lengths
    assert L.bvg_lgraph_filter(fake, W.LFILTER_NO_LOOPS, None, 0, 5, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_SAME_CLASS, a.ctypes.data, 4, 5, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_NO_LOOPS, a.ctypes.data, 4, 0, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_NO_LOOPS, None, 4, 0, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_LOWER_BOUND, a.ctypes.data, 4, 1, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_SAME_CLASS, a.ctypes.data, -1, 0, out) == W.E_ARG
    assert L.bvg_lgraph_filter(fake, W.LFILTER_DIFFERENT_CLASS, None, 4, 0, out) == W.E_ARG
    assert L.bvg_lgraph_from_csr(-1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, GAMMA, 0, 0, out) == W.E_ARG
    assert L.bvg_lgraph_from_csr_dev(-1, off.ctypes.data, a.ctypes.data, lab.ctypes.data, GAMMA, 0, 0, out) == W.E_ARG
    assert h.value == 0x1234 and nb.value == 77                                  # nothing was written


def test_python_surface(W):
    for name in ("LabelledGraph", "transpose_labelled", "union_labelled", "symmetrize_labelled", "filter_labelled_arcs", "labelled_transform_main", "label_spec"):
        assert hasattr(W, name), name
    for name in ("from_csr", "from_csr_dev", "from_graph", "num_nodes", "num_arcs", "csr", "underlying", "store_labels", "write", "close", "__enter__", "__exit__"):
        assert hasattr(W.LabelledGraph, name), name
    for call in (lambda: W.transpose_labelled([[0]]), lambda: W.union_labelled(None, None), lambda: W.symmetrize_labelled("g"),
                 lambda: W.filter_labelled_arcs(3, "NO_LOOPS"), lambda: W.LabelledGraph.from_graph([[0]])):
        with pytest.raises(W.IllegalArgumentException):
            call()                                                               # neither a LabelledGraph nor a BitStreamArcLabelledImmutableGraph
    with pytest.raises(W.IllegalArgumentException):
        W.union_labelled(None, None, "SUM")                                      # a strategy that is not built
    with pytest.raises(W.IllegalArgumentException):
        W.filter_labelled_arcs(None, "EVEN_ARCS")
    with pytest.raises(W.IllegalArgumentException):
        W.filter_labelled_arcs(None, "NO_LOOPS", lower_bound=3)
    with pytest.raises(W.IllegalArgumentException):
        W.LabelledGraph.from_csr([0, 1], [0], [1, 2], GAMMA)                     # one label per arc
    assert W.label_spec(GAMMA, 0) == "it.unimi.dsi.big.webgraph.labelling.GammaCodedIntLabel(FOO)"
    assert W.label_spec(FIXED, 13) == "it.unimi.dsi.big.webgraph.labelling.FixedWidthIntLabel(FOO,13)"
    assert W.parse_label_spec(W.label_spec(FIXED, 13)) == (FIXED, 13)


def test_command_line_refusals(W, capsys, tmp_path):
    with pytest.raises(SystemExit):
        W.labelled_transform_main([])                                            # the transform is required
    for argv in (["transposeOffline", "a"], ["transposeOffline", "a", "b", "c"], ["symmetrizeOffline", "a", "b"], ["symmetrizeOffline", "a", "b", "MIN", "x"],
                 ["union", "a", "b"], ["union", "a", "b", "c", "MIN", "x"], ["larcfilter", "a", "b"], ["larcfilter", "a", "b", "NO_LOOPS", "x"]):
        assert W.labelled_transform_main(argv) == 1, argv
        assert "arguments rather than" in capsys.readouterr().err, argv
    assert W.labelled_transform_main(["union", "a", "b", "c"]) == 1
    assert "Uniting labelled graphs requires a merge strategy" in capsys.readouterr().err
    assert W.labelled_transform_main(["nosuch", "a", "b"]) == 1
    assert "Unknown transform: nosuch" in capsys.readouterr().err
    for argv, word in ((["union", "a", "b", "c", "SUM"], "merge strategy"), (["symmetrizeOffline", "a", "b", "SUM"], "merge strategy"),
                       (["larcfilter", "a", "b", "EVEN_ARCS"], "LowerBound"), (["larcfilter", "a", "b", "LowerBound(x)"], "LowerBound")):
        assert W.labelled_transform_main(argv) == 1, argv
        assert word in capsys.readouterr().err, argv
    base = str(tmp_path / "plain")
    with open(base + ".properties", "w") as f:
        f.write("graphclass=it.unimi.dsi.big.webgraph.BVGraph\nnodes=1\narcs=0\n")
    assert W.labelled_transform_main(["larcfilter", base, str(tmp_path / "out"), "NO_LOOPS"]) == 1
    assert "Filtering on labelled arcs requires a labelled graph" in capsys.readouterr().err
    with pytest.raises(W.IOException):
        W.labelled_transform_main(["transposeOffline", "/nonexistent/none", "/nonexistent/out"])
    # the unlabelled command lines answer as before
    assert W.transform_main(["larcfilter", "a", "b", "f"]) == 1
    assert "labelled" in capsys.readouterr().err
    assert W.transform_main(["union", "a", "b", "c", "strategy"]) == 1
    assert "merge strategies" in capsys.readouterr().err


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        W.LabelledGraph.from_csr([0, 1], [0], [5], GAMMA)
