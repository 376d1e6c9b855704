"""CPU: the Transform entry points (bvg_transform_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for
gfx950 and bound by the ctypes mirror; the ABI version stays 4; the argument checks, the longs files and the command line's refusals
need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = sorted(["bvg_transform_from_csr", "bvg_transform_from_csr_dev", "bvg_transform_identity", "bvg_transform_map", "bvg_transform_map_dev",
                "bvg_transform_filter", "bvg_transform_filter_dev", "bvg_transform_transpose", "bvg_transform_symmetrize", "bvg_transform_union",
                "bvg_transform_permutation", "bvg_transform_permutation_dev"])


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_transform_[a-z_0-9]*)\s*\(", text))) == NAMES
    assert re.search(r"#define BVG_TRANSFORM_DROP_LOOPS 1u", text)
    for name, value in (("TRANSFORM_NO_LOOPS", 0), ("TRANSFORM_SAME_CLASS", 1), ("TRANSFORM_DIFFERENT_CLASS", 2), ("PERM_LEX", 0), ("PERM_GRAY", 1), ("PERM_RANDOM", 2)):
        assert re.search(r"\bBVG_%s = %d\b" % (name, value), text), name
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.transform_signatures()
    assert sorted(sigs) == NAMES
    L = W.transform._transform_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert C.sizeof(W.TransformSrc) == 16 and W.TransformSrc.csr.offset == 8
    assert (W.TRANSFORM_NO_LOOPS, W.TRANSFORM_SAME_CLASS, W.TRANSFORM_DIFFERENT_CLASS, W.PERM_LEX, W.PERM_GRAY, W.PERM_RANDOM, W.TRANSFORM_DROP_LOOPS_FLAG) == (0, 1, 2, 0, 1, 2, 1)


def test_argument_checks_need_no_device(W):
    """Every refusal that is decided before a handle is looked at: the handles here are made-up addresses."""
    L = W.transform._transform_fns()
    S = W.TransformSrc
    fake, both, neither = S(None, 0x1000), S(0x1000, 0x2000), S(None, None)
    h = C.c_void_p(0x1234)
    a = np.zeros(4, dtype=np.int64); off = np.zeros(2, dtype=np.uint64)
    out = C.byref(h)
    # no out
    assert L.bvg_transform_from_csr(1, off.ctypes.data, a.ctypes.data, 0, None) == W.E_ARG
    assert L.bvg_transform_identity(C.byref(fake), None) == W.E_ARG
    assert L.bvg_transform_map(C.byref(fake), a.ctypes.data, 4, None) == W.E_ARG
    assert L.bvg_transform_filter(C.byref(fake), 0, None, 0, None) == W.E_ARG
    assert L.bvg_transform_transpose(C.byref(fake), None) == W.E_ARG
    assert L.bvg_transform_symmetrize(C.byref(fake), 0, None) == W.E_ARG
    assert L.bvg_transform_union(C.byref(fake), C.byref(fake), 0, None) == W.E_ARG
    # both or neither source set, or no source at all
    for bad in (both, neither):
        assert L.bvg_transform_identity(C.byref(bad), out) == W.E_ARG
        assert L.bvg_transform_map(C.byref(bad), a.ctypes.data, 4, out) == W.E_ARG
        assert L.bvg_transform_map_dev(C.byref(bad), a.ctypes.data, 4, out) == W.E_ARG
        assert L.bvg_transform_filter(C.byref(bad), 0, None, 0, out) == W.E_ARG
        assert L.bvg_transform_filter_dev(C.byref(bad), 0, None, 0, out) == W.E_ARG
        assert L.bvg_transform_transpose(C.byref(bad), out) == W.E_ARG
        assert L.bvg_transform_symmetrize(C.byref(bad), 0, out) == W.E_ARG
        assert L.bvg_transform_union(C.byref(bad), C.byref(fake), 0, out) == W.E_ARG
        assert L.bvg_transform_union(C.byref(fake), C.byref(bad), 0, out) == W.E_ARG
        assert L.bvg_transform_permutation(C.byref(bad), 0, 0, a.ctypes.data) == W.E_ARG
        assert L.bvg_transform_permutation_dev(C.byref(bad), 0, 0, a.ctypes.data) == W.E_ARG
    assert L.bvg_transform_identity(None, out) == W.E_ARG and L.bvg_transform_union(None, None, 0, out) == W.E_ARG
    # unknown kind or flag bit
    assert L.bvg_transform_filter(C.byref(fake), 3, None, 0, out) == W.E_ARG
    assert L.bvg_transform_filter(C.byref(fake), -1, None, 0, out) == W.E_ARG
    assert L.bvg_transform_permutation(C.byref(fake), 3, 0, a.ctypes.data) == W.E_ARG
    assert L.bvg_transform_symmetrize(C.byref(fake), 2, out) == W.E_ARG
    assert L.bvg_transform_union(C.byref(fake), C.byref(fake), 4, out) == W.E_ARG
    # node_class given with NO_LOOPS
    assert L.bvg_transform_filter(C.byref(fake), W.TRANSFORM_NO_LOOPS, a.ctypes.data, 4, out) == W.E_ARG
    assert L.bvg_transform_filter(C.byref(fake), W.TRANSFORM_NO_LOOPS, None, 4, out) == W.E_ARG
    # negative lengths; an array promised and not given
    assert L.bvg_transform_map(C.byref(fake), a.ctypes.data, -1, out) == W.E_ARG
    assert L.bvg_transform_map(C.byref(fake), None, 4, out) == W.E_ARG
    assert L.bvg_transform_filter(C.byref(fake), W.TRANSFORM_SAME_CLASS, a.ctypes.data, -1, out) == W.E_ARG
    assert L.bvg_transform_from_csr(-1, off.ctypes.data, a.ctypes.data, 0, out) == W.E_ARG
    assert L.bvg_transform_from_csr(1, None, a.ctypes.data, 0, out) == W.E_ARG
    assert L.bvg_transform_from_csr_dev(-1, off.ctypes.data, a.ctypes.data, 0, out) == W.E_ARG
    assert h.value == 0x1234                                                     # nothing was written


def test_python_surface(W):
    for name in ("map_graph", "filter_arcs", "transpose_graph", "symmetrize_graph", "simplify_graph", "union", "lexicographical_permutation",
                 "gray_code_permutation", "random_permutation", "remove_dangling", "identity_graph", "load_longs", "store_longs", "transform_main", "TransformSrc"):
        assert hasattr(W, name), name
    assert hasattr(W.ParsedGraph, "from_csr") and hasattr(W.ParsedGraph, "from_csr_dev")
    with pytest.raises(W.IllegalArgumentException):
        W.map_graph([[0]], [0])                                                  # neither a BVGraph nor a ParsedGraph
    with pytest.raises(W.IllegalArgumentException):
        W.transform.filter_arcs(None, "EVEN_ARCS")


def test_longs_round_trip_in_both_forms(W, tmp_path):
    a = np.array([0, -1, 5, (1 << 62) + 3, -(1 << 63), (1 << 63) - 1], dtype=np.int64)
    p = str(tmp_path / "a.bin")
    W.store_longs(p, a)
    assert open(p, "rb").read()[16:24] == (5).to_bytes(8, "big") and os.path.getsize(p) == 48      # BinIO: big-endian, no header
    assert np.array_equal(W.load_longs(p), a) and W.load_longs(p).dtype == np.int64
    q = str(tmp_path / "a.txt")
    W.store_longs(q, a, ascii=True)
    assert open(q).read().split("\n")[:3] == ["0", "-1", "5"]                                       # TextIO: one per line
    assert np.array_equal(W.load_longs(q, ascii=True), a)
    W.store_longs(p, np.empty(0, np.int64))
    assert len(W.load_longs(p)) == 0


def test_command_line_refusals(W, capsys):
    """Transform.main's ensureNumArgs: every transform takes at least two parameters and each has its own bounds; what is not built is
    refused with a message and 1."""
    with pytest.raises(SystemExit):
        W.transform_main([])                                                     # the transform is required
    for argv in (["identity", "a"], ["identity", "a", "b", "c"], ["lexPerm", "a", "b", "c"], ["mapOffline", "a", "b"], ["mapOffline", "a", "b", "m", "1", "t", "3", "x"],
                 ["union", "a", "b"], ["simplify", "a", "b"], ["simplify", "a", "b", "c", "d"], ["arcfilter", "a", "b"], ["transposeOffline", "a"],
                 ["gray", "a", "b", "1", "t", "x"], ["random", "a", "b", "1", "2", "t", "x"], ["removeDangling", "a"]):
        assert W.transform_main(argv) == 1, argv
        assert "arguments rather than" in capsys.readouterr().err, argv
    assert W.transform_main(["nosuch", "a", "b"]) == 1
    assert "Unknown transform: nosuch" in capsys.readouterr().err
    for argv, word in ((["compose", "a", "b", "c"], "compose"), (["larcfilter", "a", "b", "f"], "labelled"), (["union", "a", "b", "c", "strategy"], "merge strategies"),
                       (["arcfilter", "a", "b", "EVEN_ARCS"], "NO_LOOPS")):
        assert W.transform_main(argv) == 1, argv
        assert word in capsys.readouterr().err, argv
    assert W.transform_main(["random", "a", "b", "notanumber"]) == 1
    capsys.readouterr()
    with pytest.raises(SystemExit):
        W.transform_main(["-s", "NoSuchGraph", "identity", "a", "b"])
    with pytest.raises(W.IOException):
        W.transform_main(["-s", "ASCIIGraph", "identity", "/nonexistent/none", "/nonexistent/out"])


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        W.ParsedGraph.from_csr([0, 1], [0])
