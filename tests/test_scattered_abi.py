"""CPU: the scattered arc list entry points (bvg_scattered_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled
for gfx950 and bound by the ctypes mirror; the ABI version stays 4; the argument checks and the command line's refusals need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = sorted(["bvg_scattered_parse", "bvg_scattered_parse_dev", "bvg_scattered_ids", "bvg_scattered_ids_dev"])
REASONS = {1: "bad_source", 2: "bad_target", 3: "no_target", 4: "too_large", 5: "trailing", 6: "unknown_source", 7: "unknown_target"}


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_scattered_[a-z_0-9]*)\s*\(", text))) == NAMES
    assert re.search(r"#define BVG_TEXT_STRICT\s+4u", text)
    for value, name in REASONS.items():
        assert re.search(r"\bBVG_SCATTERED_%s = %d\b" % (name.upper(), value), text), name
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.scattered_signatures()
    assert sorted(sigs) == NAMES
    L = W.textgraph._scattered_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    R = W.ScatteredReport
    assert C.sizeof(R) == 104 and R.first_byte.offset == 80 and R.first_line.offset == 88 and R.first_reason.offset == 96
    assert W._abi.SCATTERED_REASONS == REASONS and W._abi.TEXT_STRICT_FLAG == 4


def test_argument_checks_need_no_device(W):
    L = W.textgraph._scattered_fns()
    known = np.array([1, 2], dtype=np.int64)
    for fn in (L.bvg_scattered_parse, L.bvg_scattered_parse_dev):
        h = C.c_void_p(0x1234); err = W.TextError(byte=7); rep = W.ScatteredReport(lines=9)
        assert fn(b"1 2\n", 4, 0, None, 0, 0, None, C.byref(rep), C.byref(err)) == W.E_ARG                       # no out
        assert fn(None, 4, 0, None, 0, 0, C.byref(h), C.byref(rep), C.byref(err)) == W.E_ARG                         # bytes promised, none given
        assert fn(b"1 2\n", 4, 8, None, 0, 0, C.byref(h), C.byref(rep), C.byref(err)) == W.E_ARG                     # unknown flag bit
        assert fn(b"1 2\n", 4, 0, known.ctypes.data, -1, 0, C.byref(h), C.byref(rep), C.byref(err)) == W.E_ARG       # n_known < 0
        assert fn(b"1 2\n", 4, 0, None, 2, 0, C.byref(h), C.byref(rep), C.byref(err)) == W.E_ARG                     # ids promised, none given
        assert h.value == 0x1234 and err.byte == 7 and rep.lines == 9                                                # nothing was written
    assert L.bvg_scattered_ids(None, None, 0) == W.E_ARG and L.bvg_scattered_ids_dev(None, None, 0) == W.E_ARG


def test_mirrors_expose_the_surface(W):
    for name in ("ScatteredGraph", "parse_scattered_arcs", "parse_scattered_arcs_dev", "load_scattered_arcs", "scattered_main", "ScatteredReport"):
        assert hasattr(W, name), name
    assert issubclass(W.ScatteredGraph, W.ParsedGraph) and hasattr(W.ScatteredGraph, "ids")
    hpp = open(os.path.join(ROOT, "webgraph-big_amd", "host", "bvgraph.hpp")).read()
    assert "parseScatteredArcs" in hpp and "class ScatteredGraph" in hpp


def test_command_line(W, tmp_path, capsys):
    with pytest.raises(SystemExit):
        W.scattered_main([])                                                    # the basename is required
    for opt in (["-f", "fn"], ["-b"], ["-C", "UTF-8"], ["-n", "3"]):
        assert W.scattered_main(opt + ["base"]) == 1                            # the translation function of the reference: a message
        assert "not supported" in capsys.readouterr().err
    assert W.scattered_main(["-T", "dir", "base"]) == 1
    assert "not supported" in capsys.readouterr().err
    assert W.scattered_main(["-c", "RESIDUALS_FOO", "base"]) == 1
    a = W.textgraph.scattered_arg_parser().parse_args(["-S", "-L", "-z", "-w", "5", "-m", "2", "-i", "0", "-k", "4", "-c", "RESIDUALS_GAMMA", "--ids", "x.ids", "--input", "in", "b"])
    assert (a.symmetrize, a.no_loops, a.zipped, a.window_size, a.max_ref_count, a.min_interval_length, a.zeta_k, a.comp, a.ids, a.input, a.basename) == \
        (True, True, True, 5, 2, 0, 4, ["RESIDUALS_GAMMA"], "x.ids", "in", "b")
    with pytest.raises(W.IOException):
        W.scattered_main(["--input", str(tmp_path / "none"), str(tmp_path / "out")])


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        W.parse_scattered_arcs(b"-1 15\n")
    with pytest.raises(W.DeviceError):
        W.parse_scattered_arcs(b"-1 15\n", ids=[-1, 15])
