"""CPU: the HyperBall entry points (bvg_hyperball_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for
gfx950 and bound by the ctypes mirror; the Python and C++ mirrors expose the object.  No compute calls: there is no GPU here."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = sorted(["bvg_hyperball_create", "bvg_hyperball_close", "bvg_hyperball_init", "bvg_hyperball_iterate", "bvg_hyperball_run", "bvg_hyperball_info",
                "bvg_hyperball_neighbourhood_function", "bvg_hyperball_registers", "bvg_hyperball_counts", "bvg_hyperball_counts_dev", "bvg_hyperball_centrality",
                "bvg_hyperball_centrality_dev", "bvg_hyperball_relative_standard_deviation"])


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)


def test_header_declares_exactly_the_hyperball_entry_points():
    text = _header()
    assert sorted(set(re.findall(r"\b(bvg_hyperball_[a-z_0-9]+)\s*\(", text))) == NAMES
    assert re.search(r"#define BVG_HB_SUM_OF_DISTANCES 1u", text) and re.search(r"#define BVG_HB_HARMONIC 2u", text)
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays
    assert not [n for n in NAMES if n.startswith("bvg_bfs_")]


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    sigs = W._abi.hyperball_signatures()
    assert sorted(sigs) == NAMES
    L = W.bvgraph._hyperball_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert L.bvg_abi_version() == 4
    assert (W.HB_SUM_OF_DISTANCES, W.HB_HARMONIC) == (1, 2)
    assert W._abi.HB_WHICH == {"sum_of_distances": 0, "harmonic": 1, "closeness": 2, "lin": 3, "nieminen": 4, "reachable": 5}
    text = _header()
    for name, value in W._abi.HB_WHICH.items():
        assert re.search(r"BVG_HB_WHICH_%s = %d\b" % (name.upper(), value), text), name


def test_argument_checks_need_no_device(W):
    L = W.bvgraph._hyperball_fns()
    h = C.c_void_p()
    fake = C.c_void_p(1)                                                        # never dereferenced: log2m and flags are looked at first
    assert L.bvg_hyperball_create(None, 6, 0, 0, C.byref(h)) == W.E_ARG
    assert L.bvg_hyperball_create(fake, 6, 0, 0, None) == W.E_ARG
    assert L.bvg_hyperball_create(fake, 3, 0, 0, C.byref(h)) == W.E_ARG
    assert L.bvg_hyperball_create(fake, 6, 4, 0, C.byref(h)) == W.E_ARG         # unknown flag bits
    assert L.bvg_hyperball_create(fake, 13, 0, 0, C.byref(h)) == W.E_UNSUPPORTED
    assert L.bvg_hyperball_init(None, 0) == W.E_ARG and L.bvg_hyperball_iterate(None) == W.E_ARG
    assert L.bvg_hyperball_run(None, -1, -1.0) == W.E_ARG
    assert L.bvg_hyperball_info(None, None, None, None, None) == W.E_ARG
    assert L.bvg_hyperball_neighbourhood_function(None, None, 0) == W.E_ARG
    assert L.bvg_hyperball_registers(None, 0, 0, None) == W.E_ARG
    assert L.bvg_hyperball_counts(None, 0, 0, None) == W.E_ARG and L.bvg_hyperball_counts_dev(None, 0, 0, None) == W.E_ARG
    assert L.bvg_hyperball_centrality(None, 0, None) == W.E_ARG and L.bvg_hyperball_centrality_dev(None, 0, None) == W.E_ARG
    L.bvg_hyperball_close(None)


def test_relative_standard_deviation(W):
    import hyperball_model as M
    for log2m, beta in ((4, 1.106), (5, 1.070), (6, 1.054), (7, 1.046), (8, 1.04), (12, 1.04)):
        want = beta / (1 << log2m) ** 0.5
        assert abs(W.HyperBall.relative_standard_deviation(log2m) - want) <= 1e-15
        assert abs(M.relative_standard_deviation(log2m) - want) <= 1e-15


def test_mirrors_expose_the_object(W):
    for name in ("init", "iterate", "run", "modified", "iteration", "neighbourhood_function", "registers", "count", "counts", "sum_of_distances", "harmonic_centrality",
                 "closeness", "lin", "nieminen", "reachable", "close", "__enter__", "__exit__"):
        assert hasattr(W.HyperBall, name), name
    assert hasattr(W.BVGraph, "hyperball") and callable(W.hyperball_main)
    hpp = open(os.path.join(ROOT, "webgraph-big_amd", "host", "bvgraph.hpp")).read()
    for name in ("class HyperBall", "iterate", "neighbourhoodFunction", "sumOfDistances", "sumOfInverseDistances", "modified", "hyperBall"):
        assert name in hpp, name
    mk = open(os.path.join(ROOT, "webgraph-big_amd", "Makefile")).read()
    assert "lib/test_hyperball_mirror" in mk and os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_hyperball_mirror.cpp"))


def test_cli_rejects_what_is_not_built(W, capsys):
    import pytest
    for argv in (["-t", "basename-t", "g"], ["-e", "g"], ["-z", "x:f", "g"], ["-Z", "x:f", "g"], ["g", "gt"]):
        with pytest.raises(SystemExit):
            W.hyperball_main(argv)
        assert "not supported" in capsys.readouterr().err
