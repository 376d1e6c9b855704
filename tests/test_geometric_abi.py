"""CPU: the exact-geometric-centrality entry points (bvg_geometric, bvg_geometric_dev) are declared in include/bvgraph_hip.h, exported by the
library cross-compiled for gfx950 and bound by the ctypes mirror; argument checks, the coefficients spec, the command line and the result
files need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["bvg_geometric", "bvg_geometric_dev"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_geometric[a-z_0-9]*)\s*\(", text))) == NAMES
    assert re.search(r"enum\s*\{\s*BVG_GEO_HARMONIC = 0, BVG_GEO_POWER_LAW = 1, BVG_GEO_EXPONENTIAL = 2, BVG_GEO_TABLE = 3\s*\}", text)
    assert re.search(r"#define BVG_GEO_COUNTERS\s+8\b", text)
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays
    for n in NAMES:                                                             # (the ABI tests of the other analytics match their prefixes)
        assert not n.startswith(("bvg_scc", "bvg_bfs_", "bvg_hyperball_"))


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    sigs = W._abi.geometric_signatures()
    assert sorted(sigs) == NAMES
    L = W.bvgraph._geometric_fns()
    for n in NAMES:
        assert sigs[n] == [vp, C.c_int, C.c_double, vp, u64, i64, i64, vp, vp, vp, u64, C.POINTER(u64), vp] and getattr(L, n).argtypes == sigs[n]
    assert (W.GEO_HARMONIC, W.GEO_POWER_LAW, W.GEO_EXPONENTIAL, W.GEO_TABLE) == (0, 1, 2, 3)
    assert len(W.GEO_COUNTERS) == 8 and W._abi.GEO_COUNTER_WORDS == 8


def test_argument_checks_need_no_device(W):
    """Every refusal is BVG_E_ARG before any device call and writes nothing.  Without a device there is no handle, so each case is
    given with g == NULL as well: the status is the same and no output is touched (tests/test_gpu_geometric.py repeats them on a graph)."""
    L = W.bvgraph._geometric_fns()
    cen = np.full(4, 7, dtype=np.float32); rea = np.full(4, 7, dtype=np.int64); hist = np.full(4, 7, dtype=np.uint64); ctr = np.full(8, 7, dtype=np.uint64)
    hl = C.c_uint64(5)
    table = np.array([0.0, 1.0])
    c, r, h, k = cen.ctypes.data, rea.ctypes.data, hist.ctypes.data, ctr.ctypes.data
    for fn in (L.bvg_geometric, L.bvg_geometric_dev):
        assert fn(None, W.GEO_HARMONIC, 0.0, None, 0, 0, 4, c, r, h, 4, C.byref(hl), k) == W.E_ARG                    # no handle
        assert fn(None, 4, 0.0, None, 0, 0, 4, c, r, h, 4, C.byref(hl), k) == W.E_ARG                                 # unknown kind
        assert fn(None, -1, 0.0, None, 0, 0, 4, c, r, h, 4, C.byref(hl), k) == W.E_ARG
        assert fn(None, W.GEO_TABLE, 0.0, None, 2, 0, 4, c, r, h, 4, C.byref(hl), k) == W.E_ARG                       # a table kind without a table
        assert fn(None, W.GEO_TABLE, 0.0, table.ctypes.data, 0, 0, 4, c, r, h, 4, C.byref(hl), k) == W.E_ARG          # ... of no entries
        assert fn(None, W.GEO_HARMONIC, 0.0, None, 0, 3, 2, c, r, h, 4, C.byref(hl), k) == W.E_ARG                    # from > to
        assert fn(None, W.GEO_HARMONIC, 0.0, None, 0, -1, 2, c, r, h, 4, C.byref(hl), k) == W.E_ARG                   # outside [0, nodes]
        assert fn(None, W.GEO_HARMONIC, 0.0, None, 0, 0, 4, c, r, h, 4, None, k) == W.E_ARG                           # hist without hist_len
    assert hl.value == 5 and (cen == 7).all() and (rea == 7).all() and (hist == 7).all() and (ctr == 7).all()          # nothing was written


def test_python_mirror_refuses_before_the_library(W):
    f = W.bvgraph._geometric_coeffs
    assert f("harmonic") == (W.GEO_HARMONIC, 0.0, None) and f(("power", -1))[:2] == (W.GEO_POWER_LAW, -1.0) and f(("exp", 2))[:2] == (W.GEO_EXPONENTIAL, 2.0)
    kind, _, table = f([0, 1, 1])
    assert kind == W.GEO_TABLE and table.dtype == np.float64 and table.tolist() == [0.0, 1.0, 1.0]
    for bad in ("closeness", ("lin", 1.0), [], np.zeros((2, 2))):
        with pytest.raises(W.IllegalArgumentException):
            f(bad)


def test_coefficients_spec(W):
    p = W.parse_coefficients_spec
    full = "it.unimi.dsi.big.webgraph.algo.LinearGeometricCentrality"
    assert p("HarmonicCoefficients") == "harmonic" and p(full + "$HarmonicCoefficients") == "harmonic" and p(full + ".HarmonicCoefficients") == "harmonic"
    assert p("PowerLawCoefficients(-1.5)") == ("power", -1.5) and p(full + "$PowerLawCoefficients(2)") == ("power", 2.0)
    assert p("ExponentialCoefficients(0.5)") == ("exp", 0.5) and p(full + "$ExponentialCoefficients(1e-1)") == ("exp", 0.1)
    for bad in ("NoSuchCoefficients", "NoSuchCoefficients(1)", "java.lang.String", "HarmonicCoefficients(1)", "PowerLawCoefficients", "PowerLawCoefficients(1,2)",
                "PowerLawCoefficients(x)", "ExponentialCoefficients(1", "some.other.Package$HarmonicCoefficients", ""):
        with pytest.raises(W.IllegalArgumentException):
            p(bad)


def test_command_line(W, tmp_path, capsys):
    with pytest.raises(SystemExit):
        W.geometric_main([])                                                    # four arguments are required
    with pytest.raises(SystemExit):
        W.geometric_main(["base", "HarmonicCoefficients", "c"])
    with pytest.raises(SystemExit):
        W.geometric_main(["base", "NoSuchCoefficients", "c", "r"])              # refused before the graph is loaded
    args = W.bvgraph.geometric_arg_parser().parse_args(["-m", "-T", "8", "base", "PowerLawCoefficients(-1)", "c.bin", "r.bin"])
    assert (args.mapped, args.threads, args.graphBasename, args.coefficientsSpec, args.centralityFilename, args.reachableFilename) == \
        (True, 8, "base", "PowerLawCoefficients(-1)", "c.bin", "r.bin")
    capsys.readouterr()
    with pytest.raises(W.IOException):
        W.geometric_main([str(tmp_path / "no-such-graph"), "HarmonicCoefficients", str(tmp_path / "c"), str(tmp_path / "r")])


def test_result_files_round_trip(W, tmp_path):
    cen = np.array([1.5, 0.0, np.inf, 1 + 1 / 3], dtype=np.float32); rea = np.array([1, 258, (1 << 40) + 3, 0], dtype=np.int64)
    cp, rp = str(tmp_path / "c.bin"), str(tmp_path / "r.bin")
    assert W.store_geometric(W.GeometricResult(cen, rea), cp, rp) == [cp, rp]
    raw = open(cp, "rb").read()
    assert raw[:4] == bytes([0x3F, 0xC0, 0x00, 0x00]) and raw[8:12] == bytes([0x7F, 0x80, 0, 0]) and len(raw) == 16   # 1.5f and +inf as BinIO.storeFloats writes them
    raw = open(rp, "rb").read()
    assert raw[8:16] == bytes([0, 0, 0, 0, 0, 0, 1, 2]) and raw[16:24] == bytes([0, 0, 1, 0, 0, 0, 0, 3]) and len(raw) == 32   # big-endian longs
    c, r = W.load_geometric(cp, rp)
    assert c.dtype == np.float32 and r.dtype == np.int64 and np.array_equal(c, cen) and np.array_equal(r, rea)


def test_mirrors_expose_the_result(W):
    for name in ("linear_geometric_centrality", "linearGeometricCentrality", "linear_geometric_centrality_dev"):
        assert hasattr(W.BVGraph, name), name
    # closeness and Lin from a sum-of-distances run, by the formulas bvg_hyperball_centrality documents
    r = W.GeometricResult(np.array([4.0, 0.0, 2.0], dtype=np.float32), np.array([3, 1, 2]), np.array([3, 2, 1], dtype=np.uint64), {"passes": 1}, (5, 8), (W.GEO_POWER_LAW, 1.0))
    assert r.closeness().tolist() == [0.25, 0.0, 0.5] and r.lin().tolist() == [2.25, 1.0, 2.0]
    assert r.neighbourhood_function().tolist() == [3, 5, 6] and r.counters["passes"] == 1 and "[5, 8)" in repr(r)
    with pytest.raises(W.IllegalStateException):
        W.GeometricResult(np.zeros(1, np.float32), np.ones(1, np.int64), coefficients=(W.GEO_HARMONIC, 0.0)).closeness()
    hpp = open(os.path.join(ROOT, "webgraph-big_amd", "host", "bvgraph.hpp")).read()
    for name in ("class LinearGeometricCentrality", "struct HarmonicCoefficients", "struct PowerLawCoefficients", "struct ExponentialCoefficients",
                 "linearGeometricCentrality(const Coeffs& coeffs)", "const std::vector<double>& table", "void compute()", "std::vector<float> centrality",
                 "std::vector<int64_t> reachable"):
        assert name in hpp, name
