"""CPU: the breadth-first-visit entry points (bvg_bfs_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for
gfx950 and bound by the ctypes mirror; the Python and C++ mirrors expose the visit object.  No compute calls: there is no GPU here."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ["bvg_bfs_clear", "bvg_bfs_close", "bvg_bfs_counters", "bvg_bfs_create", "bvg_bfs_get", "bvg_bfs_get_dev", "bvg_bfs_info", "bvg_bfs_visit", "bvg_bfs_visit_all"]


def _header():
    return open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read()


def test_header_declares_the_visit_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bvg_bfs_[a-z_0-9]+)\s*\(", text)))
    assert declared == NAMES
    assert re.search(r"#define BVG_BFS_PARENT 1u", text) and re.search(r"#define BVG_BFS_COUNTERS 8\b", text)
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    sigs = W._abi.bfs_signatures()
    assert sorted(sigs) == NAMES
    L = W.bvgraph._bfs_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert W.BFS_PARENT == 1 and len(W.BFS_COUNTERS) == 8 and W._abi.BFS_COUNTER_WORDS == 8
    assert lib.bvg_bfs_create(None, 0, None) == W.E_ARG and lib.bvg_bfs_visit(None, C.c_int64(0), None) == W.E_ARG   # argument checks need no device
    lib.bvg_bfs_close.restype = None
    lib.bvg_bfs_close(None)


def test_mirrors_expose_the_visit_object(W):
    for name in ("clear", "visit", "visit_all", "round", "queue", "cut_points", "marker", "dist", "max_distance", "node_at_max_distance", "close", "__enter__", "__exit__"):
        assert hasattr(W.BreadthFirstVisit, name), name
    assert hasattr(W.BVGraph, "breadth_first_visit")
    hpp = open(os.path.join(ROOT, "webgraph-big_amd", "host", "bvgraph.hpp")).read()
    for name in ("class ParallelBreadthFirstVisit", "visitAll", "maxDistance", "nodeAtMaxDistance", "cutPoints", "breadthFirstVisit"):
        assert name in hpp, name
