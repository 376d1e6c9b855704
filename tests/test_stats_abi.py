"""CPU: the graph-statistics entry points (bvg_stats_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for
gfx950 and bound by the ctypes mirror; argument checks, the command line and the result files need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["bvg_stats_close", "bvg_stats_compute", "bvg_stats_distribution", "bvg_stats_get", "bvg_stats_indegrees", "bvg_stats_indegrees_dev"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_stats[a-z_0-9]*)\s*\(", text))) == NAMES
    assert re.search(r"#define BVG_STATS_KEEP_INDEGREES 1u", text) and re.search(r"#define BVG_STATS_OUT\s+0\b", text) and re.search(r"#define BVG_STATS_IN\s+1\b", text)
    assert sorted(set(re.findall(r"#define (BVG_STATS_\w+)", text))) == ["BVG_STATS_IN", "BVG_STATS_KEEP_INDEGREES", "BVG_STATS_OUT"]
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.stats_signatures()
    assert sorted(sigs) == NAMES
    L = W.bvgraph._stats_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert C.sizeof(W.StatsSummary) == 656 and W.StatsSummary.log_delta.offset == 18 * 8 and W.StatsSummary.min_outdegree.offset == 80
    assert (W._abi.STATS_KEEP_INDEGREES_FLAG, W._abi.STATS_OUT, W._abi.STATS_IN) == (1, 0, 1)


def test_argument_checks_need_no_device(W):
    L = W.bvgraph._stats_fns()
    h = C.c_void_p(0x1234)
    assert L.bvg_stats_compute(None, 0, C.byref(h)) == W.E_ARG                  # no graph
    assert L.bvg_stats_compute(None, 2, C.byref(h)) == W.E_ARG                  # unknown flag bit
    assert L.bvg_stats_compute(None, 0, None) == W.E_ARG                        # no out
    assert h.value == 0x1234                                                    # nothing was written
    sm = W.StatsSummary(nodes=77)
    assert L.bvg_stats_get(None, C.byref(sm)) == W.E_ARG and sm.nodes == 77
    ln = C.c_uint64(5); out = np.full(4, 9, dtype=np.uint64); ind = np.full(4, 9, dtype=np.int64)
    for which in (0, 1, 2, -1):
        assert L.bvg_stats_distribution(None, which, out.ctypes.data, 4, C.byref(ln)) == W.E_ARG
    for fn in (L.bvg_stats_indegrees, L.bvg_stats_indegrees_dev):
        assert fn(None, 0, 4, ind.ctypes.data) == W.E_ARG
    assert ln.value == 5 and (out == 9).all() and (ind == 9).all()
    L.bvg_stats_close(None)                                                     # a no-op


def test_mirrors_expose_the_result(W):
    assert hasattr(W.BVGraph, "stats")
    for name in ("GraphStats", "java_double_str", "store_stats", "stats_main", "StatsSummary"):
        assert hasattr(W, name), name
    hpp = open(os.path.join(ROOT, "webgraph-big_amd", "host", "bvgraph.hpp")).read()
    for name in ("class GraphStats", "stats(bool keepIndegrees", "outdegreeDistribution()", "indegreeDistribution()", "indegrees(int64_t from", "bvg_stats_summary summary"):
        assert name in hpp, name
    assert "lib/test_stats_mirror" in open(os.path.join(ROOT, "webgraph-big_amd", "Makefile")).read()


def test_command_line(W, tmp_path, capsys):
    with pytest.raises(SystemExit):
        W.stats_main([])                                                        # the basename is required
    with pytest.raises(SystemExit):
        W.stats_main(["--no-such-option", "x"])
    ap = W.bvgraph.stats_arg_parser()
    args = ap.parse_args(["-s", "base", "out"])
    assert (args.save_degrees, args.basename, args.results_basename) == (True, "base", "out")
    args = ap.parse_args(["base"])
    assert (args.save_degrees, args.basename, args.results_basename) == (False, "base", None)
    assert "Java-serialised" in ap.format_help()
    capsys.readouterr()
    with pytest.raises(W.IOException):
        W.stats_main([str(tmp_path / "no-such-graph")])


HAND = dict(nodes=4, arcs=6, loops=1, dangling=1, terminal=1, num_gaps=5, tot_gap=11, tot_loc=9, min_outdegree=0, min_outdegree_node=3, max_outdegree=3,
            max_outdegree_node=0, min_indegree=1, min_indegree_node=3, max_indegree=2, max_indegree_node=2)
HAND_TEXT = ("nodes=4\narcs=6\nloops=1\nsuccessoravggap=2.200\navglocality=1.500\nminoutdegree=0\nmaxoutdegree=3\nminoutdegreenode=3\nmaxoutdegreenode=0\n"
             "dangling=1\nterminal=1\npercdangling=25.0\navgoutdegree=1.5\nsuccessorlogdeltastats=3,2\nsuccessoravglogdelta=0.661\n"
             "minindegree=1\nmaxindegree=2\nminindegreenode=3\nmaxindegreenode=2\navgindegree=1.5\n")
HAND_MORE = "buckets=2\npercbuckets=50.0\nsccs=5\nmaxsccsize=5\npercmaxscc=125.0\nminsccsize=1\npercminscc=25.0\n"


def test_result_files(W, tmp_path):
    gs = W.GraphStats([3, 2], [1, 1, 1, 1], [0, 2, 2], np.array([1, 2, 2, 1], dtype=np.int64), **HAND)
    base = str(tmp_path / "r")
    assert W.store_stats(gs, base) == [base + ".stats", base + ".outdegree", base + ".indegree"]
    assert open(base + ".stats", "rb").read() == HAND_TEXT.encode()
    assert open(base + ".outdegree").read() == "1\n1\n1\n1\n" and open(base + ".indegree").read() == "0\n2\n2\n"
    assert not os.path.exists(base + ".sccdistr") and not os.path.exists(base + ".indegrees")
    base2 = str(tmp_path / "q")
    paths = W.store_stats(gs, base2, buckets=np.array([True, False, True, False]), scc_sizes=[5, 1, 1, 3, 1], save_degrees=True, outdegrees=[3, 2, 1, 0])
    assert paths == [base2 + e for e in (".stats", ".outdegree", ".indegree", ".sccdistr", ".outdegrees", ".indegrees")]
    assert open(base2 + ".stats", "rb").read() == (HAND_TEXT + HAND_MORE).encode()
    assert open(base2 + ".sccdistr").read() == "5\t1\n3\t1\n1\t3\n"
    assert open(base2 + ".outdegrees").read() == "3\n2\n1\n0\n" and open(base2 + ".indegrees").read() == "1\n2\n2\n1\n"
    assert gs.properties(buckets=2) == HAND_TEXT + HAND_MORE[:HAND_MORE.index("sccs")]
    with pytest.raises(W.IllegalArgumentException):
        W.store_stats(gs, base2, save_degrees=True)                             # no outdegrees given


def test_big_decimal_rounding_and_empty_graph(W):
    # scale 3, HALF_EVEN: 0.0005 -> 0.000, 0.0015 -> 0.002, 0.0025 -> 0.002; sums beyond 64 bits stay exact
    for tot, want in ((1, "0.000"), (3, "0.002"), (5, "0.002"), (7, "0.004"), ((1 << 64) * 2000 + 1001, "18446744073709551616.500")):
        kv = dict(l.split("=", 1) for l in W.GraphStats(**dict(HAND, tot_gap=tot, num_gaps=2000)).properties().splitlines())
        assert kv["successoravggap"] == want, tot
    e = W.GraphStats()
    assert (e.min_outdegree, e.min_indegree) == ((1 << 63) - 1,) * 2 and list(e.outdegree_distribution) == [0] and e.indegrees is None
    text = e.properties()
    assert "minoutdegree=9223372036854775807\n" in text and "percdangling=NaN\n" in text and "successorlogdeltastats=\nsuccessoravglogdelta=0\n" in text
    assert text.startswith("nodes=0\narcs=0\nloops=0\nsuccessoravggap=0.000\navglocality=0.000\n")
