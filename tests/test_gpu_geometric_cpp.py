"""GPU: LinearGeometricCentrality through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program
(tests/cpp/test_geometric_mirror.cpp), on a hand graph with every node as a source and on cnr-2000 with the sources [0, 64): what it
prints against the numpy model (tests/geometric_model.py), by the rule of tests/test_gpu_geometric.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import geometric_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(basename, spec, *sources):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_geometric_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_geometric_mirror"])
    out = subprocess.run([exe, basename, spec] + [str(s) for s in sources], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict((l.split(" ", 1) + [""])[:2] for l in out.stdout.splitlines() if l)
    m = re.fullmatch(r"sources=(\d+) words=(\d+) passes=(\d+)", lines["OK"])
    assert m, out.stdout
    cen = np.array([int(v, 16) for v in lines["C"].split()], dtype=np.uint32).view(np.float32)
    return cen, np.array(lines["R"].split(), dtype=np.int64), np.array(lines["H"].split(), dtype=np.uint64), [int(v) for v in m.groups()]


def test_cpp_mirror_on_a_hand_graph(W, tools, tmp_path):
    n, arcs = M.HAND["star"]
    off, adj = M.csr_of(n, arcs)
    tools.store((off, adj)).write(str(tmp_path / "star"))
    counts = M.distance_counts(off, adj, range(n))
    for arg, spec in (("harmonic", "harmonic"), ("power:1", ("power", 1)), ("exp:0.5", ("exp", 0.5)), ("table:0,1,1", [0, 1, 1])):
        cen, rea, hist, (k, words, passes) = _run(str(tmp_path / "star"), arg)
        assert (k, words, passes) == (n, 1, 1)
        assert np.array_equal(rea, M.reachable(counts)) and np.array_equal(hist, M.histogram(counts))
        assert np.array_equal(cen, M.exact(counts, M.coefficient(spec)))        # halves, quarters and integers: exact in float
    assert rea.tolist() == [9, 1, 1, 9, 1, 1, 1, 1, 1] and hist.tolist() == [9, 9, 7]   # the centre and leaf 3 reach everything


def test_cpp_mirror_on_cnr2000(cnr_csr):
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.int64); off[1:] = np.cumsum(deg)
    counts = M.distance_counts_pull(off, succ, range(64))
    cen, rea, hist, (k, words, passes) = _run(os.path.join(ROOT, "tests", "golden", "cnr-2000"), "harmonic", 0, 64)
    assert (k, words, passes) == (64, 1, 1)
    assert np.array_equal(rea, M.reachable(counts)) and np.array_equal(hist, M.histogram(counts))
    assert M.within_one_spacing(cen, M.exact(counts, M.coefficient("harmonic")))
