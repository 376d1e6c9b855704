"""GPU: the graph product through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: composeGraphs) driven by a compiled C++ program
on cnr-2000; what it prints against the model (tests/compose_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import compose_model as CM
from conftest import CNR, ROOT
from test_gpu_transform_cpp import chk

pytestmark = pytest.mark.gpu


def test_cpp_mirror_composes_cnr2000(cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_compose_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_compose_mirror"])
    out = subprocess.run([exe, CNR], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    deg, succ = cnr_csr
    g = (np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ)
    off, adj = CM.cached("cnr_square", lambda: CM.compose(g, g))
    assert lines[0] == "nodes 325557 arcs 34174066 products 96065788 report_arcs 34174066 rows %d" % int(np.sum(CM.bounds(g, g) > 0))
    assert lines[1] == "off_chk %016x adj_chk %016x" % (chk(off), chk(adj))
    assert lines[2] == "mixed_equal 1"
    assert lines[3] == "refusal invalid_argument" and lines[4] == "refusal invalid_argument" and lines[5] == "OK"
