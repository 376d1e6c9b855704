"""GPU: graph statistics through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program on cnr-2000:
the printed summary, the heads of both distributions and a checksum of the indegrees against the model (tests/stats_model.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import stats_model as SM
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mirror_stats_of_cnr2000(cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_stats_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_stats_mirror"])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "cnr-2000")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.uint64); off[1:] = np.cumsum(deg, dtype=np.uint64)
    m = SM.model(off, succ)
    od, idist, ind = m["outdegree_distribution"], m["indegree_distribution"], m["indegrees"]
    mix = sum(int(v) * (x + 1) for x, v in enumerate(ind.tolist())) % (1 << 64)
    want = ["OK nodes=%d arcs=%d loops=%d dangling=%d terminal=%d num_gaps=%d tot_gap=%d:%d tot_loc=%d:%d"
            % (m["nodes"], m["arcs"], m["loops"], m["dangling"], m["terminal"], m["num_gaps"], m["tot_gap"] >> 64, m["tot_gap"] & (2 ** 64 - 1), m["tot_loc"] >> 64,
               m["tot_loc"] & (2 ** 64 - 1)),
            "OUT min=%d@%d max=%d@%d len=%d head=%d,%d,%d" % (m["min_outdegree"], m["min_outdegree_node"], m["max_outdegree"], m["max_outdegree_node"], len(od), od[0], od[1], od[2]),
            "IN min=%d@%d max=%d@%d len=%d head=%d,%d,%d sum=%d mix=%d" % (m["min_indegree"], m["min_indegree_node"], m["max_indegree"], m["max_indegree_node"], len(idist),
                                                                         idist[0], idist[1], idist[2], int(ind.sum()), mix),
            "BINS " + ",".join(str(v) for v in m["log_delta"])]
    assert out.stdout.splitlines() == want, out.stdout
    assert re.search(r"IN min=1@325468 max=18235@205307 ", out.stdout)
