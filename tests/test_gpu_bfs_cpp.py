"""GPU: ParallelBreadthFirstVisit through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program on
cnr-2000, checked against the CPU breadth-first search of tests/test_gpu_bfs.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, CNR
from test_gpu_bfs import cpu_bfs, cpu_visit_all

pytestmark = pytest.mark.gpu


def _chk(W, v):
    return sum(W.arc_mix(i, int(c) % (1 << 64)) for i, c in enumerate(v)) % (1 << 64)


def test_cpp_mirror_visits_of_cnr2000(W, cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_bfs_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_bfs_mirror"])
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.int64); off[1:] = np.cumsum(deg)
    starts = [100000, 325556, 3]
    out = subprocess.run([exe, CNR] + [str(s) for s in starts], capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stdout + out.stderr
    visits = re.findall(r"VISIT start=(\d+) visited=(\d+) maxdist=(-?\d+) far=(\d+) queue=([0-9a-f]+) cuts=([0-9a-f]+) dist=([0-9a-f]+) parents=([0-9a-f]+)", out.stdout)
    assert [int(v[0]) for v in visits] == starts, out.stdout
    for v, s in zip(visits, starts):
        queue, cuts, dist, parent = cpu_bfs(off, succ, s)
        assert [int(x) for x in v[1:4]] == [len(queue), len(cuts) - 2, int(queue[-1])]
        assert [int(x, 16) for x in v[4:]] == [_chk(W, queue), _chk(W, cuts), _chk(W, dist), _chk(W, parent)]
    m = re.search(r"ALL rounds=(\d+) marker=([0-9a-f]+)", out.stdout)
    assert m, out.stdout
    marker, rnd, _, _, _ = cpu_visit_all(off, succ, False)
    assert (int(m.group(1)), int(m.group(2), 16)) == (rnd + 1, _chk(W, marker))
