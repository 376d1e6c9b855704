"""GPU: HyperBall through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program on cnr-2000 with
log2m 6, against the Python mirror (bit for bit) and the numpy model of tests/hyperball_model.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import hyperball_model as M
from conftest import ROOT, CNR

pytestmark = pytest.mark.gpu


def test_cpp_mirror_agrees_with_python_on_cnr2000(W, cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_hyperball_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_hyperball_mirror"])
    log2m, seed, bound = 6, 5, 8
    out = subprocess.run([exe, CNR, str(log2m), str(seed), str(bound)], capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stdout + out.stderr
    run = re.search(r"RUN iteration=(-?\d+) modified=(\d+)", out.stdout)
    nf = re.search(r"^NF((?: [0-9a-f]{16})+)$", out.stdout, flags=re.M)
    st = re.search(r"STATE registers=([0-9a-f]+) sod=([0-9a-f]+) sid=([0-9a-f]+) count0=([0-9a-f]+)", out.stdout)
    assert run and nf and st, out.stdout
    cpp_nf = np.array([int(x, 16) for x in nf.group(1).split()], dtype=np.uint64).view(np.float64)

    def chk(values):                                                           # the sum of (index + 1) * value, modulo 2^64
        v = np.asarray(values).astype(np.uint64)
        return int((np.arange(1, len(v) + 1, dtype=np.uint64) * v).sum(dtype=np.uint64))

    g = W.BVGraph.load(CNR)
    with g.hyperball(log2m, seed=seed, sum_of_distances=True, harmonic=True) as hb:
        hb.run(bound)
        assert (int(run.group(1)), int(run.group(2))) == (hb.iteration, hb.modified())
        assert np.array_equal(cpp_nf, hb.neighbourhood_function)               # the same library: bit for bit
        regs = hb.registers()
        assert int(st.group(2), 16) == chk(hb.sum_of_distances().view(np.uint32)) and int(st.group(3), 16) == chk(hb.harmonic_centrality().view(np.uint32))
        assert int(st.group(4), 16) == int(np.array([hb.count(0)]).view(np.uint64)[0])
    deg, succ = cnr_csr
    off = np.zeros(len(deg) + 1, dtype=np.uint64); off[1:] = np.cumsum(deg)
    model = M.HyperBallModel(off, np.asarray(succ, dtype=np.int64), log2m, seed=seed)
    model.run(bound)
    assert np.array_equal(regs, model.regs) and int(run.group(2)) == model.modified and int(run.group(1)) == model.iteration
    assert int(st.group(1), 16) == chk(model.regs.reshape(-1))
    assert np.all(np.abs(cpp_nf - np.asarray(model.nf)) <= len(deg) * 2.0 ** -52 * np.asarray(model.nf))
