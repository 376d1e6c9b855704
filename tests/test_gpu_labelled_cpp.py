"""GPU: the labelled transforms through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: LabelledGraph, transposeLabelled, unionLabelled,
symmetrizeLabelled, filterLabelledArcs) driven by a compiled C++ program on cnr-2000 with the labels (31 x + y) mod 2^13; what it prints against
the model (tests/labelled_model.py) and the CPU label writer."""
import os
import subprocess

import numpy as np
import pytest

import labelled_model as LM
from conftest import CNR, ROOT
from test_gpu_transform_cpp import chk

pytestmark = pytest.mark.gpu


def line(name, g, kind=2, width=13):
    return "%s nodes %d arcs %d kind %d width %d off_chk %016x adj_chk %016x lab_chk %016x" % (name, LM.nodes(g), len(g[1]), kind, width, chk(g[0]), chk(g[1]), chk(g[2]))


def test_cpp_mirror_labelled_transforms_of_cnr2000(cnr_csr, tools):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_labelled_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_labelled_mirror"])
    out = subprocess.run([exe, CNR], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    deg, succ = cnr_csr
    off = np.concatenate([[0], np.cumsum(deg.astype(np.int64))])
    g = LM.make(off, succ, np.zeros(len(succ)))
    g = LM.make(off, succ, (31 * LM.sources(g) + succ) % (1 << 13))
    t = LM.transpose(g)
    assert lines[0] == line("source", g)
    assert lines[1] == line("transpose", t)
    assert lines[2] == "twice_equal 1 underlying_equal 1"
    assert lines[3] == line("symmetrize_min", LM.union(g, t, LM.MIN))
    assert lines[4] == "union_is_symmetrize 1"
    assert lines[5] == line("lower_bound_4096", LM.filter(g, LM.LOWER_BOUND, lower_bound=4096))
    assert lines[6] == line("no_loops", LM.filter(g, LM.NO_LOOPS))
    sl = tools.store_labels(2, 13, g[2], g[0])
    assert lines[7] == "labels bytes %d stream_chk %016x offsets_chk %016x" % (len(sl.stream), chk(sl.stream), chk(sl.offsets))
    assert lines[8:] == ["refusal invalid_argument", "refusal unsupported", "refusal invalid_argument", "refusal invalid_argument", "OK"]
