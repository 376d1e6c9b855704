"""GPU: the transforms through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: identityGraph, graphFromCSR, mapGraph, filterArcs,
transposeGraph, symmetrizeGraph, simplifyGraph, unionGraphs, the three permutations) driven by a compiled C++ program on cnr-2000; what
it prints against the model (tests/transform_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import transform_model as M
from conftest import CNR, ROOT

pytestmark = pytest.mark.gpu


def chk(values):
    """The program's checksum of an array of 64-bit words: the sum of (v[i] + 1) * (2 i + 1) modulo 2^64."""
    v = np.asarray(values).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum((v + np.uint64(1)) * (np.uint64(2) * np.arange(len(v), dtype=np.uint64) + np.uint64(1)), dtype=np.uint64))


def test_cpp_mirror_transforms_of_cnr2000(cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_transform_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_transform_mirror"])
    out = subprocess.run([exe, CNR], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    deg, succ = cnr_csr
    g = (np.concatenate([[0], np.cumsum(deg.astype(np.int64))]), succ)
    assert lines[0] == "nodes 325557 arcs 3216152 identity 1 from_csr 1"
    assert lines[1] == "transpose_equal 1 symmetrize_equal 1 union_equal 1 simplify_loops 0 simplify_symmetric 1 simplify_is_filter 1"
    # the permutations as their first and last entries and their sums would say little: the whole arrays, through one checksum
    lex = M.permutation_of_csr(*g, False)
    words = lines[2].split()
    assert words[0] == "lex_chk" and words[2] == "gray_chk" and words[4] == "random_chk"
    assert words[1] == "%016x" % chk(lex)
    assert words[3] == "%016x" % chk(M.permutation_of_csr(*g, True))
    assert words[5] == "%016x" % chk(M.random_permutation(len(deg), 42))
    want = M.map_graph(*g, lex)
    assert lines[3].startswith("mapped nodes 325557 arcs %d off_chk %016x adj_chk %016x " % (len(want[1]), chk(want[0]), chk(want[1])))
    assert " map_back 1 store_equal 1 graph_bytes " in lines[3]
    assert lines[4] == "refusal invalid_argument" and lines[5] == "refusal invalid_argument" and lines[6] == "OK"
