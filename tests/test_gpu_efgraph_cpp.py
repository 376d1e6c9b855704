"""GPU: EFGraph through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program on cnr-2000: BVGraph ->
device store -> EFGraph; the printed sizes, checksums, scan and skipTo answers against the golden lists and the model's formulas."""
import os
import subprocess

import numpy as np
import pytest

import efgraph_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_mirror_efgraph_of_cnr2000(cnr_golden, cnr_csr):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_efgraph_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_efgraph_mirror"])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "cnr-2000")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    deg, succ = cnr_csr
    n = len(deg)
    bits = int(sum(M.record_bits(int(d), n, 8) * int(c) for d, c in zip(*np.unique(deg, return_counts=True))))
    mix = int(np.sum(succ.astype(np.uint64) * np.arange(1, len(succ) + 1, dtype=np.uint64), dtype=np.uint64))
    key = np.array([M.arc_mix(x, 1) - M.arc_mix(x, 0) for x in range(n)], dtype=np.uint64)                    # k1 of every node
    k0 = np.array([M.arc_mix(x, 0) for x in range(n)], dtype=np.uint64)
    src = np.repeat(np.arange(n), deg)
    chk = int(np.sum(key[src] * succ.astype(np.uint64) + k0[src], dtype=np.uint64))
    nodes = [x for x in range(0, n, 997) for _ in range(0, n + 1, n // 7)]
    bounds = [b for _ in range(0, n, 997) for b in range(0, n + 1, n // 7)]
    want = [(lambda a, i: int(a[i]) if i < len(a) else -1)(cnr_golden[x], int(np.searchsorted(cnr_golden[x], b))) for x, b in zip(nodes, bounds)]
    skipmix = sum((v % (1 << 64)) * (i + 1) for i, v in enumerate(want)) % (1 << 64)
    assert out.stdout.splitlines() == [
        "OK nodes=%d arcs=%d bytes=%d bits=%d mix=%d" % (n, len(succ), 8 * (bits // 64 + 1), bits, mix),
        "SCAN nodes=%d arcs=%d chk=%d outdegree0=%d" % (n, len(succ), chk, deg[0]),
        "SKIP queries=%d agree=%d mix=%d" % (len(want), len(want), skipmix)], out.stdout
