"""GPU: ConnectedComponents through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program, on
cnr-2000 cut into blocks of 1024 nodes (arcs x -> y with x // 1024 == y // 1024), checked against a CPU union-find."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_components import _cut, cpu_components, sorted_by_size

pytestmark = pytest.mark.gpu


def _label_chk(W, v):
    return sum(W.arc_mix(i, int(c)) for i, c in enumerate(v)) % (1 << 64)


def test_cpp_mirror_components_of_cut_cnr2000(W, tools, cnr_csr, tmp_path):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_components_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_components_mirror"])
    deg, succ = cnr_csr
    n = len(deg)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    off, adj, s = _cut(src, succ, n, 1024)
    st = tools.store((off, adj), W.default_params(min_interval_length=3), threads=4)
    st.write(str(tmp_path / "cut"))
    out = subprocess.run([exe, str(tmp_path / "cut")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"OK nodes=(\d+) count=(\d+) chk=([0-9a-f]+) sizes_chk=([0-9a-f]+) sorted_chk=([0-9a-f]+) sorted_sizes_chk=([0-9a-f]+)", out.stdout)
    assert m, out.stdout
    k, comp, sizes = cpu_components(n, s, adj)
    c2, s2 = sorted_by_size(comp, sizes)
    assert (int(m.group(1)), int(m.group(2))) == (n, k)
    assert [int(m.group(i), 16) for i in (3, 4, 5, 6)] == [_label_chk(W, v) for v in (comp, sizes, c2, s2)]
