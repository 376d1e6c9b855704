"""GPU: StronglyConnectedComponents through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp) driven by a compiled C++ program
on cnr-2000: the count, the largest size and the bucket counts against the known answers (tests/scc_cases.py: CNR)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from scc_cases import CNR

pytestmark = pytest.mark.gpu


def test_cpp_mirror_scc_of_cnr2000():
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_scc_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_scc_mirror"])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "cnr-2000")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"OK nodes=(\d+) count=(\d+) largest=(\d+) singletons=(\d+) bucket_components=(\d+) bucket_nodes=(\d+)", out.stdout)
    assert m, out.stdout
    assert [int(v) for v in m.groups()] == [CNR["nodes"], CNR["components"], CNR["largest"][0], CNR["singletons"], CNR["bucket_components"], CNR["bucket_nodes"]]
