"""GPU: text graphs through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: loadASCIIGraph, loadArcList, storeASCIIGraph,
storeArcList) driven by a compiled C++ program on cnr-2000; what it prints against the golden text and the golden .graph."""
import os
import subprocess

import pytest

from conftest import CNR, ROOT

pytestmark = pytest.mark.gpu


def fnv(data):
    h = 1469598103934665603
    for c in data:
        h = ((h ^ c) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_cpp_mirror_text_round_trip_of_cnr2000(cnr_golden):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_text_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_text_mirror"])
    out = subprocess.run([exe, CNR], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    graph = open(CNR + ".graph", "rb").read()
    arcs_bytes = sum(len(b"%d" % (x + 5)) * len(l) + sum(len(b"%d" % (int(t) + 5)) for t in l) + 2 * len(l) for x, l in enumerate(cnr_golden))
    assert lines[0] == "nodes 325557 arcs 3216152"
    assert lines[1].split()[:2] == ["ascii_bytes", "22248688"] and lines[1].endswith("pieces_equal 1")
    assert lines[2].split()[:2] == ["arcs_bytes", str(arcs_bytes)]
    assert lines[3] == "round_trips 1 store_equal 1 graph_bytes %d graph_fnv %016x" % (len(graph), fnv(graph))       # the parsed text, stored: cnr-2000.graph
    assert lines[4] == "refusal -1 5 3 8" and lines[5] == "refusal -4 7 2 5" and lines[6] == "OK"
