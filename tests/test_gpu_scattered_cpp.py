"""GPU: scattered arc lists through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: parseScatteredArcs) driven by a compiled C++
program (tests/cpp/test_scattered_mirror.cpp); what it prints against the model (tests/scattered_model.py)."""
import os
import subprocess

import pytest

import scattered_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

KNOWN = [2, -1, 7]
CASES = [("", b"-1 15\n15 2\n2 -1\nOOPS!\n-1 2"), ("SL", b"# c\n5 5\n5 6 x\r\n7\n-9223372036854775808 5\n"), ("K", b"2 -1\n3 2\n2 3\n7 7\n"), ("X", b"1 2\n\n3 X\n")]
CODES = {None: 0, "bad_source": 1, "bad_target": 2, "no_target": 3, "too_large": 4, "trailing": 5, "unknown_source": 6, "unknown_target": 7}


def test_cpp_mirror_parses_scattered_arcs():
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_scattered_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_scattered_mirror"])
    out = subprocess.run([exe] + [flags + ":" + text.decode().replace("\n", "|") for flags, text in CASES], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    want = []
    for flags, text in CASES:
        r = M.parse(text, "S" in flags, "L" in flags, KNOWN if "K" in flags else None)
        rep = r["report"]
        if "X" in flags and rep["first_reason"]:
            want.append("refusal -4 %d %d %d" % (CODES[rep["first_reason"]], rep["first_line"], rep["first_byte"]))
            continue
        off, adj = M.csr(r["nodes"], r["arcs"])
        want.append("nodes %d arcs %d ids" % (r["nodes"], len(r["arcs"])) + "".join(" %d" % v for v in r["ids"]))
        want.append("off" + "".join(" %d" % v for v in off))
        want.append("adj" + "".join(" %d" % v for v in adj))
        want.append("report " + " ".join(str(rep[k]) for k in M.COUNTS + ("first_byte", "first_line")) + " %d" % CODES[rep["first_reason"]])
    assert out.stdout.splitlines() == want + ["OK"]
