"""GPU: the labelled graph product through the C++ host mirror (webgraph-big_amd/host/bvgraph.hpp: composeLabelled) driven by a compiled C++
program: the reference's own case under the five semirings and one row of 300 lists of the same successor with every tier forced; what it
prints against the model (tests/lcompose_model.py)."""
import os
import subprocess

import pytest

import lcompose_model as LC
from conftest import ROOT

pytestmark = pytest.mark.gpu

LISTS = 300


def line(name, g, kind, width, rows):
    arcs = " ".join("%d>%d:%d" % (x, z, v) for x, r in enumerate(LC.rows_of(g)) for z, v in r)
    return "%s nodes %d arcs %d kind %d width %d rows %d %d %d : %s" % (name, len(g[0]) - 1, len(g[1]), kind, width, rows[0], rows[1], rows[2], arcs)


@pytest.mark.parametrize("tier", [0, 1, 2])
def test_cpp_mirror_composes_labelled_graphs(tier):
    exe = os.path.join(ROOT, "webgraph-big_amd", "lib", "test_lcompose_mirror")
    if not os.path.exists(exe):                                                # (build() makes it; only a tree built before it existed lacks it)
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "webgraph-big_amd"), "lib/test_lcompose_mirror"])
    env = dict(os.environ, BVG_TEST_KNOBS="1", BVG_COMPOSE_TIER=str(tier))
    out = subprocess.run([exe, str(LISTS)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    ref = LC.from_rows([[(1, 2), (2, 10), (3, 1)], [(2, 4)], [], [(2, 1)]])
    a = LC.from_rows([[(6 + i, i % 3 + 1) for i in range(LISTS)]], 6 + LISTS)
    b = LC.from_rows([[] for _ in range(6)] + [[(5, i + 1)] for i in range(LISTS)])
    lim = [int(v) for v in lines[10].split()[1:]]
    assert lines[10].startswith("limits ") and 2 <= lim[0] < lim[1]
    small = [0, 0, 0]; small[tier] = 1                                         # the reference's one row (bound 2) goes where it is forced
    big = [0, 0, 0]; big[max(tier, 0 if LISTS <= lim[0] else 1 if LISTS <= lim[1] else 2)] = 1
    for s in LC.SEMIRINGS:
        assert lines[s] == line("reference_%d" % s, LC.from_rows(LC.compose_rows(ref, ref, s)), LC.GAMMA, 0, small)
        assert lines[5 + s] == line("same_key_%d" % s, LC.from_rows(LC.compose_rows(a, b, s)), LC.FIXED, 31, big)
    assert LC.compose(a, b, LC.PLUS_TIMES, LC.FIXED, 3) == ("range", 1, (0, 5))
    assert lines[11] == "refusal invalid_argument out_of_range 1 first 0 5"
    assert lines[12:] == ["refusal invalid_argument"] * 3 + ["OK"]
