"""GPU: random chains of three labelled transforms against the model (tests/labelled_model.py), and the label stream of every result against
the CPU writer (tooling.store_labels).  BVG_LABELLED_FUZZ=<n> cases (default 40), seeded."""
import os

import numpy as np
import pytest

import labelled_model as LM

pytestmark = pytest.mark.gpu

GAMMA, FIXED = 1, 2
CASES = int(os.environ.get("BVG_LABELLED_FUZZ", "40"))


def _step(W, rng, lg, g, other_lg, other):
    """One random operation on the resident graph and on the model."""
    op = rng.choice(["transpose", "union", "union_rev", "symmetrize", "lower_bound", "no_loops", "same_class", "different_class"])
    strategy = str(rng.choice([LM.KEEP_FIRST, LM.MIN, LM.MAX]))
    n = LM.nodes(g)
    if op == "transpose":
        return W.transpose_labelled(lg), LM.transpose(g), op
    if op == "union":
        return W.union_labelled(lg, other_lg, strategy), LM.union(g, other, strategy), op + " " + strategy
    if op == "union_rev":
        return W.union_labelled(other_lg, lg, strategy), LM.union(other, g, strategy), op + " " + strategy
    if op == "symmetrize":
        return W.symmetrize_labelled(lg, strategy), LM.symmetrize(g, strategy), op + " " + strategy
    if op == "lower_bound":
        bound = int(rng.integers(-1, int(g[2].max()) + 2)) if len(g[2]) else 0
        return W.filter_labelled_arcs(lg, "LOWER_BOUND", lower_bound=bound), LM.filter(g, LM.LOWER_BOUND, lower_bound=bound), "%s %d" % (op, bound)
    if op == "no_loops":
        return W.filter_labelled_arcs(lg, "NO_LOOPS"), LM.filter(g, LM.NO_LOOPS), op
    cls = rng.integers(0, 3, n)
    kind = LM.SAME_CLASS if op == "same_class" else LM.DIFFERENT_CLASS
    return W.filter_labelled_arcs(lg, kind, node_class=cls), LM.filter(g, kind, node_class=cls), op


@pytest.mark.parametrize("case", range(CASES))
def test_random_chain_against_the_model(W, tools, case):
    rng = np.random.default_rng(770000 + case)
    kind = int(rng.choice([GAMMA, FIXED]))
    width = int(rng.integers(0, 32)) if kind == FIXED else 0
    lab_max = min((1 << width) - 1, (1 << 31) - 1) if kind == FIXED else int(rng.choice([0, 1, 100, (1 << 31) - 1]))
    n = int(rng.integers(1, 601))
    dens = float(rng.choice([0.0, 0.02, 0.2, 0.6]))
    g = LM.random_graph(rng, n, dens, heavy=case % 3 == 0, lab_max=lab_max)
    other = LM.random_graph(rng, int(rng.integers(1, 601)), float(rng.choice([0.0, 0.02, 0.2])), lab_max=lab_max)
    trail = ["n=%d dens=%g kind=%d width=%d" % (n, dens, kind, width)]
    lg = W.LabelledGraph.from_csr(g[0], g[1], g[2], kind, width)
    other_lg = W.LabelledGraph.from_csr(other[0], other[1], other[2], kind, width)
    try:
        for _ in range(3):
            nxt, g, what = _step(W, rng, lg, g, other_lg, other)
            lg.close()
            lg = nxt
            trail.append(what)
            off, adj, lab = lg.csr()
            assert (lg.kind, lg.width, lg.num_nodes(), lg.num_arcs()) == (kind, width, LM.nodes(g), len(g[1])), trail
            assert np.array_equal(off, g[0]) and np.array_equal(adj, g[1]) and np.array_equal(lab, g[2]), trail
        stream, offsets = lg.store_labels()
        sl = tools.store_labels(kind, width, g[2], g[0])
        assert stream.tobytes() == sl.stream.tobytes() and np.array_equal(offsets, sl.offsets), trail
    finally:
        lg.close(); other_lg.close()
