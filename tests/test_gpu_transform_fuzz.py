"""GPU: random graphs from the shapes the compressor's fuzz draws, through random sequences of the transforms, every step chained on the
device (the result of one call is the source of the next) and held against the model (tests/transform_model.py).

BVG_TRANSFORM_FUZZ=<n> runs n cases (default below), BVG_TRANSFORM_FUZZ_SEED=<s> picks the seed; every case has a generator of its own,
seeded with (seed, case), and the failing case, step and operation are in the assertion message."""
import os

import numpy as np
import pytest

import transform_model as M
from test_gpu_fuzz import _adjacency

pytestmark = pytest.mark.gpu

DEFAULT_CASES = 40
OPS = ["map", "filter", "transpose", "symmetrize", "simplify", "union", "lex", "gray", "random", "dangling"]


def _draw_graph(rng, tools):
    n = int(rng.choice([1, 2, 63, 64, 65, 130, 900]))
    shape = str(rng.choice(["eu_like", "web_like", "fuzz"]))
    gseed = int(rng.integers(0, 1 << 30))
    if shape == "eu_like":
        off, adj = tools.synth_adjacency(n, seed=gseed, synth=tools.eu_like(mean_deg=float(rng.choice([10, 40]))), chunk_nodes=1 << 16)
    elif shape == "web_like":
        off, adj = tools.synth_adjacency(n, seed=gseed, synth=tools.web_like(window=int(rng.choice([7, 100]))), chunk_nodes=1 << 16)
    else:
        off, adj = _adjacency(rng, n)
    return (np.asarray(off).astype(np.int64), np.asarray(adj, dtype=np.int64)), dict(n=n, shape=shape, graph_seed=gseed)


def _step(W, rng, op, g, model, other, other_model):
    """One operation on the device graph g and on the model: (new device graph, new model)."""
    n = len(model[0]) - 1
    if op == "map":
        f = rng.integers(-1, max(1, [n, n // 2, n + 9][int(rng.integers(3))]), size=n)
        return W.map_graph(g, f), M.map_graph(*model, f)
    if op == "filter":
        kind = str(rng.choice(["NO_LOOPS", "SAME_CLASS", "DIFFERENT_CLASS"]))
        cls = None if kind == "NO_LOOPS" else rng.integers(0, 3, size=n)
        return W.filter_arcs(g, kind, cls), M.filter_arcs(*model, kind, cls)
    if op == "transpose":
        return W.transpose_graph(g), M.transpose(*model)
    if op == "symmetrize":
        return W.symmetrize_graph(g), M.symmetrize(*model)
    if op == "simplify":
        return W.simplify_graph(g), M.symmetrize(*model, drop_loops=True)
    if op == "union":
        drop = bool(rng.integers(2))
        return W.union(g, other, drop_loops=drop), M.union(model, other_model, drop_loops=drop)
    if op == "dangling":
        return W.remove_dangling(g), M.map_graph(*model, M.remove_dangling_map(model[0]))
    if op == "random":
        seed = int(rng.integers(0, 1 << 62))
        perm = W.random_permutation(g, seed)
        assert np.array_equal(perm, M.random_permutation(n, seed))
    else:
        perm = (W.gray_code_permutation if op == "gray" else W.lexicographical_permutation)(g)
        assert np.array_equal(perm, M.permutation_of_csr(*model, op == "gray"))
    return W.map_graph(g, perm), M.map_graph(*model, perm)


def test_random_sequences_of_transforms(W, tools):
    cases = int(os.environ.get("BVG_TRANSFORM_FUZZ", DEFAULT_CASES))
    seed = int(os.environ.get("BVG_TRANSFORM_FUZZ_SEED", "29"))
    for case in range(cases):
        rng = np.random.default_rng([seed, case])
        model, what = _draw_graph(rng, tools)
        other_model, _ = _draw_graph(rng, tools)
        what.update(seed=seed, case=case)
        g = W.ParsedGraph.from_csr(*model)
        other = W.ParsedGraph.from_csr(*other_model)
        try:
            for step in range(4):
                op = str(rng.choice(OPS))
                try:
                    nxt, model = _step(W, rng, op, g, model, other, other_model)
                except AssertionError as e:
                    raise AssertionError("%r step %d %s: %s" % (what, step, op, e))
                g.close()
                g = nxt
                off, adj = g.csr()
                assert M.same((off, adj), model), (what, step, op)
            if case % 4 == 0:                                        # the resident result compresses to what the CPU encoder writes
                graph, offsets = g.store()
                ref = tools.store((model[0].astype(np.uint64), model[1]), W.default_params().clone(nodes=len(model[0]) - 1, arcs=len(model[1])))
                assert np.array_equal(offsets, ref.offsets) and graph.tobytes() == ref.graph.tobytes(), what
        finally:
            g.close(); other.close()
