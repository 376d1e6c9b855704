"""Randomised parity of the device compressor (bvg_store, csrc/bvg_encode.hip) with the CPU tooling over its whole parameter space:
graph shape x n x window (0..127) x max_ref_count x min_interval_length x zeta_k x codings x chunking.  Every case: offsets and bytes
equal the tooling's; the CPU oracle decodes the DEVICE's bytes back to the adjacency; one case in four the HIP decoder does too
(store -> decode on the device).

BVG_STORE_FUZZ=<n> runs n cases (default below), BVG_STORE_FUZZ_SEED=<s> picks the seed, BVG_STORE_FUZZ_FROM=<c> starts at case c: every
case has a generator of its own, seeded with (seed, case), so a case replays alone (BVG_STORE_FUZZ_FROM=c BVG_STORE_FUZZ=c+1).

The default count is set by time: a plain run is to cost what tests/test_gpu_fuzz.py's plain run (16 cases) costs, so that it stays a test
that runs every time.  Measured on one MI355X: test_gpu_fuzz.py at its default 3.2 s (3.27 s and 3.23 s, at the commit before this file);
this file 16 ms per case (200 cases on a fresh seed: 3.22 s; 24 cases: 0.6 - 0.8 s, of which 0.3 s is the first call).  On the host emulator
(tests/emu) a case costs 0.33 s (60 cases: 19.6 s), which is why tests/test_emu.py runs ten per lane order and not the default.
Chosen: 200 cases.
"""
import os

import numpy as np
import pytest

from test_gpu_fuzz import _adjacency
from test_gpu_store import _csr, _far_graph

pytestmark = pytest.mark.gpu

DEFAULT_CASES = 200


def _draw(rng, tools):
    n = int(rng.choice([1, 2, 63, 64, 65, 130, 900, 6000]))
    kw = dict(window_size=int(rng.choice([0, 1, 2, 7, 31, 63, 64, 65, 100, 127])), max_ref_count=int(rng.choice([0, 1, 2, 3, 50, -1])),
              min_interval_length=int(rng.choice([0, 1, 2, 3, 4, 9])), zeta_k=int(rng.choice([1, 2, 3, 5, 7])))
    if rng.random() < 0.5:
        kw.update(outdegree_coding=int(rng.choice([1, 2])), block_coding=int(rng.choice([1, 2, 5])), residual_coding=int(rng.choice([1, 2, 3, 6, 7])),
                  reference_coding=int(rng.choice([1, 2, 5])), block_count_coding=int(rng.choice([1, 2, 5])))
        if kw["residual_coding"] == 3: kw["zeta_k"] = int(rng.choice([1, 2, 3, 8]))                  # (Golomb's modulus travels in zeta_k)
    chunk = int(rng.choice([0, 1, 2, 5, 63, 64, 65, 100, 1000, 5000]))
    shape = str(rng.choice(["eu_like", "web_like", "fuzz", "far"]))
    gseed = int(rng.integers(0, 1 << 30))
    if shape == "eu_like":
        adj = tools.synth_adjacency(n, seed=gseed, synth=tools.eu_like(mean_deg=float(rng.choice([10, 40]))), chunk_nodes=1 << 16)
    elif shape == "web_like":
        adj = tools.synth_adjacency(n, seed=gseed, synth=tools.web_like(window=int(rng.choice([7, 100]))), chunk_nodes=1 << 16)
    elif shape == "fuzz":
        adj = _adjacency(rng, n)
    else:
        adj = _csr(_far_graph(n, gseed, dists=tuple(int(v) for v in rng.integers(1, 128, 7)), members=int(rng.integers(2, 5)), empty_every=int(rng.choice([2, 5, 1000])))[0])
    return n, kw, chunk, shape, gseed, adj


def test_random_graphs_and_parameters_through_the_device_compressor(W, tools, oracle):
    cases = int(os.environ.get("BVG_STORE_FUZZ", DEFAULT_CASES))
    seed = int(os.environ.get("BVG_STORE_FUZZ_SEED", "11"))
    for case in range(int(os.environ.get("BVG_STORE_FUZZ_FROM", "0")), cases):
        rng = np.random.default_rng([seed, case])
        n, kw, chunk, shape, gseed, (off, adj) = _draw(rng, tools)
        what = dict(seed=seed, case=case, n=n, shape=shape, graph_seed=gseed, chunk=chunk, **kw)
        p = W.default_params(**kw).clone(nodes=n, arcs=len(adj))
        try:
            want = tools.store((off, adj), p, chunk_nodes=chunk)
            graph, offsets = W.store((off, adj), p, chunk_nodes=chunk)
            assert np.array_equal(offsets, want.offsets), "offsets differ from node %d on" % int(np.argmax(offsets != want.offsets))
            assert graph.tobytes() == want.graph.tobytes(), "bytes differ"
            deg, dec = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), offsets).decode_range(0, n)
            assert np.array_equal(deg, np.diff(off.astype(np.int64))) and np.array_equal(dec, adj), "the oracle does not decode the device's bytes to the adjacency"
            if case % 4 == 0:                                                  # store -> decode, both on the device
                g = W.BVGraph.from_memory(p, graph, offsets)
                try:
                    deg, dec = g.decode_range(0, n)
                finally:
                    g.close()
                assert np.array_equal(deg, np.diff(off.astype(np.int64))) and np.array_equal(dec, adj), "the HIP decoder does not decode the device's bytes to the adjacency"
        except BaseException:
            print("store fuzz case that failed:", what, flush=True)
            raise
        if case % 100 == 99: print("store fuzz: %d of %d cases" % (case + 1, cases), flush=True)    # (long runs: `pytest -s` shows progress)
