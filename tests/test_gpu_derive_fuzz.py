"""Randomised parity of the derived offsets index (csrc/bvg_derive.hip, csrc/bvg_derive_seq.hip) with the encoder's offsets and the oracle's
derivation: graph shape x tiling (tens of chunks) x window x max_ref_count x min_interval_length x zeta_k x codings x leading / trailing
empty nodes x warm-up x round kernel, every case on both walks (tests/derive_cases.py: offsets, the walk used, rounds <= chunks + 1, one
scan).

BVG_DERIVE_FUZZ=<n> runs n cases (default below: 92 ms per case measured on one MI355X over 3 000 cases, so 40 cases are 3.7 s; 0.5 - 1 s
per case on the host emulator), BVG_DERIVE_FUZZ_SEED=<s> picks the seed,
BVG_DERIVE_FUZZ_FROM=<c> starts at case c: every case has a generator of its own, seeded with (seed, case), so a case replays alone.

Left out: NOTHING.  The generator draws only streams the walks can read, so every case ends in a comparison of offsets (the test counts
them):
  * Golomb residuals (modulus in zeta_k) only over local_adjacency(reach = 9): every coded value is at most 19, so its unary quotient is
    below 40 for every modulus, which is what the device's decoder takes (derive_cases.golomb_bound_ok, asserted on the drawn adjacency);
  * node ids stay below 2^31: gamma, delta, zeta_k and nibble codes of such values have at most 63 bits.
Unary codes may have any length (the reference, block-count and block codings are drawn from all the header allows): both walks read them.
tests/test_derive_oracle.py draws 2 000 cases of this generator on the CPU and checks that the oracle derives the encoder's offsets for
every one of them."""
import os

import numpy as np
import pytest

from derive_cases import ROUTES, check_derivation, golomb_bound_ok, local_adjacency, set_route, with_empty_nodes
from test_gpu_fuzz import _adjacency

DEFAULT_CASES = 40


def draw(rng, tools, W):
    """One case: (what, Stored, route, expected walk)."""
    n = int(rng.choice([1, 2, 63, 64, 65, 130, 900, 3000]))
    window = int(rng.choice([0, 1, 2, 3, 4, 7, 8, 31, 63, 64, 65, 100, 126, 127, 128, 200]))
    kw = dict(window_size=window, max_ref_count=int(rng.choice([0, 1, 3, 50, -1])) if window else 0,
              min_interval_length=int(rng.choice([0, 1, 2, 4, 7])), zeta_k=int(rng.integers(1, 8)))
    golomb = False
    if rng.random() < 0.5:
        kw.update(outdegree_coding=int(rng.choice([1, 2])), block_coding=int(rng.choice([1, 2, 5])), block_count_coding=int(rng.choice([1, 2, 5])),
                  reference_coding=int(rng.choice([1, 2, 5])), residual_coding=int(rng.choice([1, 2, 3, 6, 7])))
        golomb = kw["residual_coding"] == 3
        if golomb: kw["zeta_k"] = int(rng.choice([1, 2, 3, 8, 100]))
    shape = "local" if golomb else str(rng.choice(["eu_like", "web_like", "fuzz", "local"]))
    gseed = int(rng.integers(0, 1 << 30))
    if shape == "eu_like":
        off, adj = tools.synth_adjacency(min(n, 900), seed=gseed, synth=tools.eu_like(mean_deg=float(rng.choice([10, 40]))), chunk_nodes=1 << 16)
    elif shape == "web_like":
        off, adj = tools.synth_adjacency(n, seed=gseed, synth=tools.web_like(window=int(rng.choice([7, 100]))), chunk_nodes=1 << 16)
    elif shape == "fuzz":
        off, adj = _adjacency(rng, n)
    else:
        off, adj = local_adjacency(rng, n, reach=9)
    if golomb:
        assert golomb_bound_ok(off, adj, kw["zeta_k"])
    lead, trail = int(rng.choice([0, 0, 1, 7, 64, 1000])), int(rng.choice([0, 0, 1, 9, 500]))
    off, adj = with_empty_nodes(off, adj, lead, trail)
    chunk = int(rng.choice([0, 0, 64, 1000]))
    st = tools.store((off, adj), W.default_params(**kw), chunk_nodes=chunk)
    copies = int(rng.choice([1, 1, 3, 20])) if st.params.nodes >= 900 else 1
    if copies > 1 and int(st.offsets[-1]) > 0:
        st = tools.tile_host(st, copies)
    route = str(rng.choice(sorted(ROUTES)))
    what = dict(n=n, shape=shape, graph_seed=gseed, lead=lead, trail=trail, chunk=chunk, copies=copies, route=route, **kw)
    return what, st, route, ("parallel" if window <= 127 else "fallback")


@pytest.mark.gpu
def test_random_streams_through_both_walks(W, tools, oracle, capfd, monkeypatch):
    cases = int(os.environ.get("BVG_DERIVE_FUZZ", DEFAULT_CASES))
    seed = int(os.environ.get("BVG_DERIVE_FUZZ_SEED", "23"))
    first = int(os.environ.get("BVG_DERIVE_FUZZ_FROM", "0"))
    compared = 0
    for case in range(first, cases):
        rng = np.random.default_rng([seed, case])
        what, st, route, expect = draw(rng, tools, W)
        what.update(seed=seed, case=case)
        set_route(monkeypatch, route)
        try:
            check_derivation(W, oracle, capfd, monkeypatch, st.params, st.graph, st.offsets, expect, what=what)
            compared += 1
        except BaseException:
            with capfd.disabled():
                print("derive fuzz case that failed:", what, flush=True)
            raise
        if case % 100 == 99:
            with capfd.disabled():
                print("derive fuzz: %d of %d cases" % (case + 1, cases), flush=True)
    assert compared == cases - first, "every case must end in a comparison"
