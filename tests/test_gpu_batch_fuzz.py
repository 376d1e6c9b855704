"""Randomised parity of random access (bvg_successors_batch) with the adjacency the test wrote down: node count x shape x BV parameters
(windows and reference counts of tests/batch_cases.py, interval length, zeta k, non-default codings) x forced tier (as is / giant kernel on
every block / generic kernel / 64-bit kernels) x index built or not x handle kind (node base, bvg_copy, bvg_tile, no_index) x request
pattern x request count; for one case in four the requests are biased to the nodes of largest own_reach.  Every case compares
outdegrees and successors with batch_cases.expected(), element for element, twice on the same handle.

BVG_BATCH_FUZZ=<n> runs n cases (default below), BVG_BATCH_FUZZ_SEED=<s> picks the seed, BVG_BATCH_FUZZ_FROM=<c> starts at case c: every
case has a generator of its own, seeded with (seed, case), so a case replays alone (BVG_BATCH_FUZZ_FROM=c BVG_BATCH_FUZZ=c+1): every draw
of the cases before it is skipped with them and nothing of them is run.  A failing case prints its tuple.

DEFAULT_CASES IS NOT YET SIZED BY A GPU MEASUREMENT: 24 is a guess from the cost of the same draws in tests/test_gpu_fuzz.py, the GPU
time of this file is not known, and no run of a few thousand fresh-seed cases has been made on a GPU; the first engineer with a GPU run
of this file writes its seconds here and the count and outcome of the fresh-seed run into the README.
On the host emulator (tests/emu) a case costs 1 - 20 s, and a minute and more where a draw has 6 000 nodes, long chains and thousands of
requests (every deep request is a range decode of its own): tests/test_emu.py runs ten cases per lane order of a seed it names."""
import os

import numpy as np
import pytest

import batch_cases as BC

pytestmark = pytest.mark.gpu

DEFAULT_CASES = 24
DEFAULT_SEED = 53
TIERS = ("as_is", "as_is", "giant", "force_slow", "force_wide")


def draw(rng):
    """One case: (what, everything needed to run it).  All draws are made here."""
    n = int(rng.choice([1, 70, 900, 6000]))
    shape = str(rng.choice(BC.SHAPES))
    kw = dict(window_size=int(rng.choice(BC.WINDOWS)), max_ref_count=int(rng.choice(BC.MAX_REF_COUNTS)),
              min_interval_length=int(rng.choice([0, 2, 4])), zeta_k=int(rng.choice([1, 3, 5])))
    if rng.random() < 0.3:
        kw.update({k: int(rng.choice(v)) for k, v in BC.CODINGS.items()})
    tier = str(rng.choice(TIERS))
    indexed = bool(rng.random() < 0.5)
    kind = str(rng.choice([k for k in BC.HANDLE_KINDS if k != "indexed"]))
    pattern = str(rng.choice(BC.PATTERNS))
    count = int(rng.choice([1, 40, 1000, 5000]))
    biased = bool(rng.random() < 0.25)
    graph_seed, request_seed = int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 31))
    what = dict(n=n, shape=shape, params=kw, tier=tier, indexed=indexed, handle=kind, pattern=pattern, count=count, biased=biased,
                graph_seed=graph_seed, request_seed=request_seed)
    return what


def run(W, tools, monkeypatch, what):
    monkeypatch.delenv("BVG_GIANT", raising=False)
    if what["tier"] == "giant":
        monkeypatch.setenv("BVG_GIANT", "2")
    n = what["n"]
    rng = np.random.default_rng(what["graph_seed"])
    st = BC.store_lists(tools, BC.shape_lists(what["shape"], n, rng, tools), W.default_params(**what["params"]))
    default_codings = "residual_coding" not in what["params"]
    reach = BC.reaches(st) if default_codings else np.zeros(n, dtype=np.int64)      # (own_reach reads default codings only: no bias elsewhere)
    order = np.argsort(-reach, kind="stable")
    deep = order[:max(1, n // 20)][reach[order[:max(1, n // 20)]] > 0]
    deg = np.array([len(l) for l in st.lists])
    rng = np.random.default_rng(what["request_seed"])
    nodes = BC.requests(what["pattern"], n, deg, deep, rng, count=what["count"])
    if what["biased"] and len(deep):
        nodes = np.concatenate([nodes, rng.choice(deep, what["count"])])[rng.permutation(len(nodes) + what["count"])]
    tuning = {"force_slow": True} if what["tier"] == "force_slow" else {"force_wide": True} if what["tier"] == "force_wide" else None
    keep, g, lists, base = BC.open_kind(W, st, what["handle"], tuning)
    try:
        if what["indexed"]:
            keep[0].scan(); keep[0].build_index()
        if what["handle"] == "tile":
            nodes = nodes + n * rng.integers(0, 3, len(nodes))
        for again in (0, 1):
            BC.check_batch(g, lists, nodes if not again else nodes[::-1], dict(what, again=again), base=base)
    finally:
        for x in keep[::-1]:
            x.close()


def test_random_batches(W, tools, monkeypatch):
    cases = int(os.environ.get("BVG_BATCH_FUZZ", DEFAULT_CASES))
    seed = int(os.environ.get("BVG_BATCH_FUZZ_SEED", DEFAULT_SEED))
    first = int(os.environ.get("BVG_BATCH_FUZZ_FROM", "0"))
    compared = 0
    for c in range(first, cases):
        what = draw(np.random.default_rng([seed, c]))
        what.update(seed=seed, case=c)
        try:
            run(W, tools, monkeypatch, what)
            compared += 1
        except BaseException:
            print("batch fuzz case that failed:", what, flush=True)
            raise
        if c % 100 == 99: print("batch fuzz: %d of %d cases" % (c + 1, cases), flush=True)          # (long runs: `pytest -s` shows progress)
    assert compared == cases - first, "every case must end in a comparison"
