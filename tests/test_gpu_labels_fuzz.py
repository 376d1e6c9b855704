"""Randomised parity of the arc-label decoder (csrc/bvg_labels.hip) with the plain model (tests/labels_model.py): class x width x node count x
value pattern x list lengths x leading bits x range x one defect or none, drawn from tests/label_cases.py and checked by its one rule
(the device returns 0 exactly when the model decodes, and then the arrays are equal; otherwise the documented error, nothing handed out).

BVG_LABELS_FUZZ=<n> runs n cases (default below), BVG_LABELS_FUZZ_SEED=<s> picks the seed, BVG_LABELS_FUZZ_FROM=<c> starts at case c: every
case has a generator of its own, seeded with (seed, case), so a case replays alone (BVG_LABELS_FUZZ_FROM=c BVG_LABELS_FUZZ=c+1).

Left out: NOTHING.  Every case ends in a comparison (the test counts them).  List streams that decode to more than 2^22 elements would be
sized instead of compared (label_cases' module docstring); tests/test_labels_model.py draws the first 400 cases of the default seed on
the CPU and asserts that none is of that kind, and that the draws hit every outcome.

A case costs 13 ms on the host emulator (tests/emu; 400 cases: 5.3 s), most of it the model's."""
import os

import numpy as np
import pytest

import label_cases as LC

pytestmark = pytest.mark.gpu

DEFAULT_CASES = 20
DEFAULT_SEED = 41
KINDS = (LC.GAMMA, LC.FIXED, LC.LIST, LC.LONG_LIST)


def draw(rng):
    """One case: (what, Case, ranges)."""
    kind = int(rng.choice(KINDS))
    width = int(rng.choice(list(LC.widths(kind))))
    n = int(rng.choice([1, 2, 63, 255, 256, 257, 513, 1025]))
    pattern = str(rng.choice(LC.PATTERNS))
    lens_mode = str(rng.choice(["zero", "one", "mixed", "mixed"]))
    lead = int(rng.integers(0, 24))
    case = LC.make("fuzz", kind, width, LC.degrees(n, rng, big=int(rng.choice([0, 40, 300])), top=int(rng.choice([2, 4, 9]))), pattern, rng, lens_mode=lens_mode, lead=lead)
    defect = str(rng.choice(["none"] * 6 + ["flip"] * 6 + LC.defect_names(case)))
    if defect != "none":
        case = LC.apply_defect(case, defect, rng)
    a, b = sorted(int(v) for v in rng.integers(0, n + 1, size=2))
    ranges = [(0, n), (a, b)]
    what = dict(kind=LC.KIND_NAMES[kind], width=width, n=n, pattern=pattern, lens=lens_mode, lead=lead, defect=case.name, ranges=ranges)
    return what, case, ranges


def test_random_label_streams(W):
    cases = int(os.environ.get("BVG_LABELS_FUZZ", DEFAULT_CASES))
    seed = int(os.environ.get("BVG_LABELS_FUZZ_SEED", DEFAULT_SEED))
    first = int(os.environ.get("BVG_LABELS_FUZZ_FROM", "0"))
    compared = 0
    for c in range(first, cases):
        what, case, ranges = draw(np.random.default_rng([seed, c]))
        what.update(seed=seed, case=c)
        try:
            seen = LC.check_parity(W, case, ranges=ranges, what=what)
            assert isinstance(seen, str) or len(seen) == 2
            compared += 1
        except BaseException:
            print("labels fuzz case that failed:", what, flush=True)
            raise
        if c % 100 == 99: print("labels fuzz: %d of %d cases" % (c + 1, cases), flush=True)          # (long runs: `pytest -s` shows progress)
    assert compared == cases - first, "every case must end in a comparison"
