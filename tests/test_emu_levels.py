"""CPU: tests/test_gpu_levels.py on the emulated library (tests/emu) -- every case in the forward lane order, three of the seven in the reversed one (NOT dense,
dense_pool1024, dense_no_d2 and the 85-VGPR sparse case: a time trade, 85 s + 33 s on one machine), one of the three node-by-node places each.
The passes of a sub-row order their LDS traffic with wave_sync() alone, so a list that is read before it is complete shows in one of the two orders; the reversed
order runs the cases with the most sub-rows, the long records and the short records on the 128-VGPR instantiation.  The GPU run has all of it."""
import os

import pytest

from test_emu import ROOT, _gpu_file_on_the_emulator, emu_lib  # noqa: F401  (the fixture builds the emulated library)

ON_THE_EMULATOR = {"fwd": "levels", "rev": "dense_pool512 or long or sparse_16_waves"}


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_levels_and_liveness_on_the_emulator(emu_lib, order):
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_levels.py"), "-k", ON_THE_EMULATOR[order]], BVG_LEVELS_PLACES="1")
