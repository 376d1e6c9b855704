"""CPU: tests/test_gpu_recorded_positions.py on the emulated library (tests/emu), in both lane orders, one of the two node-by-node places each.
The pass that places a sub-row's extras from their recorded positions orders its LDS traffic with wave_sync() alone: it reads the parked residuals behind the barrier that
ends the residual phase, and the levels read what it stored behind the barrier that ends it.  A value read before it is written shows in one of the two orders.  The forward
order runs the default geometry, the handles that share an index and a loaded index; the reversed
one entries recorded with full super-rows read with super-rows cut short, and the change of geometry and of instantiation (the entries of the lists without reference) between recording and reading.  The GPU run has all of it."""
import os

import pytest

from test_emu import ROOT, _gpu_file_on_the_emulator, emu_lib  # noqa: F401  (the fixture builds the emulated library)

ON_THE_EMULATOR = {"fwd": "pool1024 or share or loaded", "rev": "large_scratch or geometry"}


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_recorded_positions_on_the_emulator(emu_lib, order):
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_recorded_positions.py"), "-k", ON_THE_EMULATOR[order]], BVG_POS_PLACES="1")
