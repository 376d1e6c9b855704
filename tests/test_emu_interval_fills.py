"""CPU: tests/test_gpu_interval_fills.py on the emulated library (tests/emu), in both lane orders, one of the two node-by-node places each.
The wave-wide interval fill orders its LDS traffic with wave_sync() alone: the interval entries are read behind the barrier that ends the residual phase, and the lists
that copy from a filled root read it behind the barrier that ends the fill.  A list that is read before it is complete shows in one of the two orders.  The forward order
runs the 32-bit cases, the reversed one the smallest pool, the 64-bit-id path and the checksum contract.  The GPU run has all of it."""
import os

import pytest

from test_emu import ROOT, _gpu_file_on_the_emulator, emu_lib  # noqa: F401  (the fixture builds the emulated library)

ON_THE_EMULATOR = {"fwd": "pool1024 or min2 or no_d2 or waves18", "rev": "pool640 or wide or moved_interval"}


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_interval_fills_on_the_emulator(emu_lib, order):
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_interval_fills.py"), "-k", ON_THE_EMULATOR[order]], BVG_FILLS_PLACES="1")
