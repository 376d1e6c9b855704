"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step returned -- the arc count and the 64-bit checksum of the line it
prints -- and the same workload gives the same outputs whatever the number of steps, and whether the run is plain or --full (the workload
is seeded: two builds can be compared output for output; the --full run gates its handle against the CPU oracle, the plain one must agree)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(steps, out, *extra):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--shape", "cnr", "--target-gib", "1", "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline",
                        "--no-index-leg", "--no-real-leg", "--no-wide-leg", "--dump-outputs", str(out)] + list(extra), capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_step_result(tmp_path):
    got = []
    for steps, extra in ((1, ["--full"]), (3, [])):
        out = tmp_path / ("steps%d" % steps)
        line = _run(steps, out, *extra)
        arcs, bits = np.load(str(out / "arcs.npy")), np.load(str(out / "chk_bits.npy"))
        assert line["steps"] == steps
        assert int(arcs[0]) == line["arcs"] and "%016x" % sum(int(v) << i for i, v in enumerate(bits)) == line["checksum"]
        got.append((arcs, bits))
    assert all(np.array_equal(x, y) for x, y in zip(*got))
