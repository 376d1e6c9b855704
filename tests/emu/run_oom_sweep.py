"""TEST INFRASTRUCTURE (emulated library): EVERY device allocation of a sequence of calls fails once, one run per allocation.  Whichever it is,
the call either gives the oracle's answer all the same (a fallback took over: an index-less scan, a smaller workspace) or raises MemoryError
(BVG_E_NOMEM); repeated once it succeeds with the oracle's answer; and once the handles are closed no device block is left allocated
(emu_live_allocs: csrc/bvg_host.h, DevArray / DevWorkspace own every block).  Prints the allocations of a clean run per step.
    python tests/emu/run_oom_sweep.py [first_k [last_k]]"""
import atexit
import ctypes
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BVG_HIP_LIB"] = os.path.join(HERE, os.environ.get("BVG_EMU_LIB", "libbvgraph_emu.so"))     # (an absolute path wins)
os.environ["BVG_TEST_KNOBS"] = "1"
os.environ.pop("BVG_DEBUG", None)

import numpy as np  # noqa: E402
import tooling as T  # noqa: E402
import webgraph_big_amd as W  # noqa: E402
from oracle import bvg_oracle as O  # noqa: E402
import label_cases as LC  # noqa: E402
import labels_model as LM  # noqa: E402

# k's at which a call raises something other than MemoryError, as the commit before the owners did: {k: (step, exception class, reason)}
OTHER_STATUS = {}
# One call neither raises nor answers like the clean run, as before: bvg_build_index reports (entries, bytes) of the index, and an index whose build
# ran out of memory is documented as absent, not as an error (SkipIndex::kResources: the scans run without it) -- it returns 0 entries.  The call
# repeated builds the index (bvg_build_index retries a failed range at once) and must then report what the clean run reports.
ABSORBED = {"build_index": lambda got: got[0] == 0}

emu = ctypes.CDLL(os.environ["BVG_HIP_LIB"])
emu.emu_fail_malloc_at.argtypes = [ctypes.c_long]
emu.emu_malloc_count.restype = ctypes.c_long
emu.emu_live_allocs.restype = ctypes.c_long

N = 2100                                # the smallest graph (in hundreds) whose two tiles are scanned with the index built inside the scan: 117 allocations, as with 3 000 nodes
st = T.synth_store(N, seed=4, synth=T.web_like(), threads=2)
og = O.Graph.from_memory(O.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
odeg, osucc = og.decode_range(0, N)
ocum = np.concatenate([[0], np.cumsum(odeg, dtype=np.int64)])
BATCH = [3, N // 4, N // 2, N - 1]
ADJ = [[int(v) for v in osucc[ocum[i]:ocum[i + 1]] if v < 200] for i in range(200)]      # the 200-node adjacency W.store compresses
LABELS = LC.make("sweep", LC.FIXED, 7, [int(d) for d in odeg], "random", np.random.default_rng(11))
TMP = tempfile.mkdtemp(prefix="bvg_oom_sweep_")
atexit.register(shutil.rmtree, TMP, ignore_errors=True)


def flat(x):
    """a step's result as something == compares"""
    if isinstance(x, dict):
        return (x["arcs"], x["chk"], x["nodes"])
    if isinstance(x, (tuple, list)):
        return tuple(flat(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.tobytes())
    return x


class Run:
    """the handles of one run; every step takes the run and returns what is compared"""
    g = c = t = lab = None

    def close(self):
        for h in (self.lab, self.t, self.c, self.g):
            if h is not None:
                h.close()


def s_open(r): r.g = W.BVGraph.from_memory(st.params, st.graph, st.offsets, device=0)
def s_copy(r): r.c = r.g.copy(); r.c.set_tuning(block_bits=16384)
def s_tile(r): r.t = r.g.tile(2)
def s_labels(r): r.lab = W.BitStreamArcLabelledImmutableGraph.from_memory(r.g, LABELS.kind, LABELS.width, LABELS.stream, LABELS.offsets)
def s_index_file(r): r.g.load_index(r.g.save_index(os.path.join(TMP, "g.bvgidx")))


STEPS = [
    ("open", s_open),
    ("scan 1", lambda r: r.g.scan()),
    ("scan 2", lambda r: r.g.scan()),
    ("decode_range", lambda r: r.g.decode_range(10, 500)),
    ("successors_batch", lambda r: r.g.successors_batch(BATCH)),
    ("outdegrees", lambda r: r.g.outdegrees()),
    ("split_by_arcs", lambda r: r.g.split_by_arcs(3)),
    ("shard_bounds", lambda r: r.g.shard_bounds(4)),
    ("copy + set_tuning", s_copy),
    ("scan of the copy", lambda r: r.c.scan()),
    ("build_index", lambda r: r.g.build_index()),
    ("save_index + load_index", s_index_file),
    ("tile", s_tile),
    ("scan of the tile", lambda r: r.t.scan()),
    ("store", lambda r: W.store(ADJ, params=st.params)),
    ("labels open", s_labels),
    ("labels decode_range", lambda r: r.lab.decode_range(10, 500)),
]


def oracle_results():
    """what the oracle (the tooling's compressor, the label model) says of the steps it can answer; the others are taken from the clean run"""
    o = og.scan()
    cpu = T.store(ADJ, params=st.params)
    lab = LM.decode(LABELS.kind, LABELS.width, LABELS.stream, LABELS.offsets, 10, 500, LABELS.deg[10:500])
    rng = (odeg[10:500], osucc[ocum[10]:ocum[500]])
    return {
        "scan 1": o, "scan 2": o, "scan of the copy": o, "decode_range": rng, "outdegrees": odeg,
        "successors_batch": (odeg[BATCH], np.concatenate([osucc[ocum[x]:ocum[x + 1]] for x in BATCH])),
        "store": (cpu.graph, cpu.offsets),
        "labels decode_range": rng + (np.asarray(lab.labels, dtype=np.int32),),
    }


def run(k, expect):
    """one run with the k-th allocation failing (0: none): (results, allocations per step, problems)"""
    live0 = emu.emu_live_allocs()
    r = Run(); out = {}; counts = []; problems = []
    emu.emu_fail_malloc_at(k)
    try:
        for name, step in STEPS:
            c0 = emu.emu_malloc_count()
            try:
                got = step(r)
            except BaseException as e:  # noqa: B902  (whatever the call raises is judged below)
                want = OTHER_STATUS[k][1] if k in OTHER_STATUS and OTHER_STATUS[k][0] == name else MemoryError
                if k == 0 or type(e) is not want:
                    problems.append("%s raised %r" % (name, e))
                got = step(r)                                                  # the failure was transient: the same call again (a fresh open if it was the open)
            if k and name in ABSORBED and expect is not None and flat(got) != expect[name] and ABSORBED[name](got):
                got = step(r)
            counts.append(emu.emu_malloc_count() - c0)
            out[name] = flat(got)
            if expect is not None and name in expect and out[name] != expect[name]:
                problems.append("%s differs from the oracle" % name)
    except BaseException as e:  # noqa: B902
        problems.append("%s raised %r when repeated" % (name, e))
    finally:
        emu.emu_fail_malloc_at(0)
        r.close()
    leaked = emu.emu_live_allocs() - live0
    if leaked:
        problems.append("%d device blocks left allocated after the closes" % leaked)
    return out, counts, problems


def main():
    oracle = {k: flat(v) for k, v in oracle_results().items()}
    clean, counts, problems = run(0, oracle)
    assert not problems, problems
    total = sum(counts)
    print("allocations of a clean run: %d" % total)
    for (name, _), c in zip(STEPS, counts):
        print("  %-26s %d" % (name, c))
    assert clean["scan of the tile"][0] == 2 * clean["scan 1"][0]
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    last = int(sys.argv[2]) if len(sys.argv) > 2 else total
    bad = []
    for k in range(first, last + 1):
        _, _, problems = run(k, clean)
        if problems:
            bad.append(k)
            print("k = %d: %s" % (k, "; ".join(problems)), flush=True)
    print("oom sweep: allocations %d..%d, %d failed%s" % (first, last, len(bad), (": k = " + ", ".join(map(str, bad))) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
