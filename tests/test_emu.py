"""The product's kernels on the CPU EMULATOR (tests/emu: the .hip sources compiled for the host, every lane of a wavefront a fiber) against the
oracle.  This container has no GPU: the emulator is where the wavefront code is stepped through, asserted on and run under AddressSanitizer
before it goes to the GPU box; results must not depend on the order in which the lanes run between two cross-lane operations
(BVG_EMU_ORDER=rev), or an LDS dependency lacks its wave_sync().  The emulated library is test infrastructure: the product never loads it
(tests/test_abi.py::test_product_never_touches_the_oracle covers tests/ as a whole: nothing under webgraph-big_amd/ or bench.py names it)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "libbvgraph_emu.so"])
    return os.path.join(EMU, "libbvgraph_emu.so")


def run_case(*args, **env):
    e = dict(os.environ); e.update({k: str(v) for k, v in env.items()})
    e.pop("BVG_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(EMU, "run_case.py")] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_sparse_graph_through_the_emulated_kernels(emu_lib, order):
    out = run_case(12000, 3, "web", 3, BVG_EMU_ORDER=order)
    assert "emu case ok" in out and "lean_blocks 0 " in out.splitlines()[0]          # the first scan builds the index on the checking kernels ...
    assert "lean_blocks 0 " not in out.splitlines()[2]                                # ... and the steady state runs the lean kernel


@pytest.mark.parametrize("recs,order,shape,n,seed", [(64, "fwd", "eu", 6000, 5), (64, "rev", "web", 12000, 3), (128, "fwd", "web", 12000, 3), (256, "rev", "eu", 6000, 5), (256, "fwd", "cnr", 40000, 0)])
def test_flat_scan_kernel_on_the_emulator(emu_lib, recs, order, shape, n, seed):
    """experimental/bvg_flat.hip (round 5's flat task kernel: per-record state in an LDS table, run items instead of the position loop) against the oracle: every
    pass structure (64 / 128 / 256 records per super-row), both lane orders, a dense, a sparse and the reference's own graph."""
    out = run_case(n, seed, shape, 2, BVG_FLAT=1, BVG_FLAT_RECS=recs, BVG_EMU_ORDER=order)
    assert "emu case ok" in out and "lean_blocks 0 " not in out.splitlines()[1]


def test_a_failed_allocation_during_the_index_build_is_transient(emu_lib):
    """bvg_api.hip give_up(): an out-of-memory failure of the index build is remembered (no counting pass per scan), announced once, and retried every 8th scan."""
    e = dict(os.environ); e.pop("BVG_HIP_LIB", None); e.pop("BVG_DEBUG", None)
    out = subprocess.run([sys.executable, os.path.join(EMU, "run_oom.py")], env=e, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "oom case ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stderr.count("warning: the residual skip index") == 1 and "out of device memory" in out.stderr, out.stderr[-2000:]


def test_every_allocation_failing_in_turn_leaks_nothing(emu_lib):
    """tests/emu/run_oom_sweep.py: open, two scans, decode_range, successors_batch, outdegrees, split_by_arcs, shard_bounds, a copy with another block size and
    its scan, build_index, save_index / load_index, tile(2) and its scan, W.store, arc labels, the closes -- 117 device allocations -- run once per allocation
    with that allocation failing.  Every call answers as the oracle does or raises MemoryError (BVG_E_NOMEM) and succeeds when repeated, and no device block
    is left allocated once the handles are closed: the host code holds device memory in DevArray / DevWorkspace (csrc/bvg_host.h) alone.  Before that, 31 of
    the 117 runs left up to five blocks behind (a handle whose second array could not be had, the block plan's arrays on every early return)."""
    e = dict(os.environ); e.pop("BVG_HIP_LIB", None); e.pop("BVG_DEBUG", None); e.pop("BVG_EMU_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(EMU, "run_oom_sweep.py")], env=e, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "allocations 1..117, 0 failed" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.skipif(not os.environ.get("BVG_EMU_ASAN"), reason="opt-in (BVG_EMU_ASAN=1): the AddressSanitizer build of the emulated library takes ~4 minutes to compile")
@pytest.mark.parametrize("flat", [0, 1])
def test_kernels_under_address_sanitizer(flat):
    """The LDS and global-memory indexing of the row, scan and flat kernels under ASan + UBSan (the dynamic LDS of a launch is a heap block of exactly the bytes the
    launch asked for): round 5 found one out-of-allocation LDS read in rows_kernel this way (harmless on the hardware, fixed)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "asan"])
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    out = run_case(6000, 5, "eu", 2, BVG_EMU_LIB="libbvgraph_emu_asan.so", LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", BVG_FLAT=flat, BVG_FLAT_RECS=128)
    assert "emu case ok" in out


def test_malformed_stream_suite_on_the_emulator(emu_lib):
    """tests/test_malformed_streams.py -- hand-assembled records the encoder never writes (equal heads between the three streams, cap at d, over-running copy blocks,
    negative residual counts), every tier and emission mode against the oracle -- is a GPU suite; the emulator runs its 56 GPU cases on the CPU, so the refusal and
    fail-over logic of the kernels is exercised by the driver's CPU run too."""
    e = dict(os.environ, BVG_HIP_LIB=emu_lib, BVG_TEST_KNOBS="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_malformed_streams.py"), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                         env=e, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def _gpu_file_on_the_emulator(emu_lib, order, args, **env):
    e = dict(os.environ, BVG_HIP_LIB=emu_lib, BVG_TEST_KNOBS="1", BVG_EMU_ORDER=order, **env)
    out = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider"] + args, env=e, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert out.returncode == 0 and " passed" in out.stdout and "skipped" not in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]


# what of tests/test_gpu_store.py each lane order runs here (the GPU run has all of it)
STORE_ON_THE_EMULATOR = {
    "fwd": "not 100000 and not cnr2000 and not round_trip and not fuzz_6000 and not test_device_store_equals_cpu_tooling",
    "rev": "windows_around or chunks_that or equally_cheap or one_tile or min_interval",
}


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_device_compressor_suite_on_the_emulator(emu_lib, order):
    """tests/test_gpu_store.py -- the device compressor against the CPU tooling, byte for byte, and its bytes through the oracle -- on the CPU.
    Cut from the emulated selection, for time only (all of them run on the GPU): the list of over 100 000 successors (its three cases take
    longer here than the rest together), the cnr-2000 fixture (39 s here), the 20 000-node round trip through the decoder (7 s), the
    6 000-node shapes (20 s) and the original 7 000-node parameter sets (18 x 1.1 s; the same parameters run here on 1 500 nodes).  The
    reversed lane order is for enc_choose_kernel, which orders its LDS traffic with enc_wave_sync() alone (the other three kernels have no
    cross-lane traffic at all): it runs the tests that vary the window, the chunk and the chains, the forward order everything kept.
    Measured on one machine: test_malformed_stream_suite_on_the_emulator 93 s (at the commit before this test); this test 42 s (fwd) +
    23 s (rev), the randomised test below 3 s + 5 s: 73 s together."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_store.py"), "-k", STORE_ON_THE_EMULATOR[order]])


@pytest.mark.parametrize("order,first", [("fwd", 0), ("rev", 10)])
def test_randomised_device_compressor_on_the_emulator(emu_lib, order, first):
    """tests/test_gpu_store_fuzz.py, ten cases per lane order (0.33 s a case here); the two orders run different cases."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_store_fuzz.py")], BVG_STORE_FUZZ=str(first + 10), BVG_STORE_FUZZ_FROM=str(first))


# what of tests/test_gpu_derive.py each lane order runs here (the GPU run has all of it)
DERIVE_ON_THE_EMULATOR = {
    "fwd": "truncated or more_nodes or fewer_nodes or reference_ or contradict or unary or codes_of or legal_but or degenerate or (streams_that and default) "
           "or (parameter_space and (zeta-warm0_list or golomb-warm0_crawl)) or (blind and intervals-as_is-warm0_crawl)",
    "rev": "truncated or reference_ or contradict or (parameter_space and (codings-warm0_list or intervals-default)) or (streams_that and warm0_crawl) "
           "or (chunks_that and warm0_list) or (blind and residuals-as_is-warm0_list)",
}


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_offsets_derivation_suite_on_the_emulator(emu_lib, order):
    """tests/test_gpu_derive.py -- both walks of the offsets derivation against the encoder's offsets and the oracle's derivation -- on the CPU.
    The parallel walk keeps per-lane outdegree rings in LDS at a stride of 64 dwords and derive_crawl_kernel shares its table of code lengths
    behind a __syncthreads(); the sequential walk shares two LDS rings between all lanes: the reversed lane order and the exact-size LDS block
    are for these.  Cut from the emulated selection, for time only (all of it runs on the GPU): the sweep of 72 alignments (36 s per group of
    eight here), the blind states but one case per order (20 - 28 s each), most groups of the parameter space.  The status-parity cases
    (streams that are wrong) run here in full, in both orders, before any GPU sees them.
    Found here, not on the GPU: through thousands of empty records the emulator's lanes drifted more than a ring of outdegrees apart in
    derive_offsets_kernel (bvg_derive_seq.hip now keeps them within 64 nodes with a barrier).
    Measured on one machine, next to the figures of test_device_compressor_suite_on_the_emulator: 70 s (fwd) + 75 s (rev),
    the randomised test below 5 s + 11 s: 161 s together, against the compressor selection's 73 s."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_derive.py"), "-k", DERIVE_ON_THE_EMULATOR[order]])


# the streams that are wrong or odd: what the walks read at and behind the end of a stream
DERIVE_UNDER_ASAN = "truncated or more_nodes or fewer_nodes or run_of_zeros or reference_ or contradict or unary or legal_but"


@pytest.mark.skipif(not os.environ.get("BVG_EMU_ASAN"), reason="opt-in (BVG_EMU_ASAN=1): the AddressSanitizer build of the emulated library takes ~4 minutes to compile")
def test_offsets_derivation_of_wrong_streams_under_address_sanitizer():
    """The status-parity cases of tests/test_gpu_derive.py -- truncated streams, a run of zeros to the end, more nodes than records, contradicting
    counts, references out of range -- and the unary codes beyond 64 bits under ASan + UBSan, before they go to a GPU: the walks read ahead of
    the position (BitBuf: the two words behind the current one; derive_crawl_kernel: nine bytes from every bit of the chunk; the word-at-a-time
    unary scan), and a read behind the padded copy of the stream is silent on the hardware."""
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "asan"])
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    _gpu_file_on_the_emulator(os.path.join(EMU, "libbvgraph_emu_asan.so"), "fwd", [os.path.join(ROOT, "tests", "test_gpu_derive.py"), "-k", DERIVE_UNDER_ASAN],
                              LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")


@pytest.mark.parametrize("order,first", [("fwd", 0), ("rev", 10)])
def test_randomised_offsets_derivation_on_the_emulator(emu_lib, order, first):
    """tests/test_gpu_derive_fuzz.py, ten cases per lane order; the two orders run different cases."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_derive_fuzz.py")], BVG_DERIVE_FUZZ=str(first + 10), BVG_DERIVE_FUZZ_FROM=str(first))


@pytest.mark.skipif(not os.environ.get("BVG_EMU_ASAN"), reason="opt-in (BVG_EMU_ASAN=1): the AddressSanitizer build of the emulated library takes ~4 minutes to compile")
def test_compressor_input_check_under_address_sanitizer():
    """test_degenerate_adjacencies sends offsets that point a million elements past a three-element adjacency: enc_check_kernel must refuse
    them without reading adj (before the check compared with adj_off[nodes], this run ended in an ASan report)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "asan"])
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    _gpu_file_on_the_emulator(os.path.join(EMU, "libbvgraph_emu_asan.so"), "fwd", [os.path.join(ROOT, "tests", "test_gpu_store.py"), "-k", "degenerate or min_interval or one_tile"],
                              LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")


# what of tests/test_gpu_labels.py each lane order runs here (the GPU run has all of it)
LABELS_ON_THE_EMULATOR = {
    "fwd": "not parameter_space or random",
    "rev": "prefix_sum or ranges_on_one_handle or workspace_reuse or end_of_stream or capacity or dev_entry",
}
# the streams that are wrong, and the streams that end on the last bit of the file: what the kernels read at and behind the end of a stream
LABELS_UNDER_ASAN = "defect or hand_assembled or end_of_stream or files_that_are_wrong"


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_arc_label_suite_on_the_emulator(emu_lib, order):
    """tests/test_gpu_labels.py -- the arc-label decoder against the plain model of tests/labels_model.py -- on the CPU.  The label kernels have no
    cross-lane traffic, but the prefix sum they share with the decoder (csrc/bvg_kernels.hip: scan_partials, scan_partials_serial, scan_final) adds up
    across the lanes of a wavefront and through LDS behind a __syncthreads(), so both lane orders run: the forward order everything kept, the reversed
    order the tests that vary the number of nodes and arcs that are scanned.  Cut from the emulated selection, for time only (all of it runs on the GPU):
    three of the four value patterns of the sweep over every width (test_parameter_space: 1 - 2.6 s per class and pattern here).  The status-parity cases
    (every defect, the hand-assembled codes), the end-of-stream cases and the file cases run here in full, before any GPU sees them.
    Measured on one machine, next to the figures of test_offsets_derivation_suite_on_the_emulator: the whole file 33 s; this selection 19 s (fwd) +
    9 s (rev), the randomised test below 1.5 s per order: 32 s together."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_labels.py"), "-k", LABELS_ON_THE_EMULATOR[order]])


@pytest.mark.parametrize("order,first", [("fwd", 0), ("rev", 10)])
def test_randomised_arc_labels_on_the_emulator(emu_lib, order, first):
    """tests/test_gpu_labels_fuzz.py, ten cases per lane order (13 ms a case here); the two orders run different cases."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_labels_fuzz.py")], BVG_LABELS_FUZZ=str(first + 10), BVG_LABELS_FUZZ_FROM=str(first))


@pytest.mark.skipif(not os.environ.get("BVG_EMU_ASAN"), reason="opt-in (BVG_EMU_ASAN=1): the AddressSanitizer build of the emulated library takes ~4 minutes to compile")
def test_arc_labels_of_wrong_streams_under_address_sanitizer():
    """The status-parity cases of tests/test_gpu_labels.py -- truncated streams, flipped bits, degrees off by one, an all-zero stream, gamma codes of 64 zeros
    and more, list lengths without elements -- and the streams that end on the last bit of the file, under ASan + UBSan, before they go to a GPU:
    BitCursor::peek_global loads nine bytes from the byte of every position (clamped to the last 16 bytes of the padded copy), and a read behind the copy
    is silent on the hardware."""
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "asan"])
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    _gpu_file_on_the_emulator(os.path.join(EMU, "libbvgraph_emu_asan.so"), "fwd", [os.path.join(ROOT, "tests", "test_gpu_labels.py"), "-k", LABELS_UNDER_ASAN],
                              LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")


# what of tests/test_gpu_batch.py each lane order runs here (the GPU run has all of it); the forward order in two parts, for the time limit of one run
BATCH_ON_THE_EMULATOR = {
    "fwd": "not deep_and_ordinary and not frontier_route and not (prefix_sum and (655 or 70000)) and not (parameter_space and not copies)",
    "fwd-deep": "deep_and_ordinary",
    "rev": "reach_boundary or (deep_and_ordinary and not 1500) or (prefix_sum and not 655 and not 70000)",
}


@pytest.mark.parametrize("part", sorted(BATCH_ON_THE_EMULATOR))
def test_random_access_suite_on_the_emulator(emu_lib, part):
    """tests/test_gpu_batch.py -- bvg_successors_batch against the adjacency the test wrote down, list for list -- on the CPU.  The forward
    order runs everything that fits: the reach boundary, deep and ordinary requests together (a part of its own), the capacity contract and
    the workspace growth and the streams that are wrong IN FULL (items 1, 2, 5 and 9: this is where they are seen first), every tier in one
    batch, the handles, the wide windows.  The reversed order runs the reach boundary, the deep batches up to 257 requests and the batch
    sizes up to 4 096: the prefix sum and the row kernel's cross-lane traffic are what the order can break.  Cut from the emulated
    selection, for time only (all of it runs on the GPU): the batches of 65 535, 65 536, 65 537 and 70 000 requests (96 - 100 s each
    here; the levels of the prefix sum are crossed here at 1 023 .. 4 096 requests, its serial level's second pass only on the GPU), the
    parameter sets of the shapes other than "copies" (43 x 2 - 5 s), and the visit on the frontier route (the emulated library is built
    without bvg_bfs).  The deep batches of 1 500 requests are the dearest thing kept: they belong to item 2, which runs here whole.
    Measured on one machine, next to the figures of test_arc_label_suite_on_the_emulator: the deep batches of 1 500 requests 204 s (some
    4 600 requests decoded one by one), the other deep batches 130 s, the reach boundary 36 s, the workspace growth 27 s, the tiers 20 s;
    the two forward parts together 1 030 s with the batch of 65 537 requests (96 s, cut since: about 930 s), the reversed order 226 s, the
    randomised test below 103 s + 11 s."""
    _gpu_file_on_the_emulator(emu_lib, part.split("-")[0], [os.path.join(ROOT, "tests", "test_gpu_batch.py"), "-k", BATCH_ON_THE_EMULATOR[part]])


@pytest.mark.parametrize("order,first", [("fwd", 0), ("rev", 11)])
def test_randomised_random_access_on_the_emulator(emu_lib, order, first):
    """tests/test_gpu_batch_fuzz.py, ten cases per lane order; the two orders run different cases.  A case costs 1 - 20 s here, except the
    draws of 6 000 nodes with long chains and thousands of requests, whose deep requests are decoded one by one (a minute and more: case 8
    of this seed 59 s, case 10 -- left out, for time -- over a minute): the seed is one whose other cases are short (116 s for the first ten)."""
    _gpu_file_on_the_emulator(emu_lib, order, [os.path.join(ROOT, "tests", "test_gpu_batch_fuzz.py")], BVG_BATCH_FUZZ=str(first + 10), BVG_BATCH_FUZZ_FROM=str(first),
                              BVG_BATCH_FUZZ_SEED="7")


@pytest.mark.skipif(not os.environ.get("BVG_EMU_ASAN"), reason="opt-in (BVG_EMU_ASAN=1): the AddressSanitizer build of the emulated library takes ~4 minutes to compile")
@pytest.mark.parametrize("with_deep", [False, True])
def test_workspace_growth_replayed_under_address_sanitizer(W, tmp_path, with_deep):
    """When the successors no longer fit, bvg_successors_batch frees its workspace, takes a larger one and prepares the batch again in it.
    Without that second preparation the decode reads the plan, the halos and the prefix sums from the block that was freed: the values are
    usually still there, on the host and on the device, so no comparison sees it -- AddressSanitizer does.  The calls of
    test_workspace_growth_between_the_two_preparations (tests/test_gpu_batch.py) are written to files and replayed on one fresh handle by
    tests/emu/batch_replay.cpp: a program of its own, linked against the sanitizer build of the emulated library, with nothing preloaded."""
    import numpy as np
    import batch_cases as BC
    import test_gpu_batch as TB
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU, "replay_asan"])
    h = TB.Hand(W, 7)
    (tmp_path / "params.bin").write_bytes(bytes(h.st.params))
    (tmp_path / "graph.bin").write_bytes(h.st.graph.tobytes())
    (tmp_path / "offsets.bin").write_bytes(h.st.offsets.tobytes())
    calls = TB.growth_calls(h, with_deep)
    for name, nodes in calls:
        deg, succ = BC.expected(h.st.lists, nodes)
        for ext, a, t in ((".nodes", nodes, "int64"), (".deg", deg, "int32"), (".succ", succ, "int64")):
            (tmp_path / (name + ext)).write_bytes(np.asarray(a, dtype=t).tobytes())
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    out = subprocess.run([os.path.join(EMU, "build", "batch_replay_asan"), str(tmp_path)] + [name for name, _ in calls], env=e, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "replay ok" in out.stdout and "ERROR: AddressSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-6000:]


def test_randomised_parity_of_the_lean_kernels_on_the_emulator(emu_lib):
    """tests/emu/fuzz_flat.py: random shapes, windows, reference-chain depths, interval lengths, zeta k, LDS geometries (small pools: sub-rows and compaction), records per
    super-row and lane orders; scan_kernel and the experimental flat kernel against the oracle (8 cases here; 90 ran on the final round-5 tree: BVG_EMU_FUZZ=<n> for more)."""
    n = os.environ.get("BVG_EMU_FUZZ", "8")
    out = subprocess.run([sys.executable, os.path.join(EMU, "fuzz_flat.py"), n, "5"], capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout[-3000:] + out.stderr[-1500:]


def test_dense_graph_through_the_emulated_kernels(emu_lib):
    out = run_case(6000, 5, "eu", 3)
    assert "emu case ok" in out and "lean_blocks 0 " not in out.splitlines()[2]


@pytest.mark.parametrize("dbg,order", [(4096, "fwd"), (8192, "rev"), (12288, "fwd")])
def test_round6_list_builds_on_the_emulator(emu_lib, dbg, order):
    """scan_kernel's two round-6 experiments (compiled into the emulated and the experimental library only; both measured slower: csrc/bvg_scan.hip, "MEASURED") stay bit-exact:
    WW (BVG_DBG=4096: stored lists with reference built wave-wide from lane bit vectors) and ZE (8192: position tasks by kept element over the extras' bit vectors)."""
    out = run_case(6000, 5, "eu", 3, BVG_DBG=dbg, BVG_EMU_ORDER=order)
    assert "emu case ok" in out and "lean_blocks 0 " not in out.splitlines()[2]
