"""EFGraph on the device beside BVGraph on the same graph: scan, materialise, random access, skipTo, store.

  python profiles/efgraph_bench.py [--log2-nodes 21] [--log2-quantum 8] [--warmup 3] [--steps 10]

The graph is the eu-like stand-in of tooling (tools.eu_like) with 2^21 nodes, stored once as a BVGraph (tooling's CPU encoder) and once as an
EFGraph (bvg_ef_store, which is also what "store" times).  Every figure is the best and the median of `steps` runs after `warmup` runs:
  bv_scan / ef_scan   bvg_scan / bvg_ef_scan of all nodes; time = the call's own hipEvent time (kernel_ms); edges/s, stream bytes per arc and, for
                      EF, (graph_bytes + index_bytes) / time as a share of the 8 TB/s HBM bound.  The two checksums must agree.
  ef_materialise      bvg_ef_decode_range_dev of all nodes into device buffers (wall clock of the synchronous call)
  ef_random_access    bvg_ef_successors_batch of 2^20 random nodes, host buffers (wall clock: includes the copies over PCIe)
  ef_skip_to          bvg_ef_skip_to_batch of 2^20 random (node, bound) pairs, with the pointers and with BVG_EF_NOPTR=1: the kernel's hipEvent
                      time and the wall clock of the call
  ef_store            bvg_ef_store from the host CSR (wall clock: upload, kernels, download)
Prints one line per figure and one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("BVG_TEST_KNOBS", "1")                                  # (BVG_EF_NOPTR is a test knob)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-nodes", type=int, default=21)
    ap.add_argument("--log2-quantum", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    import torch                                                             # (before the product library: one HIP runtime)
    import numpy as np
    import webgraph_big_amd as W
    import tooling as T
    torch.cuda.init()
    n = 1 << a.log2_nodes
    synth = T.eu_like()
    st = T.synth_store(n, seed=0, synth=synth, threads=16)
    off, adj = T.synth_adjacency(n, seed=0, synth=synth)
    off = np.ascontiguousarray(off, dtype=np.uint64); adj = np.ascontiguousarray(adj, dtype=np.int64)
    arcs = int(off[-1])
    out = {"nodes": n, "arcs": arcs, "log2_quantum": a.log2_quantum, "warmup": a.warmup, "steps": a.steps}

    def timed(name, call, **extra):
        ts = [call() for _ in range(a.warmup + a.steps)][a.warmup:]
        out[name] = dict(best_s=min(ts), median_s=statistics.median(ts), **extra)
        return min(ts)

    def report(name, **kw):
        out[name].update(kw)
        print("%s: %s" % (name, json.dumps(out[name])), flush=True)

    # store (and the EF stream every later figure reads)
    kept = {}

    def store():
        t0 = time.perf_counter()
        kept["ef"] = W.store_efgraph((off, adj), n, a.log2_quantum)
        return time.perf_counter() - t0
    t = timed("ef_store", store)
    data, ef_off = kept["ef"]
    report("ef_store", edges_per_s=arcs / t, stream_bytes=len(data), bits_per_arc=8 * len(data) / arcs)

    bv = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    ef = W.EFGraph.from_memory(W.EFParams(nodes=n, arcs=arcs, upper_bound=n, log2_quantum=a.log2_quantum, big_endian=0), data, ef_off)
    last = {}

    def scan_of(g, key):
        def call():
            last[key] = g.scan()
            return last[key]["kernel_ms"] * 1e-3
        return call
    t = timed("bv_scan", scan_of(bv, "bv"))
    report("bv_scan", edges_per_s=arcs / t, bytes_per_arc=last["bv"]["graph_bytes"] / arcs, launches=last["bv"]["launches"])
    t = timed("ef_scan", scan_of(ef, "ef"))
    assert (last["ef"]["arcs"], last["ef"]["chk"]) == (last["bv"]["arcs"], last["bv"]["chk"]) == (arcs, last["bv"]["chk"]), (last["ef"], last["bv"])
    read = last["ef"]["graph_bytes"] + last["ef"]["index_bytes"]
    report("ef_scan", edges_per_s=arcs / t, bytes_per_arc=last["ef"]["graph_bytes"] / arcs, bytes_read=read, hbm_share=read / t / HBM_BYTES_PER_S,
           launches=last["ef"]["launches"])

    L = W.efgraph._ef_fns()
    d_deg = torch.empty(n, dtype=torch.int32, device="cuda"); d_succ = torch.empty(arcs, dtype=torch.int64, device="cuda"); need = C.c_uint64()

    def materialise():
        t0 = time.perf_counter()
        s = L.bvg_ef_decode_range_dev(ef._h, 0, n, d_deg.data_ptr(), d_succ.data_ptr(), arcs, C.byref(need))
        assert s == 0 and need.value == arcs, (s, need.value)
        return time.perf_counter() - t0
    t = timed("ef_materialise", materialise)
    assert torch.equal(d_succ[:1 << 16].cpu(), torch.from_numpy(adj[:1 << 16]))
    report("ef_materialise", edges_per_s=arcs / t)

    rng = np.random.default_rng(0)
    nodes = rng.integers(0, n, size=1 << 20)
    got = {}

    def batch():
        t0 = time.perf_counter()
        got["b"] = ef.successors_batch(nodes)
        return time.perf_counter() - t0
    t = timed("ef_random_access", batch)
    report("ef_random_access", requests=len(nodes), arcs=int(len(got["b"][1])), requests_per_s=len(nodes) / t, edges_per_s=len(got["b"][1]) / t)

    bounds = rng.integers(0, n, size=1 << 20)
    for name, env in (("ef_skip_to", None), ("ef_skip_to_no_pointers", "1")):
        if env:
            os.environ["BVG_EF_NOPTR"] = env
        kms = []

        def skip():
            t0 = time.perf_counter()
            got[name] = ef.skip_to(nodes, bounds)
            dt = time.perf_counter() - t0
            kms.append(ef.last_kernel_ms())
            return dt
        t = timed(name, skip)
        k = min(kms[a.warmup:])
        report(name, queries=len(nodes), kernel_ms=k, queries_per_s_kernel=len(nodes) / (k * 1e-3), queries_per_s_call=len(nodes) / t)
        os.environ.pop("BVG_EF_NOPTR", None)
    assert np.array_equal(got["ef_skip_to"], got["ef_skip_to_no_pointers"])
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
