"""Strongly connected components (bvg_scc_dev) against the weakly connected ones (bvg_components_dev) on the same graph, in the same run.

  python profiles/scc_bench.py [--shape eu|cnr] [--gib G]

eu: the eu-like stand-in (one 2^21-node tools.eu_like base, as profiles/components_bench.py) tiled on the device to >= G GiB of stream
(default 8); cnr: cnr-2000 from tests/golden/ tiled to G GiB (default 4).  Each of the two: 3 warm-up calls, then 5 timed (wall clock,
labels into a device tensor), the best one reported.  The labels of a few tiles are checked against scipy's strong components of the base
(tile j's labels = the base's + j * C0).  Prints the wall time, the counters of bvg_scc (sweeps, batch decodes, trim passes, ...), the
ratio to bvg_components and one JSON line.  No rate is promised: the cost is one sweep per hop of the longest propagation chain.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch                                                                 # (before the product library: one HIP runtime)
import numpy as np

import webgraph_big_amd as W
import tooling as T
from scc_cases import arcs_of, cpu_scc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="eu", choices=["eu", "cnr"])
    ap.add_argument("--gib", type=float, default=0.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()
    if args.shape == "eu":
        n0 = 1 << 21
        st = T.synth_store(n0, seed=0, synth=T.eu_like(), threads=16)
        off0, adj0 = T.synth_adjacency(n0, seed=0, synth=T.eu_like())          # (the same generator and seed: the same graph)
        assert int(off0[-1]) == int(st.stats["arcs"])
        gib = args.gib or 8.0
    else:
        import gzip
        with gzip.open(os.path.join(ROOT, "tests", "golden", "cnr-2000.graph-txt.gz"), "rb") as f:
            lines = f.read().split(b"\n")
        n0 = int(lines[0])
        lists = [np.array(l.split(), dtype=np.int64) for l in lines[1:n0 + 1]]
        off0 = np.zeros(n0 + 1, dtype=np.uint64); off0[1:] = np.cumsum([len(l) for l in lists])
        adj0 = np.concatenate(lists)
        st = T.store((off0, adj0), W.default_params(min_interval_length=3), threads=16)
        gib = args.gib or 4.0
    c0, comp0, sizes0, _ = cpu_scc(n0, *arcs_of(off0, adj0))
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    copies = max(1, int(np.ceil(gib * (1 << 30) / len(st.graph))))
    g = base.tile(copies)
    n = g.num_nodes(); arcs = int(off0[-1]) * copies
    L = W.lib(); W.bvgraph._components_fns(); W.bvgraph._scc_fns()
    comp = torch.empty(n, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()
    ctr = np.zeros(len(W.SCC_COUNTERS), dtype=np.uint64)

    def scc():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = L.bvg_scc_dev(g._h, 0, comp.data_ptr(), None, 0, C.byref(cnt), None, ctr.ctypes.data)
        torch.cuda.synchronize()
        assert s == 0, s
        return time.perf_counter() - t0
    ts = [scc() for _ in range(args.warmup + args.steps)]
    assert cnt.value == copies * c0, (cnt.value, copies, c0)
    n_scc = int(cnt.value)
    t0 = torch.from_numpy(comp0).cuda()
    for j in (0, copies // 2, copies - 1):
        assert torch.equal(comp[j * n0:(j + 1) * n0], t0 + j * c0), "tile %d" % j
    del t0

    def components():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = L.bvg_components_dev(g._h, 0, comp.data_ptr(), None, 0, C.byref(cnt))
        torch.cuda.synchronize()
        assert s == 0, s
        return time.perf_counter() - t0
    tc = [components() for _ in range(args.warmup + args.steps)]
    a, b = min(ts[args.warmup:]), min(tc[args.warmup:])
    counters = dict(zip(W.SCC_COUNTERS, (int(v) for v in ctr)))
    res = {"shape": args.shape, "copies": copies, "nodes": n, "arcs": arcs, "stream_bytes": int(len(st.graph)) * copies, "scc": n_scc, "largest_scc_of_base": int(sizes0.max()),
           "scc_s": a, "components_s": b, "ratio_to_components": a / b, "counters": counters, "scc_all_s": ts, "components_all_s": tc}
    print("%s: %d nodes, %d arcs (%d tiles), %d strong components: scc %.1f ms, components %.1f ms, ratio %.1f; %s"
          % (args.shape, n, arcs, copies, n_scc, a * 1e3, b * 1e3, a / b, counters))
    print("JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
