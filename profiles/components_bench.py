"""Weakly connected components (bvg_components_dev) against the materialising decode (bvg_decode_range_dev) on the same graph.

  python profiles/components_bench.py [--shape eu|cnr] [--gib G]

eu: the eu-like stand-in (one 2^21-node tools.eu_like base, as profiles/mat_bench.py) tiled on the device to >= G GiB of stream (default 8);
cnr: cnr-2000 from tests/golden/ tiled to G GiB (default 4).  Components: 3 warm-up calls, then 5 timed (wall clock, labels into a device
tensor).  Decode: the same node range materialised through bvg_decode_range_dev in node ranges of <= 2^32 arcs (the graph does not fit in
HBM as a CSR), 3 warm-up passes, then 5 timed.  The labels of a few tiles are checked against a CPU union-find of the base (tile j's
labels = the base's + j * C0).  Prints edges/s of both and one JSON line; run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel split (profiles/r07_components_*).
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


def cpu_components(n, off, adj):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    off = np.asarray(off, dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    k, lab = connected_components(coo_matrix((np.ones(len(adj), np.int8), (src, np.asarray(adj, np.int64))), shape=(n, n)).tocsr(), directed=True, connection="weak")
    first = np.full(k, n, dtype=np.int64); np.minimum.at(first, lab, np.arange(n, dtype=np.int64))
    rank = np.empty(k, dtype=np.int64); rank[np.argsort(first, kind="stable")] = np.arange(k, dtype=np.int64)
    return int(k), rank[lab]


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
    c0, comp0 = cpu_components(n0, off0, adj0)
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    copies = max(1, int(np.ceil(gib * (1 << 30) / len(st.graph))))
    g = base.tile(copies)
    n = g.num_nodes(); arcs = int(off0[-1]) * copies
    L = W.lib(); W.bvgraph._components_fns()
    comp = torch.empty(n, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()

    def components():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = L.bvg_components_dev(g._h, 0, comp.data_ptr(), None, 0, C.byref(cnt))
        torch.cuda.synchronize()
        assert s == 0, s
        return time.perf_counter() - t0
    cc = [components() for _ in range(args.warmup + args.steps)]
    assert cnt.value == copies * c0, (cnt.value, copies, c0)
    t0 = torch.from_numpy(comp0).cuda()
    for j in (0, copies // 2, copies - 1):
        assert torch.equal(comp[j * n0:(j + 1) * n0], t0 + j * c0), "tile %d" % j
    del t0
    # the materialising decode over the same nodes, in node ranges of <= 2^32 arcs
    parts = max(1, -(-arcs // (1 << 32)))
    bounds = g.split_by_arcs(parts)
    cap = max(int(bounds[i + 1] - bounds[i]) for i in range(parts))
    deg = torch.empty(cap, dtype=torch.int32, device="cuda")
    need_max = 0
    need = C.c_uint64()
    for i in range(parts):
        s = L.bvg_decode_range_dev(g._h, int(bounds[i]), int(bounds[i + 1]), deg.data_ptr(), None, 0, C.byref(need))
        need_max = max(need_max, int(need.value))
    del comp
    succ = torch.empty(max(need_max, 1), dtype=torch.int64, device="cuda")

    def decode():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(parts):
            s = L.bvg_decode_range_dev(g._h, int(bounds[i]), int(bounds[i + 1]), deg.data_ptr(), succ.data_ptr(), need_max, C.byref(need))
            assert s == 0, s
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    dec = [decode() for _ in range(args.warmup + args.steps)]
    tc, td = min(cc[args.warmup:]), min(dec[args.warmup:])
    res = {"shape": args.shape, "copies": copies, "nodes": n, "arcs": arcs, "stream_bytes": int(len(st.graph)) * copies, "components": int(cnt.value),
           "components_s": tc, "components_edges_per_s": arcs / tc, "decode_s": td, "decode_edges_per_s": arcs / td, "decode_parts": parts,
           "ratio": td / tc, "components_all_s": cc, "decode_all_s": dec}
    print("%s: %d nodes, %d arcs (%d tiles), %d components: components %.1f ms -> %.1f G edges/s; materialise %.1f ms -> %.1f G edges/s; ratio %.2f"
          % (args.shape, n, arcs, copies, cnt.value, tc * 1e3, arcs / tc / 1e9, td * 1e3, arcs / td / 1e9, td / tc))
    print("JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
