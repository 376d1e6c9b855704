"""HyperBall (bvg_hyperball_*) against the materialising decode (bvg_decode_range_dev) and bvg_components_dev on the same graph.

  python profiles/hyperball_bench.py [--shape eu|cnr] [--gib G] [--log2m 4,6,8] [--iterations K]

eu: the eu-like stand-in (one 2^21-node tools.eu_like base, as profiles/components_bench.py) tiled on the device to >= G GiB of stream
(default 8); cnr: cnr-2000 from tests/golden/ tiled to G GiB (default 4).  Per log2m: 3 warm-up runs of K iterations (init + K x iterate),
then 5 timed runs; every iteration is timed on its own (wall clock around bvg_hyperball_iterate, which ends with a synchronisation) and
the best of the 5 is reported per iteration, with arcs / s.  The share of arcs that passed the modified-bit test comes from one more run in
a child process under BVG_DEBUG (the library prints the count per iteration; that run synchronises per batch and is not timed).  The
materialising decode is the same nodes through bvg_decode_range_dev in node ranges of <= 2^32 arcs, and bvg_components_dev the same
graph, both 3 warm-up calls and best of 5.  The counters of tile 0 are checked against the numpy model (tests/hyperball_model.py) of the
base graph after the last iteration for the smallest log2m.  Prints a table and one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch                                                                 # (before the product library: one HIP runtime)
import numpy as np

import webgraph_big_amd as W
import tooling as T


def base_graph(shape):
    if shape == "eu":
        n0 = 1 << 21
        st = T.synth_store(n0, seed=0, synth=T.eu_like(), threads=16)
        off0, adj0 = T.synth_adjacency(n0, seed=0, synth=T.eu_like())          # (the same generator and seed: the same graph)
        return st, off0, adj0, 8.0
    import gzip
    with gzip.open(os.path.join(ROOT, "tests", "golden", "cnr-2000.graph-txt.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    n0 = int(lines[0])
    lists = [np.array(l.split(), dtype=np.int64) for l in lines[1:n0 + 1]]
    off0 = np.zeros(n0 + 1, dtype=np.uint64); off0[1:] = np.cumsum([len(l) for l in lists])
    adj0 = np.concatenate(lists)
    return T.store((off0, adj0), W.default_params(min_interval_length=3), threads=16), off0, adj0, 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="eu", choices=["eu", "cnr"])
    ap.add_argument("--gib", type=float, default=0.0)
    ap.add_argument("--log2m", default="4,6,8")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--passes-only", action="store_true", help="(the child run under BVG_DEBUG: one run per log2m, nothing timed)")
    args = ap.parse_args()
    log2ms = [int(x) for x in args.log2m.split(",")]
    torch.cuda.init()
    st, off0, adj0, dflt = base_graph(args.shape)
    n0 = len(off0) - 1
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    copies = max(1, int(np.ceil((args.gib or dflt) * (1 << 30) / len(st.graph))))
    g = base.tile(copies)
    n = g.num_nodes(); arcs = int(off0[-1]) * copies
    K = args.iterations
    if args.passes_only:
        for log2m in log2ms:
            with g.hyperball(log2m, seed=0) as hb:
                hb.init(0)
                for _ in range(K):
                    hb.iterate()
        return
    rows = []
    for log2m in log2ms:
        with g.hyperball(log2m, seed=0) as hb:
            per_it = []
            modified = []
            for _ in range(args.warmup + args.steps):
                hb.init(0)
                ts = []
                for _ in range(K):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    hb.iterate()
                    ts.append(time.perf_counter() - t0)
                    if len(per_it) == 0:
                        modified.append(hb.modified())
                per_it.append(ts)
            best = np.min(np.array(per_it[args.warmup:]), axis=0)
            if log2m == min(log2ms):                                          # tile 0 against the model of the base graph (tiles do not touch)
                import hyperball_model as M
                model = M.HyperBallModel(off0, adj0, log2m, seed=0)
                model.init(0)
                for _ in range(K):
                    model.iterate()
                assert np.array_equal(hb.registers(0, n0), model.regs), "tile 0 differs from the model"
            rows.append({"log2m": log2m, "iteration_s": best.tolist(), "modified": modified, "counter_bytes": 2 * n << log2m})
    # the share of arcs that passed the modified-bit test: a child under BVG_DEBUG
    env = dict(os.environ, BVG_DEBUG="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--gib", str(args.gib), "--log2m", args.log2m, "--iterations", str(K), "--passes-only"],
                           env=env, capture_output=True, text=True, timeout=3000)
    passed = [int(x) for x in re.findall(r"hyperball: iteration \d+: .* passed (\d+),", child.stderr)]
    assert child.returncode == 0 and len(passed) == K * len(log2ms), child.stderr[-2000:]
    for i, r in enumerate(rows):
        r["passed"] = passed[i * K:(i + 1) * K]
    # bvg_components_dev and the materialising decode on the same graph
    L = W.lib(); W.bvgraph._components_fns()
    comp = torch.empty(n, dtype=torch.int64, device="cuda")
    cnt = C.c_uint64()

    def components():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s = L.bvg_components_dev(g._h, 0, comp.data_ptr(), None, 0, C.byref(cnt))
        torch.cuda.synchronize()
        assert s == 0, s
        return time.perf_counter() - t0
    tc = min([components() for _ in range(args.warmup + args.steps)][args.warmup:])
    del comp
    parts = max(1, -(-arcs // (1 << 32)))
    bounds = g.split_by_arcs(parts)
    cap = max(int(bounds[i + 1] - bounds[i]) for i in range(parts))
    deg = torch.empty(cap, dtype=torch.int32, device="cuda")
    need_max = 0
    need = C.c_uint64()
    for i in range(parts):
        L.bvg_decode_range_dev(g._h, int(bounds[i]), int(bounds[i + 1]), deg.data_ptr(), None, 0, C.byref(need))
        need_max = max(need_max, int(need.value))
    succ = torch.empty(max(need_max, 1), dtype=torch.int64, device="cuda")

    def decode():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(parts):
            s = L.bvg_decode_range_dev(g._h, int(bounds[i]), int(bounds[i + 1]), deg.data_ptr(), succ.data_ptr(), need_max, C.byref(need))
            assert s == 0, s
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    td = min([decode() for _ in range(args.warmup + args.steps)][args.warmup:])
    print("%s: %d nodes, %d arcs (%d tiles); materialise %.1f ms -> %.1f G edges/s; components %.1f ms -> %.1f G edges/s"
          % (args.shape, n, arcs, copies, td * 1e3, arcs / td / 1e9, tc * 1e3, arcs / tc / 1e9))
    print("log2m iteration        ms   G arcs/s  passed share  modified   vs materialise  vs components")
    for r in rows:
        for k in range(K):
            t = r["iteration_s"][k]
            print("%5d %9d %9.1f %10.2f %13.4f %9d %16.3f %13.3f" % (r["log2m"], k, t * 1e3, arcs / t / 1e9, r["passed"][k] / arcs, r["modified"][k], td / t, tc / t))
    print("JSON " + json.dumps({"shape": args.shape, "copies": copies, "nodes": n, "arcs": arcs, "stream_bytes": int(len(st.graph)) * copies, "decode_s": td, "decode_parts": parts,
                                "components_s": tc, "iterations": K, "hyperball": rows}))


if __name__ == "__main__":
    main()
