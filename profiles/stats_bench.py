"""Graph statistics (bvg_stats_compute) against weakly connected components (bvg_components_dev) on the same graph, and the two forms of
the indegree scatter against each other.

  python profiles/stats_bench.py [--shape eu|web|cnr] [--gib G]

eu / web: one 2^21-node tools.eu_like / tools.web_like base tiled on the device to >= G GiB of stream (default 8); cnr: cnr-2000 from
tests/golden/ tiled to G GiB (default 4).  The scatter form is a test knob of the library read in a fresh process, so every measurement
runs in a child: whole calls (3 warm-up, 5 timed, wall clock) with the plain and with the electing scatter, bvg_components_dev the same
way as the yardstick, and one call of each form under BVG_DEBUG, whose log line splits the call into decode and arc kernel (with a
stream synchronisation after each, which the timed calls do not have).  The summary of one tile's worth is checked against numpy
(arcs, loops, the indegree distribution).  Prints one JSON line.
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


def child(args):
    import torch                                                             # (before the product library: one HIP runtime)
    import numpy as np
    import webgraph_big_amd as W
    import tooling as T
    torch.cuda.init()
    if args.shape in ("eu", "web"):
        n0 = 1 << 21
        synth = T.eu_like() if args.shape == "eu" else T.web_like()
        st = T.synth_store(n0, seed=0, synth=synth, threads=16)
        off0, adj0 = T.synth_adjacency(n0, seed=0, synth=synth)
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
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    copies = max(1, int(np.ceil(gib * (1 << 30) / len(st.graph))))
    g = base.tile(copies)
    n = g.num_nodes(); arcs = int(off0[-1]) * copies
    res = {"shape": args.shape, "copies": copies, "nodes": n, "arcs": arcs, "stream_bytes": int(len(st.graph)) * copies, "what": args.child}
    if args.child == "components":
        L = W.lib(); W.bvgraph._components_fns()
        comp = torch.empty(n, dtype=torch.int64, device="cuda"); cnt = C.c_uint64()

        def call():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s = L.bvg_components_dev(g._h, 0, comp.data_ptr(), None, 0, C.byref(cnt))
            torch.cuda.synchronize()
            assert s == 0, s
            return time.perf_counter() - t0
    else:
        L = W.bvgraph._stats_fns()
        last = {}

        def call():
            h = C.c_void_p()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s = L.bvg_stats_compute(g._h, 0, C.byref(h))
            dt = time.perf_counter() - t0
            assert s == 0, s
            sm = W.StatsSummary(); L.bvg_stats_get(h, C.byref(sm)); last["sm"] = sm
            ln = C.c_uint64(); L.bvg_stats_distribution(h, 1, None, 0, C.byref(ln))
            d = np.zeros(ln.value, dtype=np.uint64); L.bvg_stats_distribution(h, 1, d.ctypes.data, len(d), C.byref(ln)); last["in"] = d
            L.bvg_stats_close(h)
            return dt
    times = [call() for _ in range(args.warmup + args.steps)]
    if args.child != "components":
        sm = last["sm"]
        src = np.repeat(np.arange(n0, dtype=np.int64), np.diff(off0.astype(np.int64)))
        ind0 = np.bincount(adj0, minlength=n0)
        assert sm.arcs == arcs and sm.loops == copies * int(np.count_nonzero(src == adj0)), (sm.arcs, sm.loops)
        assert np.array_equal(last["in"], copies * np.bincount(ind0).astype(np.uint64))
    res["all_s"] = times; res["best_s"] = min(times[args.warmup:]); res["edges_per_s"] = arcs / res["best_s"]
    print("JSON " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="eu", choices=["eu", "web", "cnr"])
    ap.add_argument("--gib", type=float, default=0.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"shape": args.shape}
    runs = (("plain", "stats", {}, False), ("elect", "stats", {"BVG_STATS_SCATTER": "elect"}, False), ("components", "components", {}, False),
            ("plain_split", "stats", {}, True), ("elect_split", "stats", {"BVG_STATS_SCATTER": "elect"}, True))
    for name, what, env, split in runs:
        e = dict(os.environ, BVG_TEST_KNOBS="1", **env)
        e.pop("BVG_DEBUG", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--gib", str(args.gib), "--child", what]
        if split:
            e["BVG_DEBUG"] = "1"
            cmd += ["--warmup", "1", "--steps", "1"]
        else:
            cmd += ["--warmup", str(args.warmup), "--steps", str(args.steps)]
        r = subprocess.run(cmd, env=e, capture_output=True, text=True)
        if r.returncode != 0:                                                # (stop here: nothing more is started after a failure)
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("child %s failed with %d" % (name, r.returncode))
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("JSON ")][-1][5:])
        if split:
            m = re.findall(r"\[bvg\] stats: degrees ([\d.]+) ms, plan ([\d.]+) ms \((\d+) batches.*?decode ([\d.]+) ms, arcs ([\d.]+) ms \((\w+)\), indegrees ([\d.]+) ms", r.stderr)[-1]
            out[name] = {"degrees_ms": float(m[0]), "plan_ms": float(m[1]), "batches": int(m[2]), "decode_ms": float(m[3]), "arcs_ms": float(m[4]), "form": m[5], "indegrees_ms": float(m[6])}
        else:
            out[name] = {k: j[k] for k in ("best_s", "edges_per_s", "all_s")}
            out.update({k: j[k] for k in ("copies", "nodes", "arcs", "stream_bytes")})
        print("%s: %s" % (name, json.dumps(out[name])), flush=True)
    print("JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
