"""Exact geometric centralities (bvg_geometric_dev) of 512 sources against the alternative the library had before: 512 calls of
bvg_bfs_visit, each followed by a histogram of its distances on the host, on the same sources and in the same run.

  python profiles/geometric_bench.py [--shape cnr|eu] [--sources 512] [--first X] [--nodes N]

cnr: cnr-2000 from tests/golden/; eu: one eu-like stand-in of N nodes (tools.eu_like, default 2^20).  The sources are [first, first + sources)
(default first: a quarter into the graph).  For every W in 1, 2, 4, 8 (BVG_GEO_WORDS) and for the default: --warmup calls, then --steps
timed ones (wall clock around the call, results into device tensors), the median reported with the spread, and the time per sweep.  The
visits: every source once, timed as a whole (the loop is too long to repeat; one warm-up visit before it).  The two histograms must be
equal.  Prints one line per configuration, the ratio, and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("BVG_TEST_KNOBS", "1")                                 # BVG_GEO_WORDS is a test knob
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch                                                                 # (before the product library: one HIP runtime)
import numpy as np

import webgraph_big_amd as W
import tooling as T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cnr", choices=["eu", "cnr"])
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--sources", type=int, default=512)
    ap.add_argument("--first", type=int, default=-1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-visits", action="store_true", help="leave the 512 visits out")
    args = ap.parse_args()
    torch.cuda.init()
    if args.shape == "eu":
        st = T.synth_store(args.nodes, seed=0, synth=T.eu_like(), threads=16)
        g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    else:
        g = W.BVGraph.load(os.path.join(ROOT, "tests", "golden", "cnr-2000"))
    n = g.num_nodes()
    first = args.first if args.first >= 0 else n // 4
    sources = (first, min(n, first + args.sources))
    k = sources[1] - sources[0]
    cen = torch.empty(k, dtype=torch.float32, device="cuda"); rea = torch.empty(k, dtype=torch.int64, device="cuda")
    res = {"shape": args.shape, "nodes": n, "sources": list(sources), "runs": {}}
    hist = None
    for words in (1, 2, 4, 8, None):
        if words is None:
            os.environ.pop("BVG_GEO_WORDS", None)
        else:
            os.environ["BVG_GEO_WORDS"] = str(words)
        ts = []
        for _ in range(args.warmup + args.steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            h, c = g.linear_geometric_centrality_dev("harmonic", cen, rea, sources=sources, histogram=True)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        assert hist is None or np.array_equal(h, hist)
        hist = h
        t = ts[args.warmup:]
        med = statistics.median(t)
        name = "default" if words is None else "W=%d" % words
        res["runs"][name] = {"median_s": med, "min_s": min(t), "max_s": max(t), "counters": c, "ms_per_sweep": med * 1e3 / c["sweeps"]}
        print("%-8s %d sources: %8.2f ms (min %.2f, max %.2f; %d timed), %d words, %d passes, %d sweeps, %.3f ms per sweep, resident batch %d"
              % (name, k, med * 1e3, min(t) * 1e3, max(t) * 1e3, len(t), c["words_per_node"], c["passes"], c["sweeps"], med * 1e3 / c["sweeps"], c["single_resident_batch"]))
    res["histogram"] = [int(v) for v in hist]
    if not args.no_visits:
        with g.breadth_first_visit() as v:
            v.visit(sources[0]); v.clear()                                    # warm-up
            total = np.zeros(len(hist) + 1, dtype=np.int64)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for s in range(*sources):
                v.clear()
                v.visit(s)
                d = v.dist
                b = np.bincount(d[d >= 0])
                total[:len(b)] += b
            tv = time.perf_counter() - t0
        assert np.array_equal(np.trim_zeros(total, "b").astype(np.uint64), hist), "the visits' histogram differs"
        best = res["runs"]["default"]["median_s"]
        res.update(visits_s=tv, ratio_visits_to_geometric=tv / best)
        print("visits   %d sources: %8.2f ms (bvg_bfs_visit + host histogram, once); %.1f x the default multi-source run" % (k, tv * 1e3, tv / best))
    print("JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
