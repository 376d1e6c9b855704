"""Breadth-first visit on the device (bvg_bfs_visit) against the same visit driven from the host through bvg_successors_batch.

  python profiles/bfs_bench.py [--shape eu|cnr] [--gib G] [--route frontier|sweep] [--switch DEN] [--no-host]

The two graphs of profiles/components_bench.py: the eu-like stand-in (one 2^21-node tools.eu_like base) and cnr-2000 from tests/golden/, tiled on
the device to >= G GiB of stream, so that one visit reaches one tile: the largest weak component of the base, from its smallest node.
Device visit: --warmup calls, then --steps timed (wall clock around clear + visit; the queue, cut points and dist stay on the device and are
read once, afterwards, for the check against a CPU search of the base).  Host visit (the baseline a caller had before): the frontier goes to
bvg_successors_batch level by level, marking with numpy.  --route forces one route for every level (BVG_BFS_ROUTE under the test knobs) and
--switch sets the denominator of the switch point: run the three variants to read the per-level crossover off the lines this prints
(level, frontier nodes, frontier arcs, share of the graph's arcs).  Prints traversed arcs/s and one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("BVG_TEST_KNOBS", "1")
import numpy as np

import webgraph_big_amd as W
import tooling as T
from test_gpu_bfs import cpu_bfs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="eu", choices=["eu", "cnr"])
    ap.add_argument("--gib", type=float, default=0.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--route", default=None, choices=["frontier", "sweep"])
    ap.add_argument("--switch", type=int, default=0)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if args.route:
        os.environ["BVG_BFS_ROUTE"] = args.route
    if args.switch:
        os.environ["BVG_BFS_SWITCH"] = str(args.switch)
    if args.shape == "eu":
        n0 = 1 << 21
        st = T.synth_store(n0, seed=0, synth=T.eu_like(), threads=16)
        off0, adj0 = T.synth_adjacency(n0, seed=0, synth=T.eu_like())
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
    off0 = np.asarray(off0, dtype=np.int64)
    # the start: the smallest node from which the visit is largest among a few candidates (node 0 and the heads of the longest lists)
    cands = sorted(set([0] + np.argsort(-np.diff(off0))[:4].tolist()))
    start = max(cands, key=lambda s: (len(cpu_bfs(off0, adj0, s)[0]), -s))
    queue, cuts, dist, _ = cpu_bfs(off0, adj0, start)
    deg0 = np.diff(off0)
    level_arcs = [int(deg0[queue[cuts[d]:cuts[d + 1]]].sum()) for d in range(len(cuts) - 1)]
    traversed = int(sum(level_arcs))
    base = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    copies = max(1, int(np.ceil(gib * (1 << 30) / len(st.graph))))
    g = base.tile(copies)
    arcs = int(off0[-1]) * copies
    for d, a in enumerate(level_arcs):
        print("level %3d: %9d nodes %11d arcs = %.4f %% of the graph" % (d, cuts[d + 1] - cuts[d], a, 100.0 * a / arcs))
    v = g.breadth_first_visit()

    def device():
        t0 = time.perf_counter()
        v.clear()
        k = v.visit(start)
        dt = time.perf_counter() - t0
        assert k == len(queue), (k, len(queue))
        return dt
    dev = [device() for _ in range(args.warmup + args.steps)]
    assert np.array_equal(v.queue, queue) and np.array_equal(v.cut_points, cuts) and np.array_equal(v.dist[:n0], dist)
    counters = v.counters()
    host = []
    if not args.no_host:
        def host_visit():
            t0 = time.perf_counter()
            seen = np.zeros(g.num_nodes(), dtype=bool); seen[start] = True
            frontier = np.array([start], dtype=np.int64); total = 1
            while len(frontier):
                _, succ = g.successors_batch(frontier)
                nxt = np.unique(succ[~seen[succ]])
                seen[nxt] = True; total += len(nxt); frontier = nxt
            assert total == len(queue)
            return time.perf_counter() - t0
        host = [host_visit() for _ in range(args.warmup + args.steps)]
    td = min(dev[args.warmup:]); th = min(host[args.warmup:]) if host else None
    res = {"shape": args.shape, "copies": copies, "nodes": g.num_nodes(), "arcs": arcs, "start": int(start), "visited": int(len(queue)), "levels": len(cuts) - 1,
           "traversed_arcs": traversed, "route": args.route or "auto", "switch": args.switch or 16, "device_s": td, "device_arcs_per_s": traversed / td,
           "host_s": th, "host_arcs_per_s": (traversed / th) if th else None, "counters": counters, "device_all_s": dev, "host_all_s": host}
    print("%s: visit from %d reaches %d nodes in %d levels, %d arcs traversed: device %.1f ms -> %.3f G arcs/s%s" % (
        args.shape, start, len(queue), len(cuts) - 1, traversed, td * 1e3, traversed / td / 1e9,
        "; host-driven %.1f ms -> %.3f G arcs/s" % (th * 1e3, traversed / th / 1e9) if th else ""))
    print("JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
