"""The labelled transforms on the device beside the same operations done by the model (tests/labelled_model.py) on the host's cores, and the
arc-parallel labelled union beside the per-node unlabelled union on the same inputs.

  python profiles/labelled_bench.py [--copies 16] [--warmup 1] [--steps 5] [--no-model] [--star 1000000]

Two graphs: cnr-2000 (the golden fixture: 325 557 nodes, 3.2 M arcs) and its device tiling (bvg_tile, `copies` back-to-back copies), arc
(x, y) labelled (31 x + y) mod 2^13.  Every figure is the best and the median wall clock of `steps` synchronous calls from a RESIDENT source
(a LabelledGraph / ParsedGraph built before the clock starts) after `warmup`:
  transpose / union_with_transpose (KEEP_FIRST) / symmetrize / filter_lower_bound (4096: half the arcs) / store_labels_fixed13 / store_labels_gamma
  unlabelled_union_with_transpose   W.union of the underlying graph and its transpose: the per-node kernel the labelled union is measured against
Then a star: `--star` nodes that all point at node 0, united with its transpose (one row of that many arcs), both ways.
The "model" column is NOT the reference: there is no JVM here.  It is the numpy restatement the tests use, run once per figure in this script
on the same machine, and only on graphs of at most --model-max-nodes nodes.  store_labels' host figure is the CPU writer of the tooling.
Prints one line per figure and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CNR = os.path.join(ROOT, "tests", "golden", "cnr-2000")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-max-nodes", type=int, default=400000)
    ap.add_argument("--star", type=int, default=1000000)
    a = ap.parse_args()
    import numpy as np
    import webgraph_big_amd as W
    import labelled_model as LM
    import tooling as T
    out = {"warmup": a.warmup, "steps": a.steps, "copies": a.copies}

    def timed(call):
        ts = []
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            r = call()
            ts.append(time.perf_counter() - t0)
            if hasattr(r, "close"):
                r.close()
        ts = ts[a.warmup:]
        return min(ts), statistics.median(ts)

    def once(call):
        t0 = time.perf_counter()
        call()
        return time.perf_counter() - t0

    def bench(name, off, adj, lab, with_model, rows_wanted=None):
        n, m = len(off) - 1, len(adj)
        g = W.LabelledGraph.from_csr(off, adj, lab, W.LABEL_FIXED_INT, 13)
        gg = W.LabelledGraph.from_csr(off, adj, lab, W.LABEL_GAMMA_INT)
        t = W.transpose_labelled(g)
        u, ut = g.underlying(), t.underlying()
        model = LM.make(off, adj, lab) if with_model else None
        tmodel = LM.transpose(model) if with_model else None
        rows = {}

        def row(key, dev, host=None):
            if rows_wanted is not None and key not in rows_wanted:
                return
            best, med = timed(dev)
            rows[key] = dict(best_ms=best * 1e3, median_ms=med * 1e3, arcs_per_s=m / best)
            if host is not None and model is not None:
                rows[key]["model_ms"] = once(host) * 1e3
            print("%s %s: %s" % (name, key, json.dumps(rows[key])), flush=True)

        row("transpose", lambda: W.transpose_labelled(g), lambda: LM.transpose(model))
        row("union_with_transpose", lambda: W.union_labelled(g, t), lambda: LM.union(model, tmodel))
        row("union_transpose_first", lambda: W.union_labelled(t, g), lambda: LM.union(tmodel, model))
        row("unlabelled_union_with_transpose", lambda: W.union(u, ut))
        row("unlabelled_union_transpose_first", lambda: W.union(ut, u))
        row("symmetrize", lambda: W.symmetrize_labelled(g), lambda: LM.symmetrize(model))
        row("filter_lower_bound", lambda: W.filter_labelled_arcs(g, "LOWER_BOUND", lower_bound=4096), lambda: LM.filter(model, LM.LOWER_BOUND, lower_bound=4096))
        row("store_labels_fixed13", lambda: g.store_labels(), lambda: T.store_labels(W.LABEL_FIXED_INT, 13, lab, off))
        row("store_labels_gamma", lambda: gg.store_labels(), lambda: T.store_labels(W.LABEL_GAMMA_INT, 0, lab, off))
        if "union_with_transpose" in rows and "unlabelled_union_with_transpose" in rows:
            ratio = rows["union_with_transpose"]["best_ms"] / rows["unlabelled_union_with_transpose"]["best_ms"]
            print("%s labelled arc-parallel union / unlabelled per-node union: %.3f" % (name, ratio), flush=True)
            rows["labelled_over_unlabelled_union"] = ratio
        out[name] = dict(nodes=n, arcs=m, rows=rows)
        for h in (g, gg, t, u, ut):
            h.close()

    def labels_of(off, adj):
        src = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
        return ((31 * src + adj) % (1 << 13)).astype(np.int32)

    base = W.BVGraph.load(CNR)
    for name, bv in (("cnr-2000", base), ("cnr-2000 x %d" % a.copies, base.tile(a.copies))):
        with W.identity_graph(bv) as ig:
            off, adj = ig.csr()
        bench(name, off, adj, labels_of(off, adj), not a.no_model and len(off) - 1 <= a.model_max_nodes)
        if bv is not base:
            bv.close()
    base.close()
    if a.star > 1:
        n = a.star
        off = np.concatenate([[0, 0], np.arange(1, n, dtype=np.uint64)]).astype(np.uint64)           # node 0 has no arcs, nodes 1 .. n - 1 point at node 0
        adj = np.zeros(n - 1, dtype=np.int64)
        bench("star of %d" % n, off, adj, labels_of(off, adj), not a.no_model,
              rows_wanted=("transpose", "union_with_transpose", "union_transpose_first", "unlabelled_union_with_transpose", "unlabelled_union_transpose_first", "symmetrize"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
