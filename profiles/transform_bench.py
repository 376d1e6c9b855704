"""Transform on the device beside the same operations done by the model (tests/transform_model.py) on the host's cores.

  python profiles/transform_bench.py [--copies 16] [--warmup 1] [--steps 5] [--no-model]

Two graphs: cnr-2000 (the golden fixture: 325 557 nodes, 3.2 M arcs) and its device tiling (bvg_tile, `copies` back-to-back copies, every
list translated with its copy).  Every figure is the best and the median wall clock of `steps` synchronous calls after `warmup`:
  identity                the decode of the BVGraph into a resident CSR (every other call below starts from that CSR, so none pays it again)
  map                     map_graph by a random permutation (the pairs -> CSR stage: two radix sorts)
  filter / transpose / symmetrize / simplify / union (with the transpose)
  lex / gray / random     the permutation alone, perm copied to the host
  lex+map+store ...       permutation, map_graph by it, store() at the default parameters: the end-to-end path of Transform.main's lex / gray /
                          random, compressed bytes back in host memory; bits per arc of the result beside it
The "model" column is NOT the reference: there is no JVM here.  It is the numpy / Python restatement the tests use, run in this script on
the same machine (numpy's own threading is all the parallelism it has); it says what a straightforward host implementation costs, nothing
about WebGraph's.  The model runs once per figure, and only on graphs of at most --model-max-nodes nodes.
With BVG_DEBUG=1 in the environment the library prints the stages of every permutation to stderr (keys + radix sort, open runs, merge sort).
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
    a = ap.parse_args()
    import numpy as np
    import webgraph_big_amd as W
    import transform_model as M
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

    base = W.BVGraph.load(CNR)
    for name, bv in (("cnr-2000", base), ("cnr-2000 x %d" % a.copies, base.tile(a.copies))):
        g = W.identity_graph(bv)
        n, m = g.num_nodes(), g.num_arcs()
        model = None
        if not a.no_model and n <= a.model_max_nodes:
            off, adj = g.csr()
            model = (off.astype(np.int64), adj)
        rng = np.random.default_rng(1)
        perm = rng.permutation(n).astype(np.int64)
        cls = rng.integers(0, 4, size=n)
        tr = W.transpose_graph(g)
        tmodel = M.transpose(*model) if model else None
        rows = {}

        def row(key, dev, host=None, **extra):
            best, med = timed(dev)
            rows[key] = dict(best_ms=best * 1e3, median_ms=med * 1e3, arcs_per_s=m / best, **extra)
            if host is not None and model is not None:
                rows[key]["model_ms"] = once(host) * 1e3
            print("%s %s: %s" % (name, key, json.dumps(rows[key])), flush=True)

        row("identity", lambda: W.identity_graph(bv))
        row("map", lambda: W.map_graph(g, perm), lambda: M.map_graph(*model, perm))
        row("filter_no_loops", lambda: W.filter_arcs(g, "NO_LOOPS"), lambda: M.filter_arcs(*model, "NO_LOOPS"))
        row("filter_same_class", lambda: W.filter_arcs(g, "SAME_CLASS", cls), lambda: M.filter_arcs(*model, "SAME_CLASS", cls))
        row("transpose", lambda: W.transpose_graph(g), lambda: M.transpose(*model))
        row("symmetrize", lambda: W.symmetrize_graph(g), lambda: M.symmetrize(*model))
        row("simplify", lambda: W.simplify_graph(g), lambda: M.symmetrize(*model, drop_loops=True))
        row("union", lambda: W.union(g, tr), lambda: M.union(model, tmodel))
        row("lex", lambda: W.lexicographical_permutation(g), lambda: M.permutation_of_csr(*model, False))
        row("gray", lambda: W.gray_code_permutation(g), lambda: M.permutation_of_csr(*model, True))
        row("random", lambda: W.random_permutation(g, 7), lambda: M.random_permutation(n, 7))

        bits = {}

        def end_to_end(key, permutation):
            def call():
                with W.map_graph(g, permutation(g)) as mapped:
                    graph, offsets = mapped.store()
                    bits[key] = float(offsets[-1]) / max(mapped.num_arcs(), 1)
            return call
        graph, offsets = g.store()
        bits["as stored"] = float(offsets[-1]) / max(m, 1)
        for key, permutation in (("lex", W.lexicographical_permutation), ("gray", W.gray_code_permutation), ("random", lambda x: W.random_permutation(x, 7))):
            row(key + "+map+store", end_to_end(key, permutation))
            rows[key + "+map+store"]["bits_per_arc"] = bits[key]
        print("%s bits per arc at the default parameters: %s" % (name, json.dumps(bits)), flush=True)
        out[name] = dict(nodes=n, arcs=m, rows=rows, bits_per_arc=bits)
        tr.close(); g.close()
        if bv is not base:
            bv.close()
    base.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
