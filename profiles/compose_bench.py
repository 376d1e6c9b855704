"""The graph product on the device (bvg_compose) beside the numpy model (tests/compose_model.py) on the host's cores.

  python profiles/compose_bench.py [--copies 16] [--warmup 1] [--steps 5] [--no-model] [--out profiles/compose_bench.txt]

Every figure is the best and the median wall clock of `steps` synchronous calls after `warmup`, from CSRs that are resident on the device
(the decode of the BVGraph is paid before the clock starts), the result left on the device:
  cnr o cnr          cnr-2000 with itself: 96 M products, 34 M arcs
  cnr^T o cnr        g0 = the transpose: 169 M products (rows of up to several hundred thousand products: tier 2)
  cnr o cnr x N      the device tiling (bvg_tile, `copies` back-to-back copies) with itself
and, for cnr o cnr, the same call with every row forced up one tier (BVG_COMPOSE_TIER=1, =2): what the LDS table of a wavefront is worth
against a workgroup's, and both against tables in HBM with the in-place sort.  Beside each figure the split the call reports: products,
arcs, rows per tier, batches; and the library's own split of one further call into stages (BVG_DEBUG=1).
The "model" column is NOT the reference: there is no JVM here.  It is a constructed baseline, the numpy restatement the tests use (expand
every product, np.unique per chunk of rows), run once in this script on the same machine's granted cores.
Prints one line per figure and writes them, with one JSON line, to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CNR = os.path.join(ROOT, "tests", "golden", "cnr-2000")
os.environ.setdefault("BVG_TEST_KNOBS", "1")                                   # the forced tiers are test knobs, read at each call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import webgraph_big_amd as W
    import compose_model as CM
    lines, out = [], {"warmup": a.warmup, "steps": a.steps, "copies": a.copies, "threads": os.environ.get("OMP_NUM_THREADS")}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def stages(g0, g1):
        """The library's own split of one call, which it prints to stderr under BVG_DEBUG."""
        import tempfile
        with tempfile.TemporaryFile() as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            os.environ["BVG_DEBUG"] = "1"
            try:
                W.compose(g0, g1).close()
            finally:
                del os.environ["BVG_DEBUG"]
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            found = [l.split("compose: ", 1)[1] for l in tmp.read().decode(errors="replace").splitlines() if "[bvg] compose: " in l]
        return found[-1] if found else "(nothing printed)"

    def row(key, g0, g1, tier=None, model=None):
        if tier is None:
            os.environ.pop("BVG_COMPOSE_TIER", None)
        else:
            os.environ["BVG_COMPOSE_TIER"] = str(tier)
        ts, rep = [], None
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            r, rep = W.compose(g0, g1, report=True)
            ts.append(time.perf_counter() - t0)
            r.close()
        res_stages = stages(g0, g1)
        os.environ.pop("BVG_COMPOSE_TIER", None)
        ts = ts[a.warmup:]
        best = min(ts)
        res = dict(best_ms=best * 1e3, median_ms=statistics.median(ts) * 1e3, products_per_s=rep["products"] / best, arcs_per_s=rep["arcs"] / best, **rep)
        if model is not None:
            t0 = time.perf_counter()
            CM.compose(*model)
            res["model_ms"] = (time.perf_counter() - t0) * 1e3
        out[key] = res
        say("%s: %s" % (key, json.dumps(res)))
        say("    one more call with BVG_DEBUG=1 (a synchronisation after every stage): " + res_stages)

    base = W.BVGraph.load(CNR)
    g = W.identity_graph(base)
    t = W.transpose_graph(g)
    model = None
    if not a.no_model:
        off, adj = g.csr()
        model = ((off.astype(np.int64), adj),) * 2
    row("cnr o cnr", g, g, model=model)
    row("cnr o cnr, every row in tier 1 or above", g, g, tier=1)
    row("cnr o cnr, every row in tier 2", g, g, tier=2)
    row("cnr^T o cnr", t, g)
    tiled = base.tile(a.copies)
    big = W.identity_graph(tiled)
    row("cnr o cnr x %d" % a.copies, big, big)
    for h in (big, tiled, t, g, base):
        h.close()
    lines.append(json.dumps(out))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
