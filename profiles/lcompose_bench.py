"""The labelled graph product on the device (bvg_lcompose) beside the unlabelled one (bvg_compose) on the underlying graphs.

  python profiles/lcompose_bench.py [--warmup 1] [--steps 5] [--parent-lib PATH] [--out profiles/lcompose_bench.txt]

Every figure is the best and the median wall clock of `steps` synchronous calls after `warmup`, from graphs that are resident on the device, the
result left on the device.  The labels are (31 x + y) mod 97 on arc (x, y), GammaCodedIntLabel:
  cnr o cnr          cnr-2000 with itself: 96 M products, 34 M arcs            under (min, +) and (+, x)
  cnr^T o cnr        g0 = the labelled transpose: 169 M products (tier 2)      under (min, +) and (+, x)
and cnr o cnr under (min, +) with every row forced up one tier (BVG_COMPOSE_TIER=1, =2).  A call whose labels leave the class is refused after
all of its work is done; it is timed all the same and the line says so.
THE YARDSTICK is bvg_compose on the underlying graphs, same shapes and forced tiers, in the same run on the same box: the labelled call does
the same inserts plus one atomic per product and twice the table bytes.  --parent-lib names a build of the library from the parent commit
(BVG_HIP_LIB); the unlabelled figures are then taken in a child process that loads it.  Without it they come from the library in the tree,
whose bvg_compose kernels are the parent's.  Prints one line per figure with both columns and the ratio, then each library's own split of one further call into
stages (BVG_DEBUG=1), and writes them, with one JSON line, to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CNR = os.path.join(ROOT, "tests", "golden", "cnr-2000")
os.environ.setdefault("BVG_TEST_KNOBS", "1")                                   # the forced tiers are test knobs, read at each call

SHAPES = [("cnr o cnr", False, None), ("cnr o cnr, every row in tier 1 or above", False, 1), ("cnr o cnr, every row in tier 2", False, 2),
          ("cnr^T o cnr", True, None)]


def timed(call, warmup, steps, tier):
    if tier is None:
        os.environ.pop("BVG_COMPOSE_TIER", None)
    else:
        os.environ["BVG_COMPOSE_TIER"] = str(tier)
    ts, rep = [], None
    for _ in range(warmup + steps):
        t0 = time.perf_counter()
        rep = call()
        ts.append(time.perf_counter() - t0)
    os.environ.pop("BVG_COMPOSE_TIER", None)
    ts = ts[warmup:]
    return dict(best_ms=min(ts) * 1e3, median_ms=statistics.median(ts) * 1e3, **rep)


def stages(call, tag):
    """The library's own split of one call, which it prints to stderr under BVG_DEBUG."""
    import tempfile
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["BVG_DEBUG"] = "1"
        try:
            call()
        finally:
            del os.environ["BVG_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        found = [l.split(tag, 1)[1] for l in tmp.read().decode(errors="replace").splitlines() if tag in l]
    return found[-1] if found else "(nothing printed)"


def unlabelled(warmup, steps):
    """bvg_compose over the shapes, with whatever library this process loads: {shape: figures}."""
    import webgraph_big_amd as W
    base = W.BVGraph.load(CNR)
    g = W.identity_graph(base)
    t = W.transpose_graph(g)
    out = {}

    def call(g0, g1):
        r, rep = W.compose(g0, g1, report=True)
        r.close()
        return rep

    for name, transposed, tier in SHAPES:
        out[name] = timed(lambda: call(t if transposed else g, g), warmup, steps, tier)
        if tier is not None:
            os.environ["BVG_COMPOSE_TIER"] = str(tier)
        out[name]["stages"] = stages(lambda: call(t if transposed else g, g), "[bvg] compose: ")
        os.environ.pop("BVG_COMPOSE_TIER", None)
    for h in (t, g, base):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--unlabelled-only", action="store_true", help="(the child process of --parent-lib) print the unlabelled figures as JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lcompose_bench.txt"))
    a = ap.parse_args()
    if a.unlabelled_only:
        print("UNLABELLED " + json.dumps(unlabelled(a.warmup, a.steps)))
        return
    import numpy as np
    import webgraph_big_amd as W
    lines, out = [], {"warmup": a.warmup, "steps": a.steps, "parent_lib": a.parent_lib and os.path.basename(a.parent_lib)}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if a.parent_lib:
        env = dict(os.environ, BVG_HIP_LIB=os.path.abspath(a.parent_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--unlabelled-only", "--warmup", str(a.warmup), "--steps", str(a.steps)],
                           env=env, capture_output=True, text=True, check=True)
        yard = json.loads([l for l in p.stdout.splitlines() if l.startswith("UNLABELLED ")][-1].split(" ", 1)[1])
        say("yardstick: bvg_compose of a build of the parent commit (%s, loaded by a child process)" % os.path.basename(a.parent_lib))
    else:
        yard = unlabelled(a.warmup, a.steps)
        say("yardstick: bvg_compose of the library in the tree")

    base = W.BVGraph.load(CNR)
    with W.identity_graph(base) as u:
        off, adj = u.csr()
    src = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off.astype(np.int64)))
    g = W.LabelledGraph.from_csr(off, adj, (src * 31 + adj) % 97, W.LABEL_GAMMA_INT)
    t = W.transpose_labelled(g)

    def call(g0, g1, semiring):
        try:
            r, rep = W.compose_labelled(g0, g1, semiring, report=True)
            r.close()
            return dict(rep, refused=False)
        except W.IllegalArgumentException as e:
            return dict(e.report, refused=True)

    for name, transposed, tier in SHAPES:
        for semiring in (("MIN_PLUS", "PLUS_TIMES") if tier is None else ("MIN_PLUS",)):
            res = timed(lambda: call(t if transposed else g, g, semiring), a.warmup, a.steps, tier)
            y = yard[name]
            res.update(unlabelled_best_ms=y["best_ms"], unlabelled_median_ms=y["median_ms"], unlabelled_rows=y["rows"], ratio=res["best_ms"] / y["best_ms"],
                       products_per_s=res["products"] / (res["best_ms"] / 1e3))
            if tier is not None:
                os.environ["BVG_COMPOSE_TIER"] = str(tier)
            res["stages"] = stages(lambda: call(t if transposed else g, g, semiring), "[bvg] lcompose: ")
            os.environ.pop("BVG_COMPOSE_TIER", None)
            out["%s, %s" % (name, semiring)] = res
            say("%s, %s: labelled %.2f ms (median %.2f), unlabelled %.2f ms (median %.2f), ratio %.2f; rows %r against %r%s" % (
                name, semiring, res["best_ms"], res["median_ms"], y["best_ms"], y["median_ms"], res["ratio"], res["rows"], y["rows"],
                "; REFUSED for %d labels out of range, after all of its work" % res["out_of_range"] if res["refused"] else ""))
            say("    one more call each with BVG_DEBUG=1 (a synchronisation after every stage): labelled: %s" % res["stages"])
            say("    unlabelled: %s" % y["stages"])
    for h in (t, g, base):
        h.close()
    lines.append(json.dumps(out))
    print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
