"""Scattered arc list rates (reported, not gated): a text of 2^24 arcs (argument 1: log2 of the arcs, default 24) over 2^21 identifiers,
parsed from DEVICE memory (no upload in the figures), best of three after one warm-up:
  (a) identifiers 0 .. n - 1 in order of appearance -- the one text that parse_arc_list reads as well: the YARDSTICK is parse_arc_list on
      the same bytes in the same run (the existing parser, which ends in the same pairs_to_csr);
  (b) random 62-bit identifiers;
  (c) as (b), one hub identifier as the source of a quarter of the lines.
Argument 2, a subset of "abc", selects the cases.  With BVG_DEBUG=1 in the environment the library prints the wall clock of every stage of
the scattered parser on stderr (the device is drained between stages, so their sum is a little above the plain figure)."""
import ctypes as C
import sys
import time

sys.path.insert(0, '.')
import numpy as np
import webgraph_big_amd as W

log_arcs = int(sys.argv[1]) if len(sys.argv) > 1 else 24
cases = sys.argv[2] if len(sys.argv) > 2 else "abc"
arcs, n = 1 << log_arcs, 1 << max(log_arcs - 3, 1)
rng = np.random.default_rng(24)

hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]


def text_of(s, t):
    out = []
    for lo in range(0, len(s), 1 << 20):
        out.append(b"".join(b"%d\t%d\n" % p for p in zip(s[lo:lo + (1 << 20)].tolist(), t[lo:lo + (1 << 20)].tolist())))
    return b"".join(out)


def best(f, reps=3):
    f()                                                                             # warm-up: code objects, rocPRIM's choices
    dt = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); f(); dt = min(dt, time.perf_counter() - t0)        # (every entry point returns with the device drained)
    return dt


def run(name, s, t, yardstick=False):
    text = text_of(s, t)
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), len(text)) == 0 and hip.hipMemcpy(p, text, len(text), 1) == 0
    try:
        with W.parse_scattered_arcs_dev(p.value, len(text)) as g:
            shape = "%d nodes, %d arcs" % (g.num_nodes(), g.num_arcs())
        print("[bvg] case %s" % name, file=sys.stderr, flush=True)
        dt = best(lambda: W.parse_scattered_arcs_dev(p.value, len(text)).close())
        print("%-44s %7.1f MB %8.2f ms %6.2f GB/s %7.1f M arcs/s   (%s)" % (name, len(text) / 1e6, dt * 1e3, len(text) / dt / 1e9, arcs / dt / 1e6, shape), flush=True)
        if yardstick:
            dy = best(lambda: W.parse_arc_list_dev(p.value, len(text)).close())
            print("%-44s %7.1f MB %8.2f ms %6.2f GB/s %7.1f M arcs/s   (scattered / yardstick = %.2f)" % ("    yardstick: parse_arc_list, same text", len(text) / 1e6, dy * 1e3,
                                                                                                        len(text) / dy / 1e9, arcs / dy / 1e6, dt / dy), flush=True)
    finally:
        hip.hipFree(p)


k = np.arange(arcs, dtype=np.int64)
if "a" in cases:
    s = k // (arcs // n)                                                            # node x first appears as the source of its first line ...
    t = rng.integers(0, 1 << 62, arcs, dtype=np.int64) % (s + 1)                    # ... and every target has appeared before
    run("(a) identifiers 0..n-1 in order of appearance", s, t, yardstick=True)
pool = np.unique(rng.integers(0, 1 << 62, n + n // 8, dtype=np.int64))[:n]
pool = pool[rng.permutation(len(pool))]
s, t = pool[rng.integers(0, len(pool), arcs)], pool[rng.integers(0, len(pool), arcs)]
if "b" in cases:
    run("(b) random 62-bit identifiers", s, t)
if "c" in cases:
    s = s.copy(); s[rng.random(arcs) < 0.25] = pool[0]
    run("(c) as (b), one hub on a quarter of the lines", s, t)
