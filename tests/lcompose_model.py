"""A dictionary restatement, in Python ints, of the labelled graph product (include/bvgraph_hip.h, "Labelled compose"; Transform.java:1846-1856):
what tests/test_gpu_lcompose*.py hold the device against.  A labelled graph is (off int64[n + 1], adj int64[m], lab int64[m]).  Row x of
compose(a, b, semiring) has a successor z for every pair x -> y in a, y -> z in b with y < nb, and on (x, z) the semiring's sum of
label_a(x, y) (x) label_b(y, z) over those y.  The arithmetic is exact; the range rule on top: a label outside the result's class refuses the
call, and the refusal names how many arcs were out of range and the smallest (row, successor) among them."""
import numpy as np

GAMMA, FIXED = 1, 2
MIN_PLUS, MAX_PLUS, MAX_MIN, MIN_MAX, PLUS_TIMES = 0, 1, 2, 3, 4
NAMES = {"MIN_PLUS": MIN_PLUS, "MAX_PLUS": MAX_PLUS, "MAX_MIN": MAX_MIN, "MIN_MAX": MIN_MAX, "PLUS_TIMES": PLUS_TIMES}
SEMIRINGS = sorted(NAMES.values())

_ADD = {MIN_PLUS: min, MAX_PLUS: max, MAX_MIN: max, MIN_MAX: min, PLUS_TIMES: lambda u, v: u + v}
_MUL = {MIN_PLUS: lambda u, v: u + v, MAX_PLUS: lambda u, v: u + v, MAX_MIN: min, MIN_MAX: max, PLUS_TIMES: lambda u, v: u * v}


def make(off, adj, lab):
    return np.asarray(off).astype(np.int64), np.asarray(adj).astype(np.int64), np.asarray(lab).astype(np.int64)


def from_rows(rows, n=None):
    """rows[x] = [(successor, label), ...] in any order -> a labelled graph of n >= len(rows) nodes."""
    n = len(rows) if n is None else n
    rows = [sorted(r) for r in rows] + [[] for _ in range(n - len(rows))]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]) if n else np.zeros(1)
    flat = [p for r in rows for p in r]
    return make(off, [p[0] for p in flat], [p[1] for p in flat])


def rows_of(g):
    off, adj, lab = g
    return [[(int(adj[i]), int(lab[i])) for i in range(int(off[x]), int(off[x + 1]))] for x in range(len(off) - 1)]


def compose_rows(a, b, semiring):
    """The product as rows of (successor, label) with labels as Python ints: no range rule."""
    add, mul = _ADD[semiring], _MUL[semiring]
    (off0, adj0, lab0), (off1, adj1, lab1) = a, b
    off0, adj0, lab0, off1, adj1, lab1 = (v.tolist() for v in (off0, adj0, lab0, off1, adj1, lab1))
    n0, n1 = len(off0) - 1, len(off1) - 1
    out = []
    for x in range(max(n0, n1)):
        acc = {}
        if x < n0:
            for i in range(off0[x], off0[x + 1]):
                y = adj0[i]
                if y >= n1:
                    continue                                                   # a successor b does not have contributes nothing
                u = lab0[i]
                for j in range(off1[y], off1[y + 1]):
                    z, p = adj1[j], mul(u, lab1[j])
                    acc[z] = add(acc[z], p) if z in acc else p
        out.append(sorted(acc.items()))
    return out


def class_max(kind, width):
    return (1 << 31) - 1 if kind == GAMMA else (1 << width) - 1


def out_of_range(rows, kind, width):
    """(count, (row, successor) of the smallest) of the labels outside [0, class_max]; (0, None) when every label is in range."""
    hi = class_max(kind, width)
    bad = [(x, z) for x, r in enumerate(rows) for z, v in r if not 0 <= v <= hi]
    return len(bad), (min(bad) if bad else None)


def compose(a, b, semiring, kind=GAMMA, width=0):
    """("ok", graph) or ("range", count, first arc): the whole call, with `width` the result's."""
    rows = compose_rows(a, b, semiring)
    count, first = out_of_range(rows, kind, width)
    if count:
        return "range", count, first
    return "ok", from_rows(rows)


def underlying(g):
    return g[0], g[1]
