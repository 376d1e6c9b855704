"""Test helper of tests/test_stats_model.py and tests/test_gpu_stats.py: a plain restatement of Stats.run (Stats.java:96-257) over a CSR
(off uint64[n + 1], succ int64[arcs]).  The per-arc and per-node quantities are numpy one-liners; the sums are Python ints; the extremes
are found by the reference's own scans (outdegrees upwards, indegrees downwards, strict comparisons), so ties fall as they do there; the
text of .stats is formatted here on its own (decimal with a wide context, Java's Double.toString layout), not by the package."""
import decimal
import math

import numpy as np

INT64_MAX = (1 << 63) - 1


def _scan(values, order):
    """(min, min node, max, max node) as Stats.run finds them visiting the nodes in `order` with strict comparisons."""
    mind, minn, maxd, maxn = INT64_MAX, 0, 0, 0
    v = np.asarray(values, dtype=np.int64)
    if len(v):
        # the first node in visiting order that attains the extreme wins
        lo, hi = int(v.min()), int(v.max())
        pos_lo, pos_hi = np.flatnonzero(v == lo), np.flatnonzero(v == hi)
        mind, minn = lo, int(pos_lo[0] if order > 0 else pos_lo[-1])
        if hi > 0:
            maxd, maxn = hi, int(pos_hi[0] if order > 0 else pos_hi[-1])
    return mind, minn, maxd, maxn


def model(off, succ):
    off = np.asarray(off, dtype=np.int64); succ = np.asarray(succ, dtype=np.int64)
    n = len(off) - 1
    deg = np.diff(off)
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    dist = np.abs(succ - src)
    m = {"nodes": n, "arcs": int(len(succ)), "loops": int(np.count_nonzero(dist == 0)), "dangling": int(np.count_nonzero(deg == 0))}
    first = succ[off[:-1][deg > 0]]; last = succ[off[1:][deg > 0] - 1]; node = np.flatnonzero(deg > 0); d = deg[deg > 0]
    m["terminal"] = m["dangling"] + int(np.count_nonzero((d == 1) & (first == node)))
    many = d > 1
    m["num_gaps"] = int(d[many].sum())
    v = first[many] - node[many]
    nat = np.where(v >= 0, 2 * v, -2 * v - 1)                              # Fast.int2nat
    m["tot_gap"] = sum(int(a) for a in (last[many] - first[many])) + sum(int(a) for a in nat)
    m["tot_loc"] = sum(int(a) for a in dist)
    bins = [0] * 64
    nz = dist[dist != 0]
    if len(nz):
        msb = np.frompyfunc(lambda a: int(a).bit_length() - 1, 1, 1)(nz).astype(np.int64)
        for b, c in zip(*np.unique(msb, return_counts=True)):
            bins[int(b)] = int(c)
    m["log_delta"] = bins
    indeg = np.bincount(succ, minlength=n).astype(np.int64) if n else np.zeros(0, np.int64)
    m["indegrees"] = indeg
    m["min_outdegree"], m["min_outdegree_node"], m["max_outdegree"], m["max_outdegree_node"] = _scan(deg, +1)
    m["min_indegree"], m["min_indegree_node"], m["max_indegree"], m["max_indegree_node"] = _scan(indeg, -1)
    m["outdegree_distribution"] = np.bincount(deg, minlength=m["max_outdegree"] + 1).astype(np.uint64) if n else np.zeros(1, np.uint64)
    m["indegree_distribution"] = np.bincount(indeg, minlength=m["max_indegree"] + 1).astype(np.uint64) if n else np.zeros(1, np.uint64)
    return m


SCALARS = ("nodes", "arcs", "loops", "dangling", "terminal", "num_gaps", "tot_gap", "tot_loc", "min_outdegree", "max_outdegree", "min_outdegree_node",
           "max_outdegree_node", "min_indegree", "max_indegree", "min_indegree_node", "max_indegree_node")


def assert_same(got, m, indegrees=True, what=""):
    """A GraphStats of the package against the model's dict."""
    for k in SCALARS:
        assert getattr(got, k) == m[k], (what, k, getattr(got, k), m[k])
    assert list(got.log_delta) == m["log_delta"], what
    for k in ("outdegree_distribution", "indegree_distribution"):
        a = getattr(got, k)
        assert a.dtype == np.uint64 and np.array_equal(a, m[k]), (what, k, len(a), len(m[k]))
    if indegrees:
        assert got.indegrees.dtype == np.int64 and np.array_equal(got.indegrees, m["indegrees"]), what


def java_double(x):
    if x != x:
        return "NaN"
    if x == 0:
        return "0.0"
    mant, _, e = ("%r" % float(x)).partition("e")                          # the shortest digits; then Java's layout
    d = decimal.Decimal(mant).scaleb(int(e or 0))
    digits = "".join(map(str, d.as_tuple().digits)).rstrip("0") or "0"
    e10 = d.adjusted()
    if 1e-3 <= abs(x) < 1e7:
        t = format(d, "f")
        return t if "." in t else t + ".0"
    return "%s.%sE%d" % (digits[0], digits[1:] or "0", e10)


def _div3(num, den):
    with decimal.localcontext() as c:
        c.prec = 2400                                                       # (an exact double has up to ~1075 digits: the quotient is cut far beyond them)
        return str((decimal.Decimal(num) / decimal.Decimal(den)).quantize(decimal.Decimal("0.001"), rounding=decimal.ROUND_HALF_EVEN))


def properties(m, buckets=None, scc_sizes=None):
    n = m["nodes"]
    fdiv = lambda a, b: a / b if b else float("nan")
    lines = ["nodes=%d" % n, "arcs=%d" % m["arcs"], "loops=%d" % m["loops"], "successoravggap=" + _div3(m["tot_gap"], max(1, m["num_gaps"])),
             "avglocality=" + _div3(m["tot_loc"], max(1, m["arcs"])), "minoutdegree=%d" % m["min_outdegree"], "maxoutdegree=%d" % m["max_outdegree"],
             "minoutdegreenode=%d" % m["min_outdegree_node"], "maxoutdegreenode=%d" % m["max_outdegree_node"], "dangling=%d" % m["dangling"],
             "terminal=%d" % m["terminal"], "percdangling=" + java_double(fdiv(100.0 * m["dangling"], n)), "avgoutdegree=" + java_double(fdiv(float(m["arcs"]), n))]
    bins = m["log_delta"]
    l = max([i for i in range(64) if bins[i]], default=-1)
    tot, num, g = 0.0, 0, 1
    for i in range(l + 1):
        num += bins[i]
        tot += (math.log(g * 2 + g + 1) / math.log(2) - 1) * bins[i]
        g *= 2
    lines += ["successorlogdeltastats=" + ",".join(map(str, bins[:l + 1])), "successoravglogdelta=" + ("0" if num == 0 else _div3(tot, max(1, num * 2)))]
    lines += ["minindegree=%d" % m["min_indegree"], "maxindegree=%d" % m["max_indegree"], "minindegreenode=%d" % m["min_indegree_node"],
              "maxindegreenode=%d" % m["max_indegree_node"], "avgindegree=" + java_double(fdiv(float(m["arcs"]), n))]
    if buckets is not None:
        lines += ["buckets=%d" % buckets, "percbuckets=" + java_double(fdiv(100.0 * buckets, n))]
    if scc_sizes is not None:
        s = sorted(int(v) for v in scc_sizes)
        lines += ["sccs=%d" % len(s), "maxsccsize=%d" % s[-1], "percmaxscc=" + java_double(fdiv(100.0 * s[-1], n)), "minsccsize=%d" % s[0],
                  "percminscc=" + java_double(fdiv(100.0 * s[0], n))]
    return "".join(x + "\n" for x in lines)


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if len(lists):
        off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    succ = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) and off[-1] else np.zeros(0, np.int64)
    return off, succ
