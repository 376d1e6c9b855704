"""Test helper of tests/test_geometric_model.py, tests/test_gpu_geometric.py and tests/test_gpu_geometric_cpp.py: the CPU side of the exact
geometric centralities (bvg_geometric; algo/LinearGeometricCentrality.java), in numpy (scipy is not needed).

  distance_counts(off, adj, sources)        N_d(s): per source the number of nodes at distance d = 0, 1, ... (one breadth-first visit each)
  distance_counts_pull(off, adj, sources)   the same numbers for many sources at once: 64 sources per word, every level one OR-reduction over the
                                            arcs sorted by target (the transposed graph) -- not how the device does it (it pushes along forward arcs)
  coefficient(spec)                         d -> coeff(d) in double, for "harmonic", ("power", e), ("exp", b) or a table
  exact(counts, coeff)                      sum_d coeff(d) N_d by math.fsum, rounded to np.float32 once
  reference_order(off, adj, s, coeff)       the reference's own visit restated: a FIFO queue, successors in increasing order, coeff added to a
                                            float32 once per discovered node ((float)(centrality + coeff): the sum in double, rounded to float),
                                            coeff(0) added last; returns (centrality float32, reachable)
"""
import math

import numpy as np


def coefficient(spec):
    if isinstance(spec, str):
        assert spec == "harmonic", spec
        return lambda d: 0.0 if d == 0 else 1.0 / d
    if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str):
        kind, x = spec[0], float(spec[1])
        assert kind in ("power", "exp"), spec
        return (lambda d: _pow(float(d), x)) if kind == "power" else (lambda d: _pow(x, float(d)))
    table = [float(v) for v in spec]
    return lambda d: table[d] if d < len(table) else 0.0


def _pow(x, y):
    """C's pow / Java's Math.pow: math.pow raises where they return infinity."""
    try:
        return math.pow(x, y)
    except ValueError:                                                         # 0 to a negative power
        assert x == 0 and y < 0, (x, y)
        return math.inf
    except OverflowError:
        return math.inf


def _lists(off, adj):
    off = np.asarray(off, dtype=np.int64); adj = np.asarray(adj, dtype=np.int64)
    return off, adj


def distance_counts(off, adj, sources):
    """[N(s) for s in sources], N(s) an int64 array with N(s)[d] = the nodes at distance d from s (N(s)[0] == 1)."""
    off, adj = _lists(off, adj)
    n = len(off) - 1
    out = []
    for s in sources:
        seen = np.zeros(n, dtype=bool); seen[s] = True
        frontier = np.array([s], dtype=np.int64)
        counts = [1]
        while True:
            lo, hi = off[frontier], off[frontier + 1]
            total = int((hi - lo).sum())
            if total == 0:
                break
            # the successors of the frontier: positions lo[i] .. hi[i] of adj, for every i
            idx = np.repeat(lo - np.concatenate(([0], np.cumsum(hi - lo)[:-1])), hi - lo) + np.arange(total, dtype=np.int64)
            y = np.unique(adj[idx])
            y = y[~seen[y]]
            if len(y) == 0:
                break
            seen[y] = True
            counts.append(len(y))
            frontier = y
        out.append(np.array(counts, dtype=np.int64))
    return out


def distance_counts_pull(off, adj, sources):
    """distance_counts for many sources at once (same return value)."""
    off, adj = _lists(off, adj)
    n = len(off) - 1
    sources = np.asarray(list(sources), dtype=np.int64)
    S = len(sources)
    if S == 0:
        return []
    words = (S + 63) // 64
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    order = np.argsort(adj, kind="stable")
    t_src, t_dst = src[order], adj[order]                                       # the arcs by target
    seen = np.zeros((n, words), dtype=np.uint64)
    j = np.arange(S)
    np.bitwise_or.at(seen, (sources, j // 64), np.uint64(1) << (j % 64).astype(np.uint64))   # (a node may be listed twice)
    frontier = seen.copy()
    levels = [np.ones(S, dtype=np.int64)]
    while True:
        live = np.flatnonzero(frontier.any(axis=1)[t_src])                     # arcs that leave a frontier node, still by target
        if len(live) == 0:
            break
        d = t_dst[live]
        starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
        targets = d[starts]
        reached = np.bitwise_or.reduceat(frontier[t_src[live]], starts, axis=0)
        new = np.zeros_like(seen)
        new[targets] = reached & ~seen[targets]
        rows = np.flatnonzero(new.any(axis=1))
        if len(rows) == 0:
            break
        seen |= new
        frontier = new
        bits = np.unpackbits(new[rows].view(np.uint8).reshape(len(rows), words * 8), axis=1, bitorder="little")   # bit j of word k: column 64 k + j
        levels.append(bits.sum(axis=0, dtype=np.int64)[:S])
    table = np.stack(levels, axis=1)                                           # [source, distance]
    return [row[:int(np.flatnonzero(row)[-1]) + 1] for row in table]


def histogram(counts):
    """The pairs (source, node) at every distance, over all the sources: what bvg_geometric returns as hist."""
    if not counts:
        return np.zeros(0, dtype=np.uint64)
    h = np.zeros(max(len(c) for c in counts), dtype=np.uint64)
    for c in counts:
        h[:len(c)] += c.astype(np.uint64)
    return h


def reachable(counts):
    return np.array([int(c.sum()) for c in counts], dtype=np.int64)


def exact(counts, coeff):
    """np.float32 per source: sum_d coeff(d) N_d(s), summed without intermediate rounding (math.fsum), rounded to float once."""
    out = np.empty(len(counts), dtype=np.float32)
    with np.errstate(over="ignore"):
        for i, c in enumerate(counts):
            terms = [coeff(d) * int(k) for d, k in enumerate(c) if k]
            out[i] = np.float32(math.inf if any(math.isinf(t) for t in terms) else math.fsum(terms))
    return out


def exact_double(counts, coeff):
    """The same sums, not rounded to float (the `value` of the bound on the reference's accumulated float error)."""
    return np.array([math.inf if any(math.isinf(coeff(d)) for d, k in enumerate(c) if k) else math.fsum(coeff(d) * int(k) for d, k in enumerate(c) if k)
                     for c in counts], dtype=np.float64)


def reference_order(off, adj, s, coeff):
    """(centrality float32, reachable) of source s as LinearGeometricCentrality.IterationThread computes them."""
    off, adj = _lists(off, adj)
    n = len(off) - 1
    dist = [-1] * n
    dist[s] = 0
    queue, head, reach = [int(s)], 0, 0
    c = np.float32(0)
    with np.errstate(over="ignore"):
        while head < len(queue):
            x = queue[head]; head += 1
            reach += 1
            d = dist[x] + 1
            k = coeff(d)
            for y in sorted(int(v) for v in adj[off[x]:off[x + 1]]):
                if dist[y] == -1:
                    queue.append(y)
                    dist[y] = d
                    c = np.float32(float(c) + k)
        c = np.float32(float(c) + coeff(0))
    return c, reach


def within_one_spacing(got, expected):
    """|got - expected| <= the float32 spacing at expected, element by element; infinities must be equal."""
    got = np.asarray(got, dtype=np.float32); expected = np.asarray(expected, dtype=np.float32)
    inf = np.isinf(expected)
    if not np.array_equal(got[inf], expected[inf]):
        return False
    g, e = got[~inf].astype(np.float64), expected[~inf]
    return bool(np.all(np.abs(g - e.astype(np.float64)) <= np.spacing(np.abs(e)).astype(np.float64)))


def csr_of(n, arcs):
    """(off uint64[n + 1], adj int64) of a list of (u, v) pairs, lists sorted and without duplicates."""
    arcs = sorted(set((int(u), int(v)) for u, v in arcs))
    src = np.array([a[0] for a in arcs], dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum(np.bincount(src, minlength=n)).astype(np.uint64)
    return off, np.array([a[1] for a in arcs], dtype=np.int64)


def _cycle(lo, hi):
    return [(x, x + 1) for x in range(lo, hi - 1)] + [(hi - 1, lo)]


# the hand graphs of the GPU tests: name -> (nodes, arcs)
HAND = {
    "one_node": (1, []),
    "one_self_loop": (1, [(0, 0)]),
    "two_cycle_and_sink": (3, [(0, 1), (1, 0), (1, 2)]),
    "star": (9, [(0, x) for x in range(1, 9)] + [(3, 0)]),                     # the centre reaches every leaf, leaf 3 the centre
    "two_disjoint_cycles": (11, _cycle(0, 5) + _cycle(5, 11)),
    "path_70": (70, [(x, x + 1) for x in range(69)]),                          # 69 levels; the sources cross a word boundary
    "cycle_130": (130, _cycle(0, 130)),
}

# one of every kind of coefficients; ("power", -2): coeff(0) = +inf, so every value is
COEFFS = {
    "harmonic": "harmonic",
    "sum_of_distances": ("power", 1),
    "power_minus_2": ("power", -2),
    "exp_half": ("exp", 0.5),
    "exp_0.9": ("exp", 0.9),
    "table": [0.0, 1.0, 1.0, 3.0],
}
