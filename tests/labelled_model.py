"""The yardstick of the labelled transforms (tests only): Transform's labelled half restated in numpy over CSR triples
(adj_off uint64[n + 1], adj int64[m], labels int32[m]), with converters to and from {(x, y): label} dictionaries.  Written from the behaviour
of Transform.java (transposeOffline on labelled graphs :1337-1631, union :633-635 with UnionArcLabelledImmutableGraph.java:188, filterArcs with
LowerBound :197-215), not from its text.  The label STREAM has no model here: its yardstick is the CPU writer tooling.store_labels."""
import numpy as np

KEEP_FIRST, MIN, MAX = "KEEP_FIRST", "MIN", "MAX"
NO_LOOPS, SAME_CLASS, DIFFERENT_CLASS, LOWER_BOUND = "NO_LOOPS", "SAME_CLASS", "DIFFERENT_CLASS", "LOWER_BOUND"
MERGE = {KEEP_FIRST: lambda a, b: a, MIN: np.minimum, MAX: np.maximum}


def make(off, adj, lab):
    return np.asarray(off, dtype=np.uint64), np.asarray(adj, dtype=np.int64), np.asarray(lab, dtype=np.int32)


def nodes(g):
    return len(g[0]) - 1


def sources(g):
    return np.repeat(np.arange(nodes(g), dtype=np.int64), np.diff(g[0].astype(np.int64)))


def from_arcs(n, src, dst, lab):
    """The CSR of the arcs (src[i], dst[i]) with labels lab[i]; the pairs must be distinct."""
    src, dst, lab = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(lab, dtype=np.int32)
    order = np.lexsort((dst, src))
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]) if n else np.zeros(1)
    return make(off, dst[order], lab[order])


def from_dict(n, d):
    keys = sorted(d)
    return from_arcs(n, [k[0] for k in keys], [k[1] for k in keys], [d[k] for k in keys])


def to_dict(g):
    return {(int(x), int(y)): int(l) for x, y, l in zip(sources(g), g[1], g[2])}


def from_csr(off, adj, lab):
    return make(off, adj, lab)


def csr(g):
    return g


def transpose(g):
    return from_arcs(nodes(g), g[1], sources(g), g[2])


def pad(g, n):
    off = g[0]
    return make(np.concatenate([off, np.full(n - nodes(g), off[-1], dtype=np.uint64)]), g[1], g[2])


def union(a, b, strategy=KEEP_FIRST):
    """max(n_a, n_b) nodes; an arc of one keeps its label, an arc of both gets merge(l_a, l_b), a's label first."""
    n = max(nodes(a), nodes(b))
    ka, kb = sources(a) * n + a[1], sources(b) * n + b[1]                       # increasing: the lists are sorted
    at = np.searchsorted(kb, ka)
    both = (at < len(kb)) & (kb[np.minimum(at, max(len(kb) - 1, 0))] == ka) if len(kb) else np.zeros(len(ka), bool)
    la = a[2].copy()
    la[both] = MERGE[strategy](a[2][both], b[2][at[both]])
    only_b = ~np.isin(kb, ka)
    keys, lab = np.concatenate([ka, kb[only_b]]), np.concatenate([la, b[2][only_b]])
    return from_arcs(n, keys // max(n, 1), keys % max(n, 1), lab)


def symmetrize(g, strategy=KEEP_FIRST):
    return union(g, transpose(g), strategy)


def filter(g, kind, node_class=None, lower_bound=None):
    src, dst, lab = sources(g), g[1], g[2]
    if kind == NO_LOOPS:
        keep = src != dst
    elif kind == LOWER_BOUND:
        keep = lab.astype(np.int64) >= lower_bound                              # Transform.java:213: >=, whatever the javadoc says
    else:
        c = np.asarray(node_class, dtype=np.int64)
        keep = (c[src] == c[dst]) == (kind == SAME_CLASS)
    return from_arcs(nodes(g), src[keep], dst[keep], lab[keep])


def underlying(g):
    return g[0], g[1]


def equal(g, h):
    return all(len(p) == len(q) and np.array_equal(p, q) for p, q in zip(g, h))


def random_graph(rng, n, density, heavy=False, lab_max=7):
    """A random labelled graph of n nodes: every arc with probability `density`; with heavy=True one node points at (nearly) every node."""
    m = rng.random((n, n)) < density
    if heavy and n:
        m[rng.integers(n)] = rng.random(n) < 0.9
    src, dst = np.nonzero(m)
    return from_arcs(n, src, dst, rng.integers(0, lab_max + 1, len(src)))
