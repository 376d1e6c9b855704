"""A plain numpy / Python restatement of the transforms (include/bvgraph_hip.h, "Transform"): what tests/test_gpu_transform*.py hold the
device against.  A graph is (off int64[n + 1], adj int64[m]); map, filter, union and transpose work on arc arrays with np.unique; the
lex and Gray orders are Python sorts on key tuples."""
import numpy as np

INF = float("inf")
MASK = (1 << 64) - 1


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    if len(lists):
        off[1:] = np.cumsum([len(l) for l in lists])
    adj = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) and off[-1] else np.empty(0, np.int64)
    return off, adj


def lists_of(off, adj):
    off = np.asarray(off).astype(np.int64)
    return [np.asarray(adj[off[x]:off[x + 1]], dtype=np.int64) for x in range(len(off) - 1)]


def arcs_of(off, adj):
    off = np.asarray(off).astype(np.int64)
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)), np.asarray(adj, dtype=np.int64)


def from_arcs(src, dst, n):
    """The CSR of the set of arcs (duplicates once, lists sorted) over n nodes."""
    base = max(int(n), 1)
    key = np.unique(np.asarray(src, dtype=np.int64) * base + np.asarray(dst, dtype=np.int64))
    s, d = key // base, key % base
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(s, minlength=n)) if n else 0
    return off, d


def map_graph(off, adj, f):
    f = np.asarray(f, dtype=np.int64)
    n = int(f.max()) + 1 if len(f) else 0
    s, d = arcs_of(off, adj)
    s, d = f[s], f[d]
    keep = (s >= 0) & (d >= 0)
    return from_arcs(s[keep], d[keep], max(n, 0))


def filter_arcs(off, adj, kind, node_class=None):
    s, d = arcs_of(off, adj)
    if kind == "NO_LOOPS":
        keep = s != d
    else:
        c = np.asarray(node_class, dtype=np.int64)
        keep = (c[s] == c[d]) == (kind == "SAME_CLASS")
    return from_arcs(s[keep], d[keep], len(off) - 1)


def transpose(off, adj):
    s, d = arcs_of(off, adj)
    return from_arcs(d, s, len(off) - 1)


def union(a, b, drop_loops=False):
    (sa, da), (sb, db) = arcs_of(*a), arcs_of(*b)
    s, d = np.concatenate([sa, sb]), np.concatenate([da, db])
    if drop_loops:
        keep = s != d
        s, d = s[keep], d[keep]
    return from_arcs(s, d, max(len(a[0]), len(b[0])) - 1)


def symmetrize(off, adj, drop_loops=False):
    return union((off, adj), transpose(off, adj), drop_loops)


def lex_key(l):
    """The order of Transform.lexicographicalPermutation's comparator as a key: a list that ends goes first, otherwise the LARGER successor."""
    return tuple(-int(v) for v in l) + (-INF,)


def gray_key(l):
    """The order of Transform.grayCodePermutation's comparator as a key: element k is -l[k] at even k and l[k] at odd k; one terminator,
    -inf behind a list of even length (it ends at an even position: first), +inf behind one of odd length."""
    return tuple(-int(v) if k % 2 == 0 else int(v) for k, v in enumerate(l)) + (-INF if len(l) % 2 == 0 else INF,)


def permutation(lists, key):
    """perm[x] = the rank of node x when the nodes are sorted by (key(list), node id)."""
    order = sorted(range(len(lists)), key=lambda i: (key(lists[i]), i))
    perm = np.empty(len(lists), dtype=np.int64)
    perm[np.asarray(order, dtype=np.int64)] = np.arange(len(lists), dtype=np.int64)
    return perm


def keys_of(off, adj, gray):
    """lex_key / gray_key of every list of a CSR at once (the same tuples, built from two vectorised arrays: for large graphs)."""
    off = np.asarray(off).astype(np.int64); adj = np.asarray(adj, dtype=np.int64)
    deg = np.diff(off)
    pos = np.arange(len(adj), dtype=np.int64) - np.repeat(off[:-1], deg)
    v = np.where((pos % 2 == 1) & gray, adj, -adj).tolist()
    term = np.where((deg % 2 == 1) & gray, INF, -INF).tolist()
    o = off.tolist()
    return [tuple(v[o[x]:o[x + 1]]) + (term[x],) for x in range(len(deg))]


def permutation_of_csr(off, adj, gray):
    keys = keys_of(off, adj, gray)
    order = sorted(range(len(keys)), key=lambda i: (keys[i], i))
    perm = np.empty(len(keys), dtype=np.int64)
    perm[np.asarray(order, dtype=np.int64)] = np.arange(len(keys), dtype=np.int64)
    return perm


def lexicographical_permutation(lists):
    return permutation(lists, lex_key)


def gray_code_permutation(lists):
    return permutation(lists, gray_key)


def mix64(seed, node):
    z = (seed + (node + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def random_permutation(n, seed):
    order = sorted(range(n), key=lambda i: (mix64(seed & MASK, i), i))
    perm = np.empty(n, dtype=np.int64)
    perm[np.asarray(order, dtype=np.int64)] = np.arange(n, dtype=np.int64)
    return perm


def remove_dangling_map(off):
    keep = np.diff(np.asarray(off).astype(np.int64)) != 0
    return np.where(keep, np.cumsum(keep) - 1, -1)


def same(a, b):
    """Two CSRs hold the same lists."""
    return np.array_equal(np.asarray(a[0]).astype(np.int64), np.asarray(b[0]).astype(np.int64)) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
