"""A plain numpy restatement of the graph product (include/bvgraph_hip.h, "Compose"): what tests/test_gpu_compose*.py hold the device
against.  A graph is (off int64[n + 1], adj int64[m]).  Row x of compose(a, b) is the sorted set of the successors in b of the
successors of x in a; the result has max(na, nb) nodes and a successor y >= nb contributes nothing.  The products are expanded and made
unique by np.unique on x * n + z, in chunks of rows, so memory stays with a chunk's products."""
import numpy as np

CHUNK = 20000


def bounds(a, b):
    """ub[x] = the sum of outdeg_b(y) over the successors y < nb of x in a, for the max(na, nb) rows of the result."""
    (off0, adj0), (off1, adj1) = a, b
    off0, off1, adj0 = np.asarray(off0).astype(np.int64), np.asarray(off1).astype(np.int64), np.asarray(adj0).astype(np.int64)
    n0, n1 = len(off0) - 1, len(off1) - 1
    deg1 = np.concatenate([np.diff(off1), np.zeros(1, np.int64)])           # deg1[n1] = 0: where a missing successor is sent
    per_arc = deg1[np.minimum(adj0, n1)]
    cum = np.concatenate([np.zeros(1, np.int64), np.cumsum(per_arc)])
    ub = np.zeros(max(n0, n1), dtype=np.int64)
    ub[:n0] = cum[off0[1:]] - cum[off0[:-1]]
    return ub


def compose(a, b, chunk=CHUNK):
    (off0, adj0), (off1, adj1) = a, b
    off0, off1 = np.asarray(off0).astype(np.int64), np.asarray(off1).astype(np.int64)
    adj0, adj1 = np.asarray(adj0).astype(np.int64), np.asarray(adj1).astype(np.int64)
    n0, n1 = len(off0) - 1, len(off1) - 1
    n = max(n0, n1)
    counts = np.zeros(n, dtype=np.int64)
    parts = []
    for lo in range(0, n0, chunk):
        hi = min(n0, lo + chunk)
        y = adj0[off0[lo]:off0[hi]]
        x = np.repeat(np.arange(lo, hi, dtype=np.int64), np.diff(off0[lo:hi + 1]))
        keep = y < n1
        x, y = x[keep], y[keep]
        deg = off1[y + 1] - off1[y]
        total = int(deg.sum())
        if not total:
            continue
        # product p of the chunk belongs to arc i = the last one with start[i] <= p, and is the (p - start[i])-th successor of y[i]
        start = np.cumsum(deg) - deg
        arc = np.repeat(np.arange(len(y), dtype=np.int64), deg)
        z = adj1[off1[y][arc] + (np.arange(total, dtype=np.int64) - start[arc])]
        key = np.unique(x[arc] * n + z)
        counts[lo:hi] = np.bincount(key // n - lo, minlength=hi - lo)
        parts.append(key % n)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)])
    adj = np.concatenate(parts) if parts else np.empty(0, np.int64)
    return off, adj


def compose_sets(la, lb):
    """The same over Python lists of lists, with sets."""
    n = max(len(la), len(lb))
    out = []
    for x in range(n):
        s = set()
        if x < len(la):
            for y in la[x]:
                if y < len(lb):
                    s.update(int(z) for z in lb[y])
        out.append(sorted(s))
    return out


def prefix(off, adj, k):
    """The subgraph of the nodes below k: their lists, cut to the successors below k."""
    off, adj = np.asarray(off).astype(np.int64), np.asarray(adj).astype(np.int64)
    src = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    keep = (src < k) & (adj < k)
    new_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.bincount(src[keep], minlength=k)[:k])])
    return new_off, adj[keep]


_cache = {}


def cached(name, make):
    """One model result per process and name (cnr-2000 composed with itself takes seconds): shared by the tests, never changed."""
    if name not in _cache:
        off, adj = make()
        off.setflags(write=False); adj.setflags(write=False)
        _cache[name] = (off, adj)
    return _cache[name]
