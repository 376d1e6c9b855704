"""Test helper of tests/test_gpu_scc.py and tests/test_gpu_scc_cpp.py: the CPU side of the strongly connected components (bvg_scc;
algo/StronglyConnectedComponents.java).  The partition comes from scipy's connected_components(connection="strong") when it is
importable, from an iterative Tarjan visit otherwise, over the arcs the test built itself, and is canonicalised to the library's
numbering: component c is the one whose smallest node is the c-th smallest among the components' smallest nodes.  Buckets follow the
definition read off the reference's visit: a node is in a bucket exactly when its component has at least one arc (a self-loop counts)
and no arc leaving it."""
import numpy as np

# cnr-2000 (tests/golden/cnr-2000.graph-txt.gz), computed with scipy
CNR = dict(nodes=325557, components=100977, largest=[112023, 18233, 7518, 5618, 5060], singletons=98756, bucket_components=9994,
           bucket_nodes=32848, self_loops=87442)


def tarjan_labels(n, off, adj):
    """Any labelling of the strong components of the CSR graph (off int64[n + 1], adj): Tarjan's algorithm with an explicit stack."""
    index = np.full(n, -1, dtype=np.int64); low = np.zeros(n, dtype=np.int64); lab = np.full(n, -1, dtype=np.int64)
    on = np.zeros(n, dtype=bool)
    off = [int(v) for v in off]; adj = [int(v) for v in adj]
    stack, k, clock = [], 0, 0
    for s in range(n):
        if index[s] >= 0:
            continue
        index[s] = low[s] = clock; clock += 1
        stack.append(s); on[s] = True
        work = [(s, off[s])]
        while work:
            x, at = work[-1]
            if at < off[x + 1]:
                work[-1] = (x, at + 1)
                y = adj[at]
                if index[y] < 0:
                    index[y] = low[y] = clock; clock += 1
                    stack.append(y); on[y] = True
                    work.append((y, off[y]))
                elif on[y]:
                    low[x] = min(low[x], index[y])
                continue
            work.pop()
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[x])
            if low[x] == index[x]:
                while True:
                    y = stack.pop(); on[y] = False; lab[y] = k
                    if y == x:
                        break
                k += 1
    return lab


def cpu_scc(n, src, dst, force_tarjan=False):
    """(count, comp[n], sizes[count], buckets bool[n]) in the library's numbering."""
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    if n == 0:
        return 0, np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, bool)
    lab = None
    if not force_tarjan:
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            m = coo_matrix((np.ones(len(src), dtype=np.int8), (src, dst)), shape=(n, n)).tocsr()
            lab = connected_components(m, directed=True, connection="strong")[1].astype(np.int64)
        except ImportError:
            pass
    if lab is None:
        order = np.argsort(src, kind="stable")
        off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum(np.bincount(src, minlength=n))
        lab = tarjan_labels(n, off, dst[order])
    _, lab = np.unique(lab, return_inverse=True)
    k = int(lab.max()) + 1
    first = np.full(k, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n, dtype=np.int64))
    rank = np.empty(k, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(k, dtype=np.int64)
    comp = rank[lab]
    has_arc = np.zeros(k, dtype=bool); leaves = np.zeros(k, dtype=bool)
    has_arc[comp[src]] = True
    leaves[comp[src][comp[src] != comp[dst]]] = True
    return k, comp, np.bincount(comp, minlength=k).astype(np.int64), (has_arc & ~leaves)[comp]


def sorted_by_size(comp, sizes):
    """sortBySize with ties by increasing old index (= smallest node), as in tests/test_gpu_components.py."""
    k = len(sizes)
    order = np.lexsort((np.arange(k), -sizes))
    newidx = np.empty(k, dtype=np.int64); newidx[order] = np.arange(k, dtype=np.int64)
    return newidx[comp], sizes[order]


def arcs_of(off, adj):
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)), np.asarray(adj, dtype=np.int64)


def csr_of(n, arcs):
    """(off uint64[n + 1], adj int64) of a list of (u, v) pairs, lists sorted and without duplicates."""
    arcs = sorted(set((int(u), int(v)) for u, v in arcs))
    src = np.array([a[0] for a in arcs], dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=n)).astype(np.uint64) if n else 0
    return off, np.array([a[1] for a in arcs], dtype=np.int64)


def cut(src, dst, n, B):
    """The arcs that stay inside blocks of B consecutive nodes: (off, adj, src)."""
    keep = (src // B) == (dst // B)
    s, d = src[keep], dst[keep]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(s, minlength=n)).astype(np.uint64)
    return off, d, s


def summary(k, comp, sizes, buckets, src, dst):
    """The quantities of CNR for any graph."""
    return dict(nodes=len(comp), components=k, largest=np.sort(sizes)[::-1][:5].tolist(), singletons=int((sizes == 1).sum()),
                bucket_components=len(np.unique(comp[buckets])), bucket_nodes=int(buckets.sum()), self_loops=int((np.asarray(src) == np.asarray(dst)).sum()))
