"""Transform over the C ABI (include/bvgraph_hip.h, bvg_transform_*): map, filter, transpose, symmetrise, simplify, union and the
lexicographic / Gray code / random permutations, every result a ParsedGraph (a CSR resident on the device) that can be the source of
the next call, be stored or be written as text; the unlabelled composition (bvg_compose) with its own command line; BinIO / TextIO longs; and
the command line of Transform.main (Transform.java:2070-2381)."""
import ctypes as C
import sys

import numpy as np

from . import _abi
from .bvgraph import BVGraph, IllegalArgumentException, UnsupportedOperationException, _check, lib
from .efgraph import EFGraph
from .textgraph import ParsedGraph, _class_name, _open_source, write_bvgraph

NO_LOOPS, SAME_CLASS, DIFFERENT_CLASS = "NO_LOOPS", "SAME_CLASS", "DIFFERENT_CLASS"
_FILTERS = {NO_LOOPS: _abi.TRANSFORM_NO_LOOPS, SAME_CLASS: _abi.TRANSFORM_SAME_CLASS, DIFFERENT_CLASS: _abi.TRANSFORM_DIFFERENT_CLASS}


def _transform_fns():
    """The bvg_transform_* entry points, bound on first use (a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_transform_bound", False):
        return L
    for name, args in _abi.transform_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._transform_bound = True
    return L


def _from_csr(cls, adj_off, adj, device=0):
    """ParsedGraph.from_csr: a resident graph over (adj_off uint64[n + 1], adj int64[m]), validated as bvg_store validates its input."""
    off = np.ascontiguousarray(adj_off, dtype=np.uint64); a = np.ascontiguousarray(adj, dtype=np.int64)
    if len(off) < 1:
        raise IllegalArgumentException(_abi.E_ARG, "from_csr: adj_off holds nodes + 1 entries")
    h = C.c_void_p()
    _check(_transform_fns().bvg_transform_from_csr(len(off) - 1, off.ctypes.data, a.ctypes.data if len(a) else None, device, C.byref(h)), "from_csr")
    return cls(h, device)


def _from_csr_dev(cls, nodes, off_ptr, adj_ptr, device=0):
    """bvg_transform_from_csr_dev: the arrays are in device memory."""
    h = C.c_void_p()
    _check(_transform_fns().bvg_transform_from_csr_dev(nodes, off_ptr, adj_ptr, device, C.byref(h)), "from_csr_dev")
    return cls(h, device)


ParsedGraph.from_csr, ParsedGraph.from_csr_dev = classmethod(_from_csr), classmethod(_from_csr_dev)


class _Source:
    """A BVGraph or a ParsedGraph as a bvg_transform_src; an EFGraph (no C-level source) is decoded and goes through from_csr."""

    def __init__(self, g, device=0):
        self.tmp = None
        if isinstance(g, EFGraph):
            n = g.num_nodes()
            deg, succ = g.decode_range(0, n) if n else (np.empty(0, np.int32), np.empty(0, np.int64))
            g = self.tmp = ParsedGraph.from_csr(np.concatenate([[0], np.cumsum(deg.astype(np.int64))]).astype(np.uint64), succ, device)
        if isinstance(g, ParsedGraph):
            self.src, self.device = _abi.TransformSrc(None, g._h), g._device
        elif isinstance(g, BVGraph):
            self.src, self.device = _abi.TransformSrc(g._h, None), device
        else:
            raise IllegalArgumentException(_abi.E_ARG, "a BVGraph, an EFGraph or a ParsedGraph is expected, not %r" % type(g).__name__)
        if not (self.src.graph or self.src.csr):
            raise IllegalArgumentException(_abi.E_ARG, "the graph is closed")
        self.nodes = g.num_nodes()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.tmp is not None:
            self.tmp.close()


def _graph_call(name, g, *args):
    with _Source(g) as s:
        h = C.c_void_p()
        _check(getattr(_transform_fns(), name)(C.byref(s.src), *args, C.byref(h)), name[len("bvg_transform_"):])
        return ParsedGraph(h, s.device)


def identity_graph(g):
    """The graph as a ParsedGraph of its own (bvg_transform_identity)."""
    return _graph_call("bvg_transform_identity", g)


def map_graph(g, f):
    """Transform.mapOffline: node x becomes f[x]; -1 deletes x and every arc that touches it; max(f) + 1 nodes."""
    f = np.ascontiguousarray(f, dtype=np.int64)
    return _graph_call("bvg_transform_map", g, f.ctypes.data if len(f) else None, len(f))


def filter_arcs(g, kind, node_class=None):
    """Transform.filterArcs with NO_LOOPS, or with NodeClassFilter(node_class, keepOnlySame): SAME_CLASS / DIFFERENT_CLASS."""
    if kind not in _FILTERS:
        raise IllegalArgumentException(_abi.E_ARG, "unknown arc filter %r: one of %s" % (kind, ", ".join(sorted(_FILTERS))))
    if node_class is None:
        return _graph_call("bvg_transform_filter", g, _FILTERS[kind], None, 0)
    c = np.ascontiguousarray(node_class, dtype=np.int64)
    return _graph_call("bvg_transform_filter", g, _FILTERS[kind], c.ctypes.data if len(c) else None, len(c))


def transpose_graph(g):
    """Transform.transposeOffline."""
    return _graph_call("bvg_transform_transpose", g)


def symmetrize_graph(g):
    """Transform.symmetrizeOffline: the union of the graph and its transpose."""
    return _graph_call("bvg_transform_symmetrize", g, 0)


def simplify_graph(g):
    """Transform.simplifyOffline: symmetrised, loops dropped."""
    return _graph_call("bvg_transform_symmetrize", g, _abi.TRANSFORM_DROP_LOOPS_FLAG)


def union(a, b, drop_loops=False):
    """Transform.union(a, b): max(nodes) nodes, common arcs once; drop_loops=True is Transform.simplify(g, t)."""
    with _Source(a) as sa, _Source(b) as sb:
        h = C.c_void_p()
        _check(_transform_fns().bvg_transform_union(C.byref(sa.src), C.byref(sb.src), _abi.TRANSFORM_DROP_LOOPS_FLAG if drop_loops else 0, C.byref(h)), "union")
        return ParsedGraph(h, sa.device)


def _compose_fns():
    """bvg_compose, bound on first use."""
    L = lib()
    if getattr(L, "_compose_bound", False):
        return L
    for name, args in _abi.compose_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._compose_bound = True
    return L


def compose(a, b, report=False):
    """Transform.compose(a, b), unlabelled: row x of the result is the sorted union of b's lists over a's successors of x; max(nodes) nodes; a
    successor that b does not have contributes nothing.  report=True: (graph, dict of bvg_compose_report).  A result refused for its size
    raises UnsupportedOperationException carrying the report as .report."""
    with _Source(a) as sa, _Source(b) as sb:
        h, rep = C.c_void_p(), _abi.ComposeReport()
        st = _compose_fns().bvg_compose(C.byref(sa.src), C.byref(sb.src), C.byref(rep), C.byref(h))
        try:
            _check(st, "compose")
        except UnsupportedOperationException as e:
            e.report = rep.as_dict()
            raise
        g = ParsedGraph(h, sa.device)
        return (g, rep.as_dict()) if report else g


def _permutation(g, kind, seed=0):
    with _Source(g) as s:
        perm = np.empty(s.nodes, dtype=np.int64)
        _check(_transform_fns().bvg_transform_permutation(C.byref(s.src), kind, seed & 0xFFFFFFFFFFFFFFFF, perm.ctypes.data if s.nodes else None), "permutation")
        return perm


def permutation_dev(g, kind, perm_ptr, seed=0):
    """bvg_transform_permutation_dev: kind = PERM_LEX / PERM_GRAY / PERM_RANDOM; perm_ptr: int64[nodes] in device memory."""
    with _Source(g) as s:
        _check(_transform_fns().bvg_transform_permutation_dev(C.byref(s.src), kind, seed & 0xFFFFFFFFFFFFFFFF, perm_ptr), "permutation_dev")


def lexicographical_permutation(g):
    """Transform.lexicographicalPermutation: perm[x] = the rank of x's successor list under the comparator of Transform.java:2017-2032
    (equal lists by node id); ready for map_graph."""
    return _permutation(g, _abi.PERM_LEX)


def gray_code_permutation(g):
    """Transform.grayCodePermutation (comparator of Transform.java:1946-1975; equal lists by node id)."""
    return _permutation(g, _abi.PERM_GRAY)


def random_permutation(g, seed=0):
    """A permutation drawn from the seed: the order of (mix64(seed, node), node) of include/bvgraph_hip.h -- the library's own sequence."""
    return _permutation(g, _abi.PERM_RANDOM, seed)


def _outdegrees(g):
    n = g.num_nodes()
    if isinstance(g, ParsedGraph):
        off = np.empty(n + 1, dtype=np.uint64)
        from .textgraph import _text_fns
        _check(_text_fns().bvg_text_get(g._h, off.ctypes.data, len(off), None, 0), "text_get")
        return np.diff(off.astype(np.int64))
    return g.outdegrees(0, n).astype(np.int64) if n else np.empty(0, np.int64)


def remove_dangling(g):
    """Transform.main's removeDangling: every node of outdegree 0 is deleted, the others keep their order."""
    deg = _outdegrees(g)
    keep = deg != 0
    return map_graph(g, np.where(keep, np.cumsum(keep) - 1, -1))


# ---- BinIO / TextIO longs

def load_longs(path, ascii=False):
    """BinIO.loadLongs (big-endian int64, no header) or, with ascii=True, TextIO.loadLongs (one integer per line)."""
    if ascii:
        with open(path) as f:
            return np.array([int(t) for t in f.read().split()], dtype=np.int64)
    return np.fromfile(path, dtype=">i8").astype(np.int64)


def store_longs(path, a, ascii=False):
    """BinIO.storeLongs / TextIO.storeLongs."""
    a = np.asarray(a, dtype=np.int64)
    if ascii:
        with open(path, "w") as f:
            f.write("".join("%d\n" % v for v in a.tolist()))
    else:
        a.astype(">i8").tofile(path)
    return path


# ---- Transform.main

# transform -> (fewest, most) parameters, as the ensureNumArgs calls of Transform.java:2141-2238 have them
_ARITY = {"identity": (2, 2), "grayPerm": (2, 2), "lexPerm": (2, 2), "mapOffline": (3, 6), "random": (2, 5), "arcfilter": (3, 3), "union": (3, 3), "simplify": (3, 3),
          "transposeOffline": (2, 4), "symmetrizeOffline": (2, 4), "simplifyOffline": (2, 4), "removeDangling": (2, 4), "gray": (2, 4), "lex": (2, 4)}
_NOT_BUILT = {"compose": "compose is not built", "larcfilter": "labelled graphs are not built"}


def transform_arg_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="transform_main", description="Transforms one or more graphs on the device (Transform.main): "
                                 "identity, mapOffline, transposeOffline, symmetrizeOffline, simplify, simplifyOffline, union, removeDangling, gray, grayPerm, lex, lexPerm, "
                                 "random, arcfilter NO_LOOPS.  batchSize and tempDir are accepted and ignored.")
    ap.add_argument("-s", "--source-graph-class", dest="source_graph_class", default="BVGraph")
    ap.add_argument("-d", "--dest-graph-class", dest="dest_graph_class", default="BVGraph")
    ap.add_argument("-o", "--offline", action="store_true", help="Accepted: sources are always loaded offline.")
    ap.add_argument("-a", "--ascii", action="store_true", help="Maps are in ASCII form (one integer per line).")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("transform")
    ap.add_argument("param", nargs="*")
    return ap


def _fail(msg):
    print("transform_main: " + msg, file=sys.stderr)
    return 1


def _store_result(cls, result, dest, device):
    if cls == "BVGraph":
        write_bvgraph(dest, result, device=device)
    elif cls == "ASCIIGraph":
        result.to_ascii_graph(dest)
    elif cls == "ArcListASCIIGraph":
        result.to_arc_list(dest)
    else:
        from .efgraph import write_efgraph
        write_efgraph(dest, result.csr(), device=device)


def transform_main(argv=None):
    """Transform.main: [-s CLASS] [-d CLASS] [-o] [-a] transform param...  Returns 0, or 1 after a message for what the reference refuses
    (unknown transform, wrong number of parameters) and for what is not built here (compose, larcfilter, filters other than NO_LOOPS,
    a merge strategy for union)."""
    a = transform_arg_parser().parse_args(argv)
    t, p = a.transform, a.param
    if t in _NOT_BUILT:
        return _fail(_NOT_BUILT[t])
    if t not in _ARITY:
        return _fail("Unknown transform: " + t)
    lo, hi = _ARITY[t]
    if len(p) < lo:
        return _fail("I need at least %d arguments rather than %d." % (lo, len(p)))
    if len(p) > hi:
        if t == "union" and len(p) == 4:
            return _fail("label merge strategies are not built")
        return _fail("I need %d arguments rather than %d." % (hi, len(p)) if lo == hi else "I need at most %d arguments rather than %d." % (hi, len(p)))
    if t == "arcfilter" and p[2] != NO_LOOPS:
        return _fail("arc filter %r is not built: NO_LOOPS is" % p[2])
    try:
        cutoff = int(p[5]) if t == "mapOffline" and len(p) == 6 else -1
        seed = int(p[2]) if t == "random" and len(p) >= 3 else 0
    except ValueError as e:
        return _fail(str(e))
    scls, dcls = _class_name(a.source_graph_class), _class_name(a.dest_graph_class)
    two = t in ("union", "simplify")
    sources = [_open_source(scls, name, a.device) for name in (p[:2] if two else p[:1])]
    dest = p[2] if two else p[1]
    result = None
    try:
        g = sources[0]
        if t == "identity":
            result = identity_graph(g)
        elif t == "mapOffline":
            f = load_longs(p[2], a.ascii)
            if len(f) != g.num_nodes():
                raise IllegalArgumentException(_abi.E_ARG, "The source graph has %d nodes, but the permutation contains %d longs" % (g.num_nodes(), len(f)))
            if cutoff != -1:
                f = np.where(f >= cutoff, -1, f)
            result = map_graph(g, f)
        elif t == "transposeOffline":
            result = transpose_graph(g)
        elif t == "symmetrizeOffline":
            result = symmetrize_graph(g)
        elif t == "simplifyOffline":
            result = simplify_graph(g)
        elif t == "union":
            result = union(g, sources[1])
        elif t == "simplify":
            result = union(g, sources[1], drop_loops=True)
        elif t == "removeDangling":
            result = remove_dangling(g)
        elif t == "arcfilter":
            result = filter_arcs(g, NO_LOOPS)
        elif t in ("grayPerm", "lexPerm"):
            store_longs(dest, gray_code_permutation(g) if t == "grayPerm" else lexicographical_permutation(g))
            return 0
        else:
            perm = gray_code_permutation(g) if t == "gray" else lexicographical_permutation(g) if t == "lex" else random_permutation(g, seed)
            result = map_graph(g, perm)
        _store_result(dcls, result, dest, a.device)
    finally:
        if result is not None:
            result.close()
        for s in sources:
            s.close()
    return 0


def compose_arg_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="compose_main", description="Composes two graphs on the device (Transform.main's compose, unlabelled): "
                                 "source0 source1 dest.")
    ap.add_argument("-s", "--source-graph-class", dest="source_graph_class", default="BVGraph")
    ap.add_argument("-d", "--dest-graph-class", dest="dest_graph_class", default="BVGraph")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("param", nargs="*")
    return ap


def compose_main(argv=None):
    """Transform.main's `compose`: [-s CLASS] [-d CLASS] [--device N] source0 source1 dest.  Returns 0, or 1 after a message for a wrong
    number of parameters and for the fourth one (the semiring of the labelled composition, which is not built).  It is a command of its own
    because transform_main's answer to `compose` -- 1, before anything is opened -- is pinned by tests/test_transform_abi.py."""
    a = compose_arg_parser().parse_args(argv)
    p = a.param
    if len(p) == 4:
        print("compose_main: labelled graphs are not built", file=sys.stderr)
        return 1
    if len(p) != 3:
        print("compose_main: I need 3 arguments rather than %d." % len(p), file=sys.stderr)
        return 1
    scls, dcls = _class_name(a.source_graph_class), _class_name(a.dest_graph_class)
    sources, result = [], None
    try:
        for name in p[:2]:
            sources.append(_open_source(scls, name, a.device))
        result = compose(sources[0], sources[1])
        _store_result(dcls, result, p[2], a.device)
    finally:
        if result is not None:
            result.close()
        for s in sources:
            s.close()
    return 0
