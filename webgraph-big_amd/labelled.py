"""Arc-labelled graphs over the C ABI (include/bvgraph_hip.h, bvg_lgraph_*): a LabelledGraph is a CSR resident on the device plus one int label
per arc and the label class (GammaCodedIntLabel / FixedWidthIntLabel).  Transform's labelled half -- transpose, union and symmetrise under a
merge strategy, filterArcs with a LabelledArcFilter -- goes from LabelledGraph to LabelledGraph; the label stream is written on the device
(BitStreamArcLabelledImmutableGraph.store) and write() leaves the files BitStreamArcLabelledImmutableGraph.load reads; and the labelled part of
the command line of Transform.main (Transform.java:2295-2297, :2326-2328, :2372-2378).  compose_labelled is Transform.compose with a LabelSemiring
(bvg_lcompose): the product of two labelled graphs over one of a fixed menu of semirings, with a command line of its own."""
import ctypes as C
import os
import re
import sys

import numpy as np

from . import _abi
from .bvgraph import (BitStreamArcLabelledImmutableGraph, IllegalArgumentException, UnsupportedOperationException, LABEL_FIXED_INT, LABEL_GAMMA_INT,
                      _check, lib)
from .textgraph import ParsedGraph, coded_gaps, write_bvgraph

KEEP_FIRST, MIN, MAX, LOWER_BOUND = "KEEP_FIRST", "MIN", "MAX", "LOWER_BOUND"
_STRATEGIES = {KEEP_FIRST: _abi.LMERGE_KEEP_FIRST, MIN: _abi.LMERGE_MIN, MAX: _abi.LMERGE_MAX}
_FILTERS = {"NO_LOOPS": _abi.LFILTER_NO_LOOPS, "SAME_CLASS": _abi.LFILTER_SAME_CLASS, "DIFFERENT_CLASS": _abi.LFILTER_DIFFERENT_CLASS,
            LOWER_BOUND: _abi.LFILTER_LOWER_BOUND}
_LABEL_CLASSES = {LABEL_GAMMA_INT: "GammaCodedIntLabel", LABEL_FIXED_INT: "FixedWidthIntLabel"}
SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS, SEMIRING_MAX_MIN, SEMIRING_MIN_MAX, SEMIRING_PLUS_TIMES = (
    _abi.SEMIRING_MIN_PLUS, _abi.SEMIRING_MAX_PLUS, _abi.SEMIRING_MAX_MIN, _abi.SEMIRING_MIN_MAX, _abi.SEMIRING_PLUS_TIMES)
_SEMIRINGS = {"MIN_PLUS": SEMIRING_MIN_PLUS, "MAX_PLUS": SEMIRING_MAX_PLUS, "MAX_MIN": SEMIRING_MAX_MIN, "MIN_MAX": SEMIRING_MIN_MAX, "PLUS_TIMES": SEMIRING_PLUS_TIMES}
UNDERLYINGGRAPH_SUFFIX = "-underlying"      # ArcLabelledImmutableGraph.UNDERLYINGGRAPH_SUFFIX


def _labelled_fns():
    """The bvg_lgraph_* entry points, bound on first use (a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_labelled_bound", False):
        return L
    for name, args in _abi.labelled_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_lgraph_close.restype = None
    L._labelled_bound = True
    return L


def label_spec(kind, width):
    """Label.toSpec() of the class with the key FOO: what labelspec holds in basename.properties."""
    cls = "it.unimi.dsi.big.webgraph.labelling." + _LABEL_CLASSES[kind]
    return cls + ("(FOO)" if kind == LABEL_GAMMA_INT else "(FOO,%d)" % width)


class LabelledGraph:
    """An arc-labelled graph resident on the device (bvg_lgraph): adjacency in CSR form, int32 labels in successor order, the label class."""

    def __init__(self, handle, device=0):
        self._h, self._device = handle, device
        n, m, k, w = C.c_int64(), C.c_uint64(), C.c_int(), C.c_int()
        _check(_labelled_fns().bvg_lgraph_info(self._h, C.byref(n), C.byref(m), C.byref(k), C.byref(w)), "lgraph_info")
        self._n, self._m, self.kind, self.width = int(n.value), int(m.value), int(k.value), int(w.value)

    @classmethod
    def from_csr(cls, adj_off, adj, labels, kind, width=0, device=0):
        """A resident graph over (adj_off uint64[n + 1], adj int64[m], labels int32[m]): the CSR validated as ParsedGraph.from_csr validates it,
        every label against its class (gamma: >= 0; fixed: width in 0..31 and 0 <= label < 2^width)."""
        off = np.ascontiguousarray(adj_off, dtype=np.uint64); a = np.ascontiguousarray(adj, dtype=np.int64)
        lab64 = np.asarray(labels, dtype=np.int64)
        if len(off) < 1:
            raise IllegalArgumentException(_abi.E_ARG, "from_csr: adj_off holds nodes + 1 entries")
        if len(lab64) != len(a) or (len(lab64) and (lab64.min() < -(1 << 31) or lab64.max() >= (1 << 31))):
            raise IllegalArgumentException(_abi.E_ARG, "from_csr: one int label per arc")
        lab = np.ascontiguousarray(lab64, dtype=np.int32)
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_from_csr(len(off) - 1, off.ctypes.data, a.ctypes.data if len(a) else None, lab.ctypes.data if len(lab) else None,
                                                  kind, width, device, C.byref(h)), "from_csr")
        return cls(h, device)

    @classmethod
    def from_csr_dev(cls, nodes, off_ptr, adj_ptr, labels_ptr, kind, width=0, device=0):
        """bvg_lgraph_from_csr_dev: the three arrays are in device memory."""
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_from_csr_dev(nodes, off_ptr, adj_ptr, labels_ptr, kind, width, device, C.byref(h)), "from_csr_dev")
        return cls(h, device)

    @classmethod
    def from_graph(cls, g, device=0):
        """A BitStreamArcLabelledImmutableGraph, decoded once: the graph and its labels (bvg_lgraph_from_labelled)."""
        if not isinstance(g, BitStreamArcLabelledImmutableGraph):
            raise IllegalArgumentException(_abi.E_ARG, "a BitStreamArcLabelledImmutableGraph is expected, not %r" % type(g).__name__)
        if not (g._h and g.g._h):
            raise IllegalArgumentException(_abi.E_ARG, "the graph is closed")
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_from_labelled(g.g._h, g._h, C.byref(h)), "from_graph")
        return cls(h, device)

    def close(self):
        if getattr(self, "_h", None):
            _labelled_fns().bvg_lgraph_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def num_nodes(self):
        return self._n

    def num_arcs(self):
        return self._m

    numNodes, numArcs = num_nodes, num_arcs

    def csr(self):
        """(adj_off uint64[n + 1], adj int64[m], labels int32[m])."""
        off = np.empty(self._n + 1, dtype=np.uint64); adj = np.empty(self._m, dtype=np.int64); lab = np.empty(self._m, dtype=np.int32)
        _check(_labelled_fns().bvg_lgraph_get(self._h, off.ctypes.data, len(off), adj.ctypes.data if self._m else None, self._m,
                                             lab.ctypes.data if self._m else None, self._m), "lgraph_get")
        return off, adj, lab

    def csr_dev(self, off_ptr, off_cap, adj_ptr, adj_cap, labels_ptr, labels_cap):
        """bvg_lgraph_get_dev: into device buffers (capacities in elements)."""
        _check(_labelled_fns().bvg_lgraph_get_dev(self._h, off_ptr, off_cap, adj_ptr, adj_cap, labels_ptr, labels_cap), "lgraph_get_dev")

    def underlying(self):
        """The unlabelled graph as a ParsedGraph of its own: every unlabelled transform, store and the text writers apply to it."""
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_underlying(self._h, C.byref(h)), "lgraph_underlying")
        return ParsedGraph(h, self._device)

    def store_labels(self):
        """BitStreamArcLabelledImmutableGraph.store's label stream, written on the device: (the bytes of basename.labels uint8[],
        label_offsets uint64[n + 1], the bit position of every node's first label)."""
        s = C.c_void_p(); o = C.c_void_p(); nb = C.c_uint64()
        L = _labelled_fns()
        _check(L.bvg_lgraph_store_labels(self._h, C.byref(s), C.byref(nb), C.byref(o)), "lgraph_store_labels")
        try:
            stream = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_uint8)), shape=(max(int(nb.value), 1),))[:int(nb.value)].copy()
            offsets = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(self._n + 1,)).copy()
        finally:
            L.bvg_free(s); L.bvg_free(o)
        return stream, offsets

    def store_labels_dev(self, stream_ptr, cap, offsets_ptr):
        """bvg_lgraph_store_labels_dev: into device buffers (cap in bytes; offsets_ptr: uint64[n + 1]); returns the stream's length in bytes."""
        nb = C.c_uint64()
        _check(_labelled_fns().bvg_lgraph_store_labels_dev(self._h, stream_ptr, cap, C.byref(nb), offsets_ptr), "lgraph_store_labels_dev")
        return int(nb.value)

    def write(self, basename, params=None):
        """What Transform.main writes for a labelled result (Transform.java:2372-2378): basename.labels, basename.labeloffsets (the gamma-coded
        gaps of the label offsets after a leading gamma(0)), basename.properties (saveProperties, BitStreamArcLabelledImmutableGraph.java:693-699)
        and the underlying BVGraph under basename-underlying.  BitStreamArcLabelledImmutableGraph.load(basename) reads the result."""
        stream, offsets = self.store_labels()
        with open(basename + ".labels", "wb") as f:
            f.write(stream.tobytes())
        with open(basename + ".labeloffsets", "wb") as f:
            f.write(coded_gaps(offsets, _abi.GAMMA))
        under = (basename if os.path.isabs(basename) else os.path.basename(basename)) + UNDERLYINGGRAPH_SUFFIX
        with open(basename + ".properties", "w") as f:
            f.write("graphclass = it.unimi.dsi.big.webgraph.labelling.BitStreamArcLabelledImmutableGraph\n"
                    "underlyinggraph = %s\nlabelspec = %s\n" % (under, label_spec(self.kind, self.width)))
        with self.underlying() as u:
            write_bvgraph(basename + UNDERLYINGGRAPH_SUFFIX, u, params, device=self._device)
        return stream, offsets


class _LSource:
    """A LabelledGraph, used where it lies, or a BitStreamArcLabelledImmutableGraph, converted once and closed afterwards."""

    def __init__(self, g):
        self.tmp = None
        if isinstance(g, BitStreamArcLabelledImmutableGraph):
            g = self.tmp = LabelledGraph.from_graph(g)
        if not isinstance(g, LabelledGraph):
            raise IllegalArgumentException(_abi.E_ARG, "a LabelledGraph or a BitStreamArcLabelledImmutableGraph is expected, not %r" % type(g).__name__)
        if not g._h:
            raise IllegalArgumentException(_abi.E_ARG, "the graph is closed")
        self.g = g

    def __enter__(self):
        return self.g

    def __exit__(self, *exc):
        if self.tmp is not None:
            self.tmp.close()


def _strategy(name):
    if name not in _STRATEGIES:
        raise IllegalArgumentException(_abi.E_ARG, "unknown merge strategy %r: one of %s" % (name, ", ".join(sorted(_STRATEGIES))))
    return _STRATEGIES[name]


def transpose_labelled(g):
    """Transform.transposeOffline on a labelled graph: arc (x, y) with label l becomes (y, x) with label l."""
    with _LSource(g) as s:
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_transpose(s._h, C.byref(h)), "transpose_labelled")
        return LabelledGraph(h, s._device)


def union_labelled(a, b, strategy=KEEP_FIRST):
    """Transform.union(a, b, strategy): an arc of both gets merge(label_a, label_b) -- KEEP_FIRST (Labels.KEEP_FIRST_MERGE_STRATEGY), MIN or MAX."""
    st = _strategy(strategy)
    with _LSource(a) as sa, _LSource(b) as sb:
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_union(sa._h, sb._h, st, C.byref(h)), "union_labelled")
        return LabelledGraph(h, sa._device)


def symmetrize_labelled(g, strategy=KEEP_FIRST):
    """Transform.symmetrizeOffline on a labelled graph: union(g, transpose(g), strategy)."""
    st = _strategy(strategy)
    with _LSource(g) as s:
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_symmetrize(s._h, st, C.byref(h)), "symmetrize_labelled")
        return LabelledGraph(h, s._device)


def filter_labelled_arcs(g, kind, node_class=None, lower_bound=None):
    """Transform.filterArcs with a LabelledArcFilter: NO_LOOPS, SAME_CLASS / DIFFERENT_CLASS (node_class), or LOWER_BOUND -- Transform.LowerBound
    as its code has it: an arc stays iff label >= lower_bound."""
    if kind not in _FILTERS:
        raise IllegalArgumentException(_abi.E_ARG, "unknown arc filter %r: one of %s" % (kind, ", ".join(sorted(_FILTERS))))
    if (kind == LOWER_BOUND) != (lower_bound is not None):
        raise IllegalArgumentException(_abi.E_ARG, "lower_bound goes with LOWER_BOUND, and with no other filter")
    c = None if node_class is None else np.ascontiguousarray(node_class, dtype=np.int64)
    with _LSource(g) as s:
        h = C.c_void_p()
        _check(_labelled_fns().bvg_lgraph_filter(s._h, _FILTERS[kind], c.ctypes.data if c is not None and len(c) else None, len(c) if c is not None else 0,
                                                int(lower_bound) if lower_bound is not None else 0, C.byref(h)), "filter_labelled_arcs")
        return LabelledGraph(h, s._device)


def _lcompose_fns():
    """bvg_lcompose, bound on first use."""
    L = _labelled_fns()
    if getattr(L, "_lcompose_bound", False):
        return L
    for name, args in _abi.lcompose_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._lcompose_bound = True
    return L


def _semiring(s):
    if isinstance(s, str) and s in _SEMIRINGS:
        return _SEMIRINGS[s]
    if isinstance(s, (int, np.integer)) and not isinstance(s, bool) and int(s) in _SEMIRINGS.values():
        return int(s)
    raise IllegalArgumentException(_abi.E_ARG, "unknown semiring %r: one of %s" % (s, ", ".join(sorted(_SEMIRINGS))))


def compose_labelled(a, b, semiring, out_width=None, report=False):
    """Transform.compose(a, b, semiring): the successors of the unlabelled product, and on (x, z) the semiring's sum over every y with x -> y
    in a and y -> z in b of label_a(x, y) (x) label_b(y, z).  semiring: "MIN_PLUS", "MAX_PLUS", "MAX_MIN", "MIN_MAX", "PLUS_TIMES" (add, multiply)
    or its SEMIRING_* number.  out_width: the width of a FixedWidthIntLabel result (None keeps the sources').  The arithmetic is exact: a label
    outside the result's class raises IllegalArgumentException with .report, .out_of_range and .first_arc = the smallest (row, successor) among
    them; a result refused for its size raises UnsupportedOperationException with .report.  report=True: (graph, dict of bvg_lcompose_report)."""
    sr = _semiring(semiring)
    if out_width is not None and not (isinstance(out_width, (int, np.integer)) and 0 <= int(out_width) <= 31):
        raise IllegalArgumentException(_abi.E_ARG, "out_width is None or in 0..31, not %r" % (out_width,))
    with _LSource(a) as sa, _LSource(b) as sb:
        h, rep = C.c_void_p(), _abi.LComposeReport()
        st = _lcompose_fns().bvg_lcompose(sa._h, sb._h, sr, -1 if out_width is None else int(out_width), C.byref(rep), C.byref(h))
        if st == _abi.E_ARG and rep.out_of_range:
            e = IllegalArgumentException(st, "compose_labelled: %d labels outside the result's class, the first on arc (%d, %d)"
                                         % (rep.out_of_range, rep.first_row, rep.first_successor))
            e.report, e.out_of_range, e.first_arc = rep.as_dict(), int(rep.out_of_range), (int(rep.first_row), int(rep.first_successor))
            raise e
        try:
            _check(st, "compose_labelled")
        except UnsupportedOperationException as e:
            e.report = rep.as_dict()
            raise
        g = LabelledGraph(h, sa._device)
        return (g, rep.as_dict()) if report else g


# ---- Transform.main, the labelled transforms

_LARITY = {"transposeOffline": (2, 2), "symmetrizeOffline": (3, 3), "union": (4, 4), "larcfilter": (3, 3)}


def labelled_transform_arg_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="labelled_transform_main", description="Transforms arc-labelled graphs on the device (Transform.main on "
                                 "BitStreamArcLabelledImmutableGraph sources): transposeOffline src dest, symmetrizeOffline src dest STRATEGY, union src0 src1 dest "
                                 "STRATEGY, larcfilter src dest FILTER.  STRATEGY: KEEP_FIRST, MIN, MAX.  FILTER: NO_LOOPS, LowerBound(<int>); the node class "
                                 "filters are left to the API (filter_labelled_arcs).")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("transform")
    ap.add_argument("param", nargs="*")
    return ap


def _lfail(msg):
    print("labelled_transform_main: " + msg, file=sys.stderr)
    return 1


def _is_labelled(basename):
    try:
        with open(basename + ".properties") as f:
            return re.search(r"^\s*labelspec\s*[=:]", f.read(), flags=re.M) is not None
    except OSError:
        return True                                                          # (the load reports a file that is not there)


def labelled_transform_main(argv=None):
    """The labelled transforms of Transform.main: [--device N] transform param...  Returns 0, or 1 after a message for what the reference refuses
    (a union without a merge strategy, larcfilter on an unlabelled graph, a wrong number of parameters, an unknown transform) and for a
    strategy or filter that is not built."""
    a = labelled_transform_arg_parser().parse_args(argv)
    t, p = a.transform, a.param
    if t not in _LARITY:
        return _lfail("Unknown transform: " + t)
    lo, hi = _LARITY[t]
    if t == "union" and len(p) == 3:
        return _lfail("Uniting labelled graphs requires a merge strategy")       # Transform.java:2327
    if len(p) != lo:
        return _lfail("I need %d arguments rather than %d." % (hi, len(p)))
    strategy = bound = None
    if t in ("symmetrizeOffline", "union"):
        strategy = p[-1].rsplit(".", 1)[-1].replace("_MERGE_STRATEGY", "")
        if strategy not in _STRATEGIES:
            return _lfail("merge strategy %r is not built: %s are" % (p[-1], ", ".join(sorted(_STRATEGIES))))
    if t == "larcfilter":
        m = re.fullmatch(r"(?:[A-Za-z_.$]*[.$])?LowerBound\(\s*(-?\d+)\s*\)", p[2])
        if m:
            bound = int(m.group(1))
        elif p[2] != "NO_LOOPS":
            return _lfail("labelled arc filter %r is not built: NO_LOOPS and LowerBound(<int>) are" % p[2])
    names = p[:2] if t == "union" else p[:1]
    dest = p[2] if t == "union" else p[1]
    if t == "larcfilter" and not _is_labelled(names[0]):
        return _lfail("Filtering on labelled arcs requires a labelled graph")    # Transform.java:2296
    opened, sources, result = [], [], None
    try:
        for name in names:
            g = BitStreamArcLabelledImmutableGraph.load(name, a.device)
            opened.append(g)
            sources.append(LabelledGraph.from_graph(g, a.device))
        if t == "transposeOffline":
            result = transpose_labelled(sources[0])
        elif t == "symmetrizeOffline":
            result = symmetrize_labelled(sources[0], strategy)
        elif t == "union":
            result = union_labelled(sources[0], sources[1], strategy)
        elif bound is not None:
            result = filter_labelled_arcs(sources[0], LOWER_BOUND, lower_bound=bound)
        else:
            result = filter_labelled_arcs(sources[0], "NO_LOOPS")
        result.write(dest)
    finally:
        if result is not None:
            result.close()
        for s in sources:
            s.close()
        for g in opened:
            g.close()
            g.g.close()
    return 0


# ---- the labelled composition's command line

def labelled_compose_arg_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="labelled_compose_main", description="Composes two arc-labelled graphs on the device (Transform.compose with a "
                                 "LabelSemiring): source0 source1 dest SEMIRING.  SEMIRING (add_multiply): " + ", ".join(sorted(_SEMIRINGS)) + ".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--width", type=int, default=None, help="the width of a FixedWidthIntLabel result (default: the sources')")
    ap.add_argument("param", nargs="*")
    return ap


def labelled_compose_main(argv=None):
    """[--device N] source0 source1 dest SEMIRING [--width W]: loads two BitStreamArcLabelledImmutableGraphs and write()s their composition.
    Returns 0, or 1 after a message for a wrong number of parameters or an unknown semiring."""
    a = labelled_compose_arg_parser().parse_args(argv)
    p = a.param
    if len(p) != 4:
        print("labelled_compose_main: I need 4 arguments rather than %d." % len(p), file=sys.stderr)
        return 1
    if p[3] not in _SEMIRINGS:
        print("labelled_compose_main: unknown semiring %r: one of %s" % (p[3], ", ".join(sorted(_SEMIRINGS))), file=sys.stderr)
        return 1
    opened, sources, result = [], [], None
    try:
        for name in p[:2]:
            g = BitStreamArcLabelledImmutableGraph.load(name, a.device)
            opened.append(g)
            sources.append(LabelledGraph.from_graph(g, a.device))
        result = compose_labelled(sources[0], sources[1], p[3], out_width=a.width)
        result.write(p[2])
    finally:
        if result is not None:
            result.close()
        for s in sources:
            s.close()
        for g in opened:
            g.close()
            g.g.close()
    return 0
