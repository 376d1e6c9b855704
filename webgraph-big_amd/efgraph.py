"""EFGraph over the C ABI (include/bvgraph_hip.h, bvg_ef_*): the host-side mirror of it.unimi.dsi.big.webgraph.EFGraph --
load, successors, skipTo, scan, and EFGraph.store / EFGraph.main (EFGraph.java:773-849, :1178-1244)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import _abi
from ._abi import EFParams, ScanResult
from .bvgraph import (BVGraph, IllegalArgumentException, UnsupportedOperationException, _check, lib)


def _ef_fns():
    """The bvg_ef_* entry points, bound on first use (a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_ef_bound", False):
        return L
    for name, args in _abi.ef_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_ef_close.restype = None
    L._ef_bound = True
    return L


def parse_ef_properties(text):
    """bvg_ef_parse_properties: EFParams of the text of basename.properties."""
    if isinstance(text, str):
        text = text.encode()
    p = EFParams()
    _check(_ef_fns().bvg_ef_parse_properties(text, len(text), C.byref(p)), "parse_ef_properties")
    return p


def derive_ef_offsets(params, graph_bytes):
    """bvg_ef_derive_offsets (host only): the nodes + 1 offsets of a bare stream."""
    g = np.frombuffer(bytes(graph_bytes), dtype=np.uint8)
    out = np.empty(params.nodes + 1, dtype=np.uint64)
    _check(_ef_fns().bvg_ef_derive_offsets(C.byref(params), g.ctypes.data if len(g) else None, len(g), out.ctypes.data), "derive_ef_offsets")
    return out


def _csr(adj):
    if isinstance(adj, tuple):
        return np.ascontiguousarray(adj[0], dtype=np.uint64), np.ascontiguousarray(adj[1], dtype=np.int64)
    off = np.zeros(len(adj) + 1, dtype=np.uint64)
    if len(adj):
        off[1:] = np.cumsum([len(l) for l in adj], dtype=np.uint64)
    succ = np.concatenate([np.asarray(l, dtype=np.int64) for l in adj]) if len(adj) and off[-1] else np.empty(0, np.int64)
    return off, np.ascontiguousarray(succ, dtype=np.int64)


def store_efgraph(adj, upper_bound=None, log2_quantum=8, byteorder="LITTLE_ENDIAN", device=0):
    """EFGraph.store on the device (bvg_ef_store): adj = (adj_off uint64[n + 1], succ int64[m]) or a list of sorted lists.
    Returns (graph uint8[], offsets uint64[n + 1]): the bytes of basename.graph, trailing word included."""
    if byteorder not in ("LITTLE_ENDIAN", "BIG_ENDIAN"):
        raise IllegalArgumentException(_abi.E_ARG, "unknown byte order %r" % (byteorder,))
    off, succ = _csr(adj)
    n = len(off) - 1
    ub = n if upper_bound is None else int(upper_bound)
    g = C.c_void_p(); o = C.c_void_p(); nb = C.c_uint64()
    sb = succ if len(succ) else np.zeros(1, np.int64)
    L = _ef_fns()
    _check(L.bvg_ef_store(n, ub, log2_quantum, int(byteorder == "BIG_ENDIAN"), off.ctypes.data, sb.ctypes.data, device, C.byref(g), C.byref(nb), C.byref(o)), "store_efgraph")
    try:
        graph = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=(int(nb.value),)).copy()
        offsets = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    finally:
        L.bvg_free(g); L.bvg_free(o)
    return graph, offsets


def _delta_coded_gaps(offsets):
    """basename.offsets (EFGraph.java:785, :812): nodes + 1 delta-coded gaps, MSB first, the first being 0."""
    off = np.asarray(offsets, dtype=np.uint64).astype(object)
    gaps = [0] + [int(off[i + 1] - off[i]) for i in range(len(off) - 1)]
    out, acc, nbits = bytearray(), 0, 0
    for x in gaps:
        x += 1
        m = x.bit_length() - 1                    # delta(x): gamma(m), then the low m bits of x + 1
        g = m + 1
        mm = g.bit_length() - 1
        acc = (acc << (2 * mm + 1 + m)) | (g << m) | (x & ((1 << m) - 1))
        nbits += 2 * mm + 1 + m
        while nbits >= 8:
            nbits -= 8
            out.append(acc >> nbits)
            acc &= (1 << nbits) - 1
    if nbits:
        out.append(acc << (8 - nbits))
    return bytes(out)


def _format3(x):
    """DecimalFormat("0.###")."""
    s = "%.3f" % x
    return s.rstrip("0").rstrip(".") if "." in s else s


def write_efgraph(basename, adj, upper_bound=None, log2_quantum=8, byteorder="LITTLE_ENDIAN", device=0):
    """EFGraph.store(graph, upperBound, basename, log2Quantum, ..., byteOrder) (EFGraph.java:773-849): writes basename.graph, .offsets and
    .properties with the reference's keys; `compratio` is left out (it needs a log-gamma of n^2: a statistic, nothing reads it)."""
    off, succ = _csr(adj)
    n, arcs = len(off) - 1, int(off[-1])
    ub = n if upper_bound is None else int(upper_bound)
    graph, offsets = store_efgraph((off, succ), ub, log2_quantum, byteorder, device)
    with open(basename + ".graph", "wb") as f:
        f.write(graph.tobytes())
    with open(basename + ".offsets", "wb") as f:
        f.write(_delta_coded_gaps(offsets))
    deg = np.diff(off.astype(np.int64))
    bits_deg = int(np.sum(2 * np.floor(np.log2(deg + 1)).astype(np.int64) + 1)) if n else 0       # gamma(d): 2 msb(d + 1) + 1 bits
    written = len(graph) * 8
    props = [("nodes", n), ("arcs", arcs)]
    if ub != n:
        props.append(("upperbound", ub))
    props += [("quantum", 1 << log2_quantum), ("byteorder", byteorder),
              ("bitsperlink", _format3(written / arcs) if arcs else "NaN"), ("bitspernode", _format3(written / n) if n else "NaN"),
              ("avgbitsforoutdegrees", _format3(bits_deg / n) if n else "NaN"), ("bitsforoutdegrees", bits_deg),
              ("bitsforsuccessors", int(offsets[-1]) - bits_deg), ("graphclass", "it.unimi.dsi.big.webgraph.EFGraph"), ("version", 0)]
    with open(basename + ".properties", "w") as f:
        f.write("#EFGraph properties\n" + "".join("%s=%s\n" % kv for kv in props))
    return graph, offsets


class EFGraph:
    """ImmutableGraph / EFGraph surface, backed by HBM-resident data."""

    def __init__(self, handle, keep=()):
        self._h = handle
        self._keep = keep
        self._params = EFParams()
        _check(_ef_fns().bvg_ef_info(self._h, C.byref(self._params)), "info")
        self._basename = None

    @classmethod
    def load(cls, basename, device=0, mode=_abi.LOAD_STANDARD):
        h = C.c_void_p()
        _check(_ef_fns().bvg_ef_open(os.fsencode(basename), mode, device, C.byref(h)), "load(%s)" % basename)
        g = cls(h); g._basename = basename
        return g

    @classmethod
    def from_memory(cls, params, graph_bytes, offsets=None, device=0):
        g = np.frombuffer(bytes(graph_bytes), dtype=np.uint8) if not isinstance(graph_bytes, np.ndarray) else np.ascontiguousarray(graph_bytes, dtype=np.uint8)
        o = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(_ef_fns().bvg_ef_open_mem(C.byref(params), g.ctypes.data if len(g) else None, len(g), None if o is None else o.ctypes.data, device, C.byref(h)), "ef_open_mem")
        return cls(h)

    @classmethod
    def from_device(cls, params, d_words_ptr, nbytes, d_offsets_ptr, device=0, keep=()):
        """Adopts little-endian words already in HBM (e.g. a torch tensor; pass it in `keep`)."""
        h = C.c_void_p()
        _check(_ef_fns().bvg_ef_open_dev(C.byref(params), d_words_ptr, nbytes, d_offsets_ptr, device, C.byref(h)), "ef_open_dev")
        return cls(h, keep=keep)

    def copy(self):
        h = C.c_void_p()
        _check(_ef_fns().bvg_ef_copy(self._h, C.byref(h)), "copy")
        g = EFGraph(h, keep=self._keep); g._basename = self._basename
        return g

    def close(self):
        if getattr(self, "_h", None):
            _ef_fns().bvg_ef_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def params(self):
        return self._params

    def num_nodes(self):
        return int(self._params.nodes)

    def num_arcs(self):
        if self._params.arcs < 0:
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, "numArcs")
        return int(self._params.arcs)

    def upper_bound(self):
        return int(self._params.upper_bound)

    def log2_quantum(self):
        return int(self._params.log2_quantum)

    numNodes, numArcs = num_nodes, num_arcs

    def basename(self):
        return self._basename

    def offsets(self):
        out = np.empty(self.num_nodes() + 1, dtype=np.uint64)
        _check(_ef_fns().bvg_ef_get_offsets(self._h, out.ctypes.data), "get_offsets")
        return out

    def outdegrees(self, frm=0, to=None):
        to = self.num_nodes() if to is None else to
        out = np.empty(max(to - frm, 0), dtype=np.int32)
        _check(_ef_fns().bvg_ef_outdegrees(self._h, frm, to, out.ctypes.data if len(out) else None), "outdegrees")
        return out

    def _sized(self, call, count, what):
        deg = np.empty(max(count, 1), dtype=np.int32)
        need = C.c_uint64(0)
        cap = max(1024, 16 * count)
        while True:
            succ = np.empty(cap, dtype=np.int64)
            st = call(deg.ctypes.data, succ.ctypes.data, cap, C.byref(need))
            if st == _abi.E_CAPACITY:
                cap = int(need.value)
                continue
            _check(st, what)
            return deg[:count], succ[:need.value]

    def decode_range(self, frm, to):
        """(outdeg int32[to - frm], succ int64[sum]) of nodes [frm, to)."""
        if frm < 0 or to > self.num_nodes() or frm > to:
            raise IllegalArgumentException(_abi.E_ARG, "decode_range(%d,%d)" % (frm, to))
        L = _ef_fns()
        return self._sized(lambda d, s, cap, need: L.bvg_ef_decode_range(self._h, frm, to, d, s, cap, need), to - frm, "decode_range(%d,%d)" % (frm, to))

    def successors_batch(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        L = _ef_fns()
        return self._sized(lambda d, s, cap, need: L.bvg_ef_successors_batch(self._h, nodes.ctypes.data if len(nodes) else None, len(nodes), d, s, cap, need), len(nodes), "successors_batch")

    def successor_array(self, x):
        if x < 0 or x >= self.num_nodes():
            raise IllegalArgumentException(_abi.E_ARG, "successors(%d)" % x)
        return self.decode_range(x, x + 1)[1]

    def skip_to(self, nodes, bounds):
        """skipTo(bounds[i]) on a fresh iterator over successors(nodes[i]): the smallest successor >= bounds[i], or -1."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64); bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if nodes.shape != bounds.shape or nodes.ndim != 1:
            raise IllegalArgumentException(_abi.E_ARG, "skip_to: nodes and bounds are one-dimensional arrays of one length")
        out = np.empty(len(nodes), dtype=np.int64)
        if len(nodes):
            _check(_ef_fns().bvg_ef_skip_to_batch(self._h, nodes.ctypes.data, bounds.ctypes.data, len(nodes), out.ctypes.data), "skip_to")
        return out

    def last_kernel_ms(self):
        ms = C.c_double()
        _check(_ef_fns().bvg_ef_last_kernel_ms(self._h, C.byref(ms)), "last_kernel_ms")
        return ms.value

    def scan(self, frm=0, to=None):
        to = self.num_nodes() if to is None else to
        r = ScanResult()
        _check(_ef_fns().bvg_ef_scan(self._h, frm, to, C.byref(r)), "scan")
        return r.as_dict()


def bvgraph_to_efgraph(graph, upper_bound=None, log2_quantum=8, byteorder="LITTLE_ENDIAN", device=0, basename=None, batch_arcs=1 << 26):
    """BVGraph.to_efgraph: decodes the graph in arc-bounded decode_range batches into one CSR and stores it as an EFGraph; with
    `basename` the three files are written too.  Returns the EFGraph, loaded from the bytes just written."""
    n = graph.num_nodes()
    deg = graph.outdegrees(0, n).astype(np.int64) if n else np.empty(0, np.int64)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum(deg, dtype=np.uint64)
    succ = np.empty(int(off[-1]), dtype=np.int64)
    lo = 0
    while lo < n:
        hi = int(np.searchsorted(off, off[lo] + np.uint64(batch_arcs), side="right")) - 1      # the most nodes whose arcs fit the batch
        hi = min(max(hi, lo + 1), n)
        succ[int(off[lo]):int(off[hi])] = graph.decode_range(lo, hi)[1]
        lo = hi
    ub = n if upper_bound is None else int(upper_bound)
    if basename is not None:
        data, offsets = write_efgraph(basename, (off, succ), ub, log2_quantum, byteorder, device)
    else:
        data, offsets = store_efgraph((off, succ), ub, log2_quantum, byteorder, device)
    p = EFParams(nodes=n, arcs=int(off[-1]), upper_bound=ub, log2_quantum=log2_quantum, big_endian=int(byteorder == "BIG_ENDIAN"))
    g = EFGraph.from_memory(p, data, offsets, device)
    g._basename = basename
    return g


BVGraph.to_efgraph = bvgraph_to_efgraph


def efgraph_arg_parser():
    ap = argparse.ArgumentParser(prog="efgraph_main", description="Compresses a graph using the Elias-Fano representation (EFGraph.main, EFGraph.java:1178-1244). "
                                 "The source is the basename of a BVGraph or of an EFGraph; the destination is written as an EFGraph.")
    ap.add_argument("-q", "--log2-quantum", type=int, default=8, dest="log2_quantum", help="The base-two logarithm of the indexing quantum.")
    ap.add_argument("-o", "--offline", action="store_true", help="No-op for backward compatibility.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("sourceBasename")
    ap.add_argument("destBasename", nargs="?")
    return ap


def efgraph_main(argv=None):
    """EFGraph.main: [-q log2Quantum] source [dest].  Without a destination the reference only precomputes offset caches (-L / -F),
    which need a JVM: here that is an error message."""
    a = efgraph_arg_parser().parse_args(argv)
    if a.destBasename is None:
        print("efgraph_main: no destination basename: nothing to do (the offset-list caches of --list / --fixed-width-list are not built)", file=sys.stderr)
        return 1
    if a.log2_quantum < 0:
        print("efgraph_main: log2Quantum must not be negative", file=sys.stderr)
        return 1
    with open(a.sourceBasename + ".properties") as f:
        cls = [l.split("=", 1)[1].strip() for l in f if l.split("=", 1)[0].strip() == "graphclass"]
    if cls and cls[-1].replace("class ", "").endswith(".EFGraph"):
        src = EFGraph.load(a.sourceBasename, a.device, _abi.LOAD_OFFLINE)
        n = src.num_nodes()
        deg, succ = src.decode_range(0, n)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum(deg.astype(np.int64), dtype=np.uint64)
        write_efgraph(a.destBasename, (off, succ), None, a.log2_quantum, "LITTLE_ENDIAN" if sys.byteorder == "little" else "BIG_ENDIAN", a.device)
        src.close()
    else:
        src = BVGraph.load(a.sourceBasename, a.device, _abi.LOAD_OFFLINE)
        bvgraph_to_efgraph(src, None, a.log2_quantum, "LITTLE_ENDIAN" if sys.byteorder == "little" else "BIG_ENDIAN", a.device, basename=a.destBasename).close()
        src.close()
    return 0
