"""Text graphs over the C ABI (include/bvgraph_hip.h, bvg_text_*): ASCIIGraph (basename.graph-txt) and arc lists, read into a CSR
that stays on the device and written from a BVGraph, an EFGraph or an adjacency; arc lists of arbitrary numeric identifiers
(bvg_scattered_*: ScatteredArcsASCIIGraph); BVGraph.store to disk (write_bvgraph); and the command lines of ASCIIGraph.main,
ArcListASCIIGraph.main, BVGraph.main (BVGraph.java:2613-2715) and ScatteredArcsASCIIGraph.main."""
import argparse
import ctypes as C
import gzip
import os
import sys

import numpy as np

from . import _abi
from ._abi import TextError
from .bvgraph import BVGraph, BVGraphError, IllegalArgumentException, UnsupportedOperationException, _EXC, _check, lib
from .efgraph import EFGraph, _csr, _format3

_RANGE_ITEMS = 1 << 26          # successors + nodes formatted per call by the file writers


def _text_fns():
    """The bvg_text_* entry points, bound on first use (a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_text_bound", False):
        return L
    for name, args in _abi.text_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_text_close.restype = None
    L._text_bound = True
    return L


def _bytes_of(data):
    if isinstance(data, str):
        data = data.encode("latin-1")
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)


def _check_text(status, err, what):
    """Raises the mapped exception of a refusal, carrying .line, .byte and .reason (a name of _abi.TEXT_REASONS; .reason_code the number)."""
    if status == 0:
        return
    if err.reason == 0:
        _check(status, what)
    reason = _abi.TEXT_REASONS.get(err.reason, str(err.reason))
    e = _EXC.get(status, BVGraphError)(status, "%s: %s at line %d, byte %d" % (what, reason.replace("_", " "), err.line, err.byte))
    e.line, e.byte, e.reason, e.reason_code = int(err.line), int(err.byte), reason, int(err.reason)
    raise e


class ParsedGraph:
    """A parsed text graph: its adjacency in CSR form, resident on the device (bvg_text)."""

    def __init__(self, handle, device=0):
        self._h, self._device = handle, device
        n, m = C.c_int64(), C.c_uint64()
        _check(_text_fns().bvg_text_info(self._h, C.byref(n), C.byref(m)), "text_info")
        self._n, self._m = int(n.value), int(m.value)

    def close(self):
        if getattr(self, "_h", None):
            _text_fns().bvg_text_close(self._h)
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
        """(adj_off uint64[n + 1], adj int64[m])."""
        off = np.empty(self._n + 1, dtype=np.uint64); adj = np.empty(self._m, dtype=np.int64)
        _check(_text_fns().bvg_text_get(self._h, off.ctypes.data, len(off), adj.ctypes.data if self._m else None, self._m), "text_get")
        return off, adj

    def csr_dev(self, off_ptr, off_cap, adj_ptr, adj_cap):
        """bvg_text_get_dev: into device buffers (capacities in elements)."""
        _check(_text_fns().bvg_text_get_dev(self._h, off_ptr, off_cap, adj_ptr, adj_cap), "text_get_dev")

    def store(self, params=None, chunk_nodes=0):
        """BVGraph.store of the resident CSR (bvg_text_store): (graph uint8[], offsets uint64[n + 1]), the bytes of bvg_store."""
        p = params if params is not None else _abi.default_params()
        g = C.c_void_p(); o = C.c_void_p(); nb = C.c_uint64()
        L = _text_fns()
        _check(L.bvg_text_store(self._h, C.byref(p), chunk_nodes, C.byref(g), C.byref(nb), C.byref(o)), "text_store")
        try:
            graph = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=(max(int(nb.value), 1),))[:int(nb.value)].copy()
            offsets = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(self._n + 1,)).copy()
        finally:
            L.bvg_free(g); L.bvg_free(o)
        return graph, offsets

    def to_ascii_graph(self, basename, range_items=None):
        off, adj = self.csr()
        return _write_csr_text(basename + ".graph-txt", _abi.TEXT_ASCII, off, adj, 0, header=True, range_items=range_items)

    def to_arc_list(self, path, shift=0, range_items=None):
        off, adj = self.csr()
        return _write_csr_text(path, _abi.TEXT_ARCS, off, adj, shift, header=False, range_items=range_items)


def parse_ascii_graph(data, device=0):
    """ASCIIGraph text (the node count, then one line of successors per node) -> ParsedGraph."""
    b = _bytes_of(data)
    h = C.c_void_p(); err = TextError()
    st = _text_fns().bvg_text_parse_ascii(b.ctypes.data if len(b) else None, len(b), device, C.byref(h), C.byref(err))
    _check_text(st, err, "parse_ascii_graph")
    return ParsedGraph(h, device)


def _arc_flags(symmetrize, no_loops):
    return (_abi.TEXT_SYMMETRIZE_FLAG if symmetrize else 0) | (_abi.TEXT_NO_LOOPS_FLAG if no_loops else 0)


def parse_arc_list(data, shift=0, symmetrize=False, no_loops=False, min_nodes=0, device=0):
    """`source TAB target` lines, sources in any order -> ParsedGraph (duplicates once; nodes = max(largest id + 1, min_nodes))."""
    b = _bytes_of(data)
    h = C.c_void_p(); err = TextError()
    st = _text_fns().bvg_text_parse_arcs(b.ctypes.data if len(b) else None, len(b), shift, _arc_flags(symmetrize, no_loops), min_nodes, device, C.byref(h), C.byref(err))
    _check_text(st, err, "parse_arc_list")
    return ParsedGraph(h, device)


def parse_ascii_graph_dev(ptr, nbytes, device=0):
    h = C.c_void_p(); err = TextError()
    _check_text(_text_fns().bvg_text_parse_ascii_dev(ptr, nbytes, device, C.byref(h), C.byref(err)), err, "parse_ascii_graph_dev")
    return ParsedGraph(h, device)


def parse_arc_list_dev(ptr, nbytes, shift=0, symmetrize=False, no_loops=False, min_nodes=0, device=0):
    h = C.c_void_p(); err = TextError()
    _check_text(_text_fns().bvg_text_parse_arcs_dev(ptr, nbytes, shift, _arc_flags(symmetrize, no_loops), min_nodes, device, C.byref(h), C.byref(err)), err, "parse_arc_list_dev")
    return ParsedGraph(h, device)


def _read(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        return f.read()


def load_ascii_graph(basename, device=0):
    """ASCIIGraph.load(basename): reads basename.graph-txt (or basename.graph-txt.gz, or the path itself when it names a file; a path
    ending in .gz goes through gzip)."""
    for path in (basename + ".graph-txt", basename + ".graph-txt.gz", basename):
        if os.path.isfile(path):
            return parse_ascii_graph(_read(path), device)
    raise _EXC[_abi.E_IO](_abi.E_IO, "load_ascii_graph(%s)" % basename)


def load_arc_list(path, shift=0, symmetrize=False, no_loops=False, min_nodes=0, device=0):
    if not os.path.isfile(path):
        raise _EXC[_abi.E_IO](_abi.E_IO, "load_arc_list(%s)" % path)
    return parse_arc_list(_read(path), shift, symmetrize, no_loops, min_nodes, device)


# ---- scattered arc lists: identifiers that are not node numbers (bvg_scattered_*)

def _scattered_fns():
    """The bvg_scattered_* entry points, bound on first use."""
    L = _text_fns()
    if getattr(L, "_scattered_bound", False):
        return L
    for name, args in _abi.scattered_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._scattered_bound = True
    return L


class ScatteredGraph(ParsedGraph):
    """A parsed scattered arc list: a ParsedGraph (store(), the transforms and compose take it) with .ids, int64[nodes], the identifier of
    every node, and .report, what the parser saw (a dict of bvg_scattered_report's fields; first_reason a name of _abi.SCATTERED_REASONS
    or None)."""

    def __init__(self, handle, report, device=0):
        ParsedGraph.__init__(self, handle, device)
        self.report = report.as_dict()
        self._ids = None

    @property
    def ids(self):
        if self._ids is None:
            ids = np.empty(self._n, dtype=np.int64)
            _check(_scattered_fns().bvg_scattered_ids(self._h, ids.ctypes.data if self._n else None, self._n), "scattered_ids")
            self._ids = ids
        return self._ids

    def ids_dev(self, ptr, cap):
        """bvg_scattered_ids_dev: into a device buffer (capacity in elements)."""
        _check(_scattered_fns().bvg_scattered_ids_dev(self._h, ptr, cap), "scattered_ids_dev")


def _check_scattered(status, err, rep, what):
    """As _check_text, the reason being a name of _abi.SCATTERED_REASONS; the exception carries .report as well."""
    if status == 0:
        return
    if err.reason == 0:
        _check(status, what)
    reason = _abi.SCATTERED_REASONS.get(err.reason, str(err.reason))
    e = _EXC.get(status, BVGraphError)(status, "%s: %s at line %d, byte %d" % (what, reason.replace("_", " "), err.line, err.byte))
    e.line, e.byte, e.reason, e.reason_code, e.report = int(err.line), int(err.byte), reason, int(err.reason), rep.as_dict()
    raise e


def _scattered_flags(symmetrize, no_loops, strict):
    return _arc_flags(symmetrize, no_loops) | (_abi.TEXT_STRICT_FLAG if strict else 0)


def parse_scattered_arcs(data, symmetrize=False, no_loops=False, ids=None, strict=False, device=0):
    """`source target` lines whose identifiers are any integers of [-2^63, 2^63) -> ScatteredGraph: every newly seen identifier gets the next
    node number, offending lines are counted and skipped (strict=True: refused).  ids: a numbering given in advance (node i has identifier
    ids[i]); lines that mention other identifiers are skipped."""
    b = _bytes_of(data)
    known = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
    h = C.c_void_p(); err = TextError(); rep = _abi.ScatteredReport()
    pad = np.zeros(1, dtype=np.int64)                                       # (a pointer that is not NULL for an empty numbering)
    st = _scattered_fns().bvg_scattered_parse(b.ctypes.data if len(b) else None, len(b), _scattered_flags(symmetrize, no_loops, strict),
                                              None if known is None else (known.ctypes.data if len(known) else pad.ctypes.data), 0 if known is None else len(known),
                                              device, C.byref(h), C.byref(rep), C.byref(err))
    _check_scattered(st, err, rep, "parse_scattered_arcs")
    return ScatteredGraph(h, rep, device)


def parse_scattered_arcs_dev(ptr, nbytes, symmetrize=False, no_loops=False, ids_ptr=None, n_ids=0, strict=False, device=0):
    """The text, and the given numbering if any, in device memory."""
    h = C.c_void_p(); err = TextError(); rep = _abi.ScatteredReport()
    st = _scattered_fns().bvg_scattered_parse_dev(ptr, nbytes, _scattered_flags(symmetrize, no_loops, strict), ids_ptr, n_ids, device, C.byref(h), C.byref(rep), C.byref(err))
    _check_scattered(st, err, rep, "parse_scattered_arcs_dev")
    return ScatteredGraph(h, rep, device)


def load_scattered_arcs(path, symmetrize=False, no_loops=False, ids=None, strict=False, device=0):
    if not os.path.isfile(path):
        raise _EXC[_abi.E_IO](_abi.E_IO, "load_scattered_arcs(%s)" % path)
    return parse_scattered_arcs(_read(path), symmetrize, no_loops, ids, strict, device)


def _sized_text(call, what):
    """The capacity contract of the format calls: a sizing call, then the call that writes."""
    need = C.c_uint64(0)
    st = call(None, 0, C.byref(need))
    if st == 0:
        return b""
    if st != _abi.E_CAPACITY:
        _check(st, what)
    out = np.empty(int(need.value), dtype=np.uint8)
    _check(call(out.ctypes.data, len(out), C.byref(need)), what)
    return out.tobytes()


def format_csr(kind, first_node, adj_off, adj, shift=0):
    """bvg_text_format_csr: the text of an adjacency in host memory (kind: _abi.TEXT_ASCII / TEXT_ARCS; node x of it is first_node + x)."""
    off = np.ascontiguousarray(adj_off, dtype=np.uint64); a = np.ascontiguousarray(adj, dtype=np.int64)
    L = _text_fns()
    return _sized_text(lambda o, cap, need: L.bvg_text_format_csr(kind, first_node, len(off) - 1, off.ctypes.data, a.ctypes.data if len(a) else None, shift, o, cap, need), "format_csr")


def _format_ascii_range(self, frm, to):
    """The lines of nodes [frm, to) as ASCIIGraph.store writes them (every successor followed by one space)."""
    L = _text_fns()
    return _sized_text(lambda o, cap, need: L.bvg_text_format_ascii(self._h, frm, to, o, cap, need), "format_ascii(%d,%d)" % (frm, to))


def _format_arcs_range(self, frm, to, shift=0):
    """One `source TAB target` line per arc of nodes [frm, to)."""
    L = _text_fns()
    return _sized_text(lambda o, cap, need: L.bvg_text_format_arcs(self._h, frm, to, shift, o, cap, need), "format_arcs(%d,%d)" % (frm, to))


def _ranges(self, k):
    n = self.num_nodes()
    if n == 0:
        return []
    if k is None:
        try:
            arcs = self.num_arcs()
        except UnsupportedOperationException:
            arcs = int(self.outdegrees(0, n).astype(np.int64).sum())
        k = max(1, -(-(arcs + n) // _RANGE_ITEMS))
    b = [int(x) for x in self.split_by_arcs(min(k, n))]
    return [(b[i], b[i + 1]) for i in range(len(b) - 1) if b[i] < b[i + 1]]


def _bv_to_ascii_graph(self, basename, ranges=None):
    """ASCIIGraph.store(graph, basename): basename.graph-txt, written range after range (bvg_split_by_arcs; `ranges` = how many)."""
    path = basename + ".graph-txt"
    with open(path, "wb") as f:
        f.write(b"%d\n" % self.num_nodes())
        for lo, hi in _ranges(self, ranges):
            f.write(_format_ascii_range(self, lo, hi))
    return path


def _bv_to_arc_list(self, path, shift=0, ranges=None):
    """ArcListASCIIGraph.store(graph, path, shift)."""
    with open(path, "wb") as f:
        for lo, hi in _ranges(self, ranges):
            f.write(_format_arcs_range(self, lo, hi, shift))
    return path


BVGraph.format_ascii, BVGraph.format_arcs = _format_ascii_range, _format_arcs_range
BVGraph.to_ascii_graph, BVGraph.to_arc_list = _bv_to_ascii_graph, _bv_to_arc_list


def _write_csr_text(path, kind, off, adj, shift, header, first_node=0, mode="wb", range_items=None):
    """An adjacency in host memory, in node ranges of at most range_items (default _RANGE_ITEMS) successors + nodes; the output does
    not depend on the ranges."""
    off = np.ascontiguousarray(off, dtype=np.uint64); adj = np.ascontiguousarray(adj, dtype=np.int64)
    n = len(off) - 1
    per = _RANGE_ITEMS if range_items is None else max(1, int(range_items))
    with open(path, mode) as f:
        if header:
            f.write(b"%d\n" % n)
        lo = 0
        while lo < n:
            key = off[lo:].astype(np.int64) - int(off[lo]) + np.arange(n - lo + 1)       # successors + nodes before every node of the rest
            hi = lo + max(1, int(np.searchsorted(key, per, side="right")) - 1)
            hi = min(hi, n)
            f.write(format_csr(kind, first_node + lo, off[lo:hi + 1] - off[lo], adj[int(off[lo]):int(off[hi])], shift))   # the slice, and offsets into the slice
            lo = hi
    return path


def _ef_batches(self, per=None):
    per = _RANGE_ITEMS if per is None else max(1, int(per))
    n = self.num_nodes()
    cum = np.concatenate([[0], np.cumsum(self.outdegrees(0, n).astype(np.int64))]) + np.arange(n + 1) if n else np.zeros(1, np.int64)
    lo = 0
    while lo < n:
        hi = min(n, lo + max(1, int(np.searchsorted(cum, cum[lo] + per, side="right")) - 1 - lo))
        yield lo, hi
        lo = hi


def _ef_to_ascii_graph(self, basename, range_items=None):
    path = basename + ".graph-txt"
    with open(path, "wb") as f:
        f.write(b"%d\n" % self.num_nodes())
        for lo, hi in _ef_batches(self, range_items):
            deg, succ = self.decode_range(lo, hi)
            f.write(format_csr(_abi.TEXT_ASCII, lo, np.concatenate([[0], np.cumsum(deg.astype(np.int64))]).astype(np.uint64), succ))
    return path


def _ef_to_arc_list(self, path, shift=0, range_items=None):
    with open(path, "wb") as f:
        for lo, hi in _ef_batches(self, range_items):
            deg, succ = self.decode_range(lo, hi)
            f.write(format_csr(_abi.TEXT_ARCS, lo, np.concatenate([[0], np.cumsum(deg.astype(np.int64))]).astype(np.uint64), succ, shift))
    return path


EFGraph.to_ascii_graph, EFGraph.to_arc_list = _ef_to_ascii_graph, _ef_to_arc_list


# ---- BVGraph.store to disk

def _put_fields(bits, ends, values, widths):
    """Sets, MSB first, the `widths` low bits of `values` so that each field ends just before bit position `ends`."""
    for j in range(int(widths.max()) if len(widths) else 0):
        sel = (widths > j) & ((values >> np.uint64(j)) & np.uint64(1)).astype(bool)
        bits[ends[sel] - 1 - j] = 1


def coded_gaps(offsets, coding=_abi.GAMMA):
    """The bytes of basename.offsets (BVGraph.java:2228, :2311): the n + 1 gaps of the bit offsets, the first being offsets[0], gamma or
    delta coded, MSB first."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = bytearray()
    carry = np.zeros(0, dtype=np.uint8)
    step = 1 << 20
    for lo in range(0, len(off), step):
        part = off[lo:lo + step]
        prev = np.concatenate([[off[lo - 1] if lo else np.uint64(0)], part[:-1]]).astype(np.uint64)
        v = part - prev + np.uint64(1)                                   # gamma(x): msb(x + 1) zeros, then x + 1 in msb + 1 bits
        m = np.floor(np.log2(v.astype(np.float64))).astype(np.int64)
        m += ((v >> m.astype(np.uint64)) > 1).astype(np.int64) - ((v >> m.astype(np.uint64)) < 1).astype(np.int64)   # (float rounding near powers of two)
        if coding == _abi.GAMMA:
            w = 2 * m + 1
            ends = np.cumsum(w)
            bits = np.zeros(int(ends[-1]), dtype=np.uint8)
            _put_fields(bits, ends, v, m + 1)
        elif coding == _abi.DELTA:                                       # delta(x): gamma(msb(x + 1)), then the low msb bits of x + 1
            g = (m + 1).astype(np.uint64)
            mm = np.floor(np.log2(g.astype(np.float64))).astype(np.int64)
            w = 2 * mm + 1 + m
            ends = np.cumsum(w)
            bits = np.zeros(int(ends[-1]), dtype=np.uint8)
            _put_fields(bits, ends - m, g, mm + 1)
            _put_fields(bits, ends, v & ((np.uint64(1) << m.astype(np.uint64)) - np.uint64(1)), m)
        else:
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, "offsets coding %r" % (coding,))
        bits = np.concatenate([carry, bits])
        whole = len(bits) // 8 * 8
        out += np.packbits(bits[:whole]).tobytes()
        carry = bits[whole:]
    if len(carry):
        out += np.packbits(carry).tobytes()
    return bytes(out)


_CODING_NAMES = {_abi.DELTA: "DELTA", _abi.GAMMA: "GAMMA", _abi.GOLOMB: "GOLOMB", _abi.SKEWED_GOLOMB: "SKEWED_GOLOMB", _abi.UNARY: "UNARY", _abi.ZETA: "ZETA", _abi.NIBBLE: "NIBBLE"}
_FLAG_FIELDS = (("outdegree_coding", "OUTDEGREES_"), ("block_coding", "BLOCKS_"), ("residual_coding", "RESIDUALS_"), ("reference_coding", "REFERENCES_"),
                ("block_count_coding", "BLOCK_COUNT_"), ("offset_coding", "OFFSETS_"))


def properties_text(params, nodes, arcs, graph_bits):
    """basename.properties with the keys BVGraph.loadInternal reads (BVGraph.java:1479-1503) and the two ratios the reference adds."""
    d = _abi.default_params()
    flags = [prefix + _CODING_NAMES[getattr(params, f)] for f, prefix in _FLAG_FIELDS if getattr(params, f) != getattr(d, f)]
    return ("#BVGraph properties\nbitsperlink=%s\nbitspernode=%s\ngraphclass=it.unimi.dsi.big.webgraph.BVGraph\nversion=0\nnodes=%d\narcs=%d\n"
            "windowsize=%d\nmaxrefcount=%d\nminintervallength=%d\nzetak=%d\ncompressionflags=%s\n"
            % (_format3(graph_bits / arcs) if arcs else "NaN", _format3(graph_bits / nodes) if nodes else "NaN", nodes, arcs,
               params.window_size, params.max_ref_count, params.min_interval_length, params.zeta_k, " | ".join(flags)))


def write_bvgraph(basename, adj_or_parsed, params=None, chunk_nodes=0, device=0):
    """BVGraph.store(graph, basename, ...): compresses on the device and writes basename.graph, .offsets and .properties; the result opens
    with BVGraph.load.  adj_or_parsed: a ParsedGraph (its resident CSR is compressed where it is), (adj_off, adj), or a list of sorted lists."""
    p = params if params is not None else _abi.default_params()
    if isinstance(adj_or_parsed, ParsedGraph):
        n, m = adj_or_parsed.num_nodes(), adj_or_parsed.num_arcs()
        graph, offsets = adj_or_parsed.store(p, chunk_nodes)
    else:
        from .bvgraph import store
        off, succ = _csr(adj_or_parsed)
        n, m = len(off) - 1, int(off[-1])
        graph, offsets = store((off, succ), p, chunk_nodes, device)
    with open(basename + ".graph", "wb") as f:
        f.write(graph.tobytes())
    with open(basename + ".offsets", "wb") as f:
        f.write(coded_gaps(offsets, p.offset_coding))
    with open(basename + ".properties", "w") as f:
        f.write(properties_text(p, n, m, int(offsets[-1])))
    return graph, offsets


# ---- command lines

_CLASSES = ("BVGraph", "EFGraph", "ASCIIGraph", "ArcListASCIIGraph")


def _class_name(name):
    short = name.rsplit(".", 1)[-1]
    if short not in _CLASSES:
        raise SystemExit("unknown graph class %r: one of %s" % (name, ", ".join(_CLASSES)))
    return short


def _open_source(cls, source, device, shift=0):
    if cls == "BVGraph":
        return BVGraph.load(source, device, _abi.LOAD_OFFLINE)
    if cls == "EFGraph":
        return EFGraph.load(source, device, _abi.LOAD_OFFLINE)
    if cls == "ASCIIGraph":
        return load_ascii_graph(source, device)
    return load_arc_list(source, shift, device=device)


def _parse(ap, argv, prog):
    a, rest = ap.parse_known_args(argv)
    if rest:
        print("%s: option(s) not supported here: %s" % (prog, " ".join(rest)), file=sys.stderr)
        return None
    return a


def asciigraph_arg_parser():
    ap = argparse.ArgumentParser(prog="asciigraph_main", description="Writes a graph as basename.graph-txt (ASCIIGraph.main).")
    ap.add_argument("-g", "--graph-class", dest="graph_class", default="BVGraph", help="The class of the source graph: " + ", ".join(_CLASSES) + ".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("sourceBasename")
    ap.add_argument("destBasename")
    return ap


def asciigraph_main(argv=None):
    """ASCIIGraph.main: [-g CLASS] source dest."""
    a = _parse(asciigraph_arg_parser(), argv, "asciigraph_main")
    if a is None:
        return 1
    src = _open_source(_class_name(a.graph_class), a.sourceBasename, a.device)
    try:
        src.to_ascii_graph(a.destBasename)
    finally:
        src.close()
    return 0


def arclist_arg_parser():
    ap = argparse.ArgumentParser(prog="arclist_main", description="Writes a graph as a list of arcs, one `source TAB target` line each (ArcListASCIIGraph.main).")
    ap.add_argument("-g", "--graph-class", dest="graph_class", default="BVGraph", help="The class of the source graph: " + ", ".join(_CLASSES) + ".")
    ap.add_argument("-S", "--shift", type=int, default=0, help="A shift added to every node index.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("sourceBasename")
    ap.add_argument("dest")
    return ap


def arclist_main(argv=None):
    """ArcListASCIIGraph.main: [-g CLASS] [-S shift] source dest."""
    a = _parse(arclist_arg_parser(), argv, "arclist_main")
    if a is None:
        return 1
    src = _open_source(_class_name(a.graph_class), a.sourceBasename, a.device)
    try:
        src.to_arc_list(a.dest, a.shift)
    finally:
        src.close()
    return 0


def bvgraph_arg_parser():
    ap = argparse.ArgumentParser(prog="bvgraph_main", description="Compresses a graph as a BVGraph (BVGraph.main, BVGraph.java:2613-2715): the option letters of the reference.")
    ap.add_argument("-g", "--graph-class", dest="graph_class", default="BVGraph", help="The class of the source graph: " + ", ".join(_CLASSES) + ".")
    ap.add_argument("-w", "--window-size", dest="window_size", type=int, default=7)
    ap.add_argument("-m", "--max-ref-count", dest="max_ref_count", type=int, default=3)
    ap.add_argument("-i", "--min-interval-length", dest="min_interval_length", type=int, default=4)
    ap.add_argument("-k", "--zeta-k", dest="zeta_k", type=int, default=3)
    ap.add_argument("-c", "--comp", dest="comp", action="append", default=[], help="A compression flag (may be specified several times), e.g. RESIDUALS_GAMMA.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("sourceBasename")
    ap.add_argument("destBasename")
    return ap


def bvgraph_main(argv=None):
    """BVGraph.main: [-g CLASS] [-w W] [-m M] [-i I] [-k K] [-c FLAG]... source dest.  The reference's other options (-o, -O, -L, -F, ...)
    are refused with a message."""
    a = _parse(bvgraph_arg_parser(), argv, "bvgraph_main")
    if a is None:
        return 1
    p = _abi.default_params(window_size=a.window_size, max_ref_count=a.max_ref_count, min_interval_length=a.min_interval_length, zeta_k=a.zeta_k)
    names = {v: k for k, v in _CODING_NAMES.items()}
    for flag in a.comp:
        for f, prefix in _FLAG_FIELDS:
            if flag.startswith(prefix) and flag[len(prefix):] in names:
                setattr(p, f, names[flag[len(prefix):]])
                break
        else:
            print("bvgraph_main: unknown compression flag %r" % flag, file=sys.stderr)
            return 1
    cls = _class_name(a.graph_class)
    src = _open_source(cls, a.sourceBasename, a.device)
    try:
        if isinstance(src, ParsedGraph):
            write_bvgraph(a.destBasename, src, p, 0, a.device)
        else:
            n = src.num_nodes()
            deg = src.outdegrees(0, n).astype(np.int64) if n else np.empty(0, np.int64)
            off = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
            succ = np.empty(int(off[-1]), dtype=np.int64)
            for lo, hi in (_ranges(src, None) if cls == "BVGraph" else _ef_batches(src)):
                succ[int(off[lo]):int(off[hi])] = src.decode_range(lo, hi)[1]
            write_bvgraph(a.destBasename, (off, succ), p, 0, a.device)
    finally:
        src.close()
    return 0


def scattered_arg_parser():
    ap = argparse.ArgumentParser(prog="scattered_main", description="Reads a list of arcs whose identifiers are arbitrary integers from standard input (or --input) and "
                                 "compresses it as a BVGraph; writes basename.ids, the identifier of every node (ScatteredArcsASCIIGraph.main: its option letters).")
    ap.add_argument("-S", "--symmetrize", action="store_true", help="Force the output graph to be symmetric.")
    ap.add_argument("-L", "--no-loops", dest="no_loops", action="store_true", help="Remove loops from the output graph.")
    ap.add_argument("-z", "--zipped", action="store_true", help="The list of arcs is compressed in gzip format.")
    ap.add_argument("-w", "--window-size", dest="window_size", type=int, default=7)
    ap.add_argument("-m", "--max-ref-count", dest="max_ref_count", type=int, default=3)
    ap.add_argument("-i", "--min-interval-length", dest="min_interval_length", type=int, default=4)
    ap.add_argument("-k", "--zeta-k", dest="zeta_k", type=int, default=3)
    ap.add_argument("-c", "--comp", dest="comp", action="append", default=[], help="A compression flag (may be specified several times), e.g. RESIDUALS_GAMMA.")
    ap.add_argument("--ids", help="A file of longs in BinIO format: node i has identifier ids[i] (lines that mention others are skipped; no basename.ids is written).")
    ap.add_argument("--strict", action="store_true", help="Refuse the input at its first offending line.")
    ap.add_argument("--input", help="Read the arcs from this file in place of standard input (a name ending in .gz goes through gzip).")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("basename")
    return ap


def scattered_main(argv=None):
    """ScatteredArcsASCIIGraph.main: [-S] [-L] [-z] [-w W] [-m M] [-i I] [-k K] [-c FLAG]... [--ids FILE] [--input FILE] basename.  The
    translation function of the reference (-f, -b, -C, -n) is for string identifiers, which are not built: refused with a message, as its
    other options are.  The counts of the report go to standard error, where the reference logs."""
    argv = sys.argv[1:] if argv is None else list(argv)
    for opt in ("-f", "--function", "-b", "--byte-array", "-C", "--charset", "-n", "--n"):
        if any(x == opt or (opt.startswith("--") and x.startswith(opt + "=")) for x in argv):
            print("scattered_main: %s belongs to the translation function for string identifiers, which is not supported here (numeric identifiers: --ids FILE)" % opt, file=sys.stderr)
            return 1
    a = _parse(scattered_arg_parser(), argv, "scattered_main")
    if a is None:
        return 1
    p = _abi.default_params(window_size=a.window_size, max_ref_count=a.max_ref_count, min_interval_length=a.min_interval_length, zeta_k=a.zeta_k)
    names = {v: k for k, v in _CODING_NAMES.items()}
    for flag in a.comp:
        for f, prefix in _FLAG_FIELDS:
            if flag.startswith(prefix) and flag[len(prefix):] in names:
                setattr(p, f, names[flag[len(prefix):]])
                break
        else:
            print("scattered_main: unknown compression flag %r" % flag, file=sys.stderr)
            return 1
    if a.input is not None:
        if not os.path.isfile(a.input):
            raise _EXC[_abi.E_IO](_abi.E_IO, "scattered_main(%s)" % a.input)
        data = _read(a.input)
    else:
        data = sys.stdin.buffer.read()
    if a.zipped and not (a.input or "").endswith(".gz"):
        data = gzip.decompress(data)
    known = None
    if a.ids is not None:
        if not os.path.isfile(a.ids):
            raise _EXC[_abi.E_IO](_abi.E_IO, "scattered_main(%s)" % a.ids)
        known = np.fromfile(a.ids, dtype=">i8").astype(np.int64)            # (BinIO.loadLongs)
    g = parse_scattered_arcs(data, a.symmetrize, a.no_loops, known, a.strict, a.device)
    try:
        r = g.report
        print("scattered_main: %d lines, %d arcs kept, %d nodes, %d arcs in the graph" % (r["lines"], r["arcs"], g.num_nodes(), g.num_arcs()), file=sys.stderr)
        for k in ("bad_source", "bad_target", "no_target", "too_large", "trailing", "unknown_source", "unknown_target", "dropped_loops"):
            if r[k]:
                print("scattered_main: %s: %d lines" % (k.replace("_", " "), r[k]), file=sys.stderr)
        if r["first_reason"]:
            print("scattered_main: the first offending line is line %d (byte %d): %s" % (r["first_line"], r["first_byte"], r["first_reason"].replace("_", " ")), file=sys.stderr)
        write_bvgraph(a.basename, g, p, 0, a.device)
        if known is None:
            g.ids.astype(">i8").tofile(a.basename + ".ids")                # (BinIO.storeLongs)
    finally:
        g.close()
    return 0
