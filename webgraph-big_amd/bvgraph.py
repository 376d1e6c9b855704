"""Host-side mirror of the reference's graph API over the C ABI of libbvgraph_hip.so.

Class and method names follow the reference (paths relative to /root/reference/src/it/unimi/dsi/big/webgraph):
  ImmutableGraph.java:245-447   numNodes / numArcs / randomAccess / outdegree / successors /
                                successorBigArray / nodeIterator / splitNodeIterators / copy
  NodeIterator.java:34-133      hasNext / nextLong / outdegree / successors / successorBigArray / copy(upperBound) / skip
  LazyLongIterator.java:28-44   nextLong() returns -1 at the end; skip(n)
  BVGraph.java:1345-1464        load / loadMapped / loadOffline / loadSequential

Every decode goes through the HIP kernels (bvg_decode_range / bvg_scan); there is no CPU decode in
this package and importing it on a box without the built library or without a GPU fails loudly at
the first call that needs the device.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from . import _abi
from ._abi import Params, ScanResult, Tuning

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class BVGraphError(Exception):
    """Base of the status-code exceptions; subclasses mirror the Java exception classes."""

    def __init__(self, status, what=""):
        self.status = status
        msg = lib().bvg_strerror(status).decode() if _LIB is not None else str(status)
        super().__init__("%s [%d] %s" % (what, status, msg))


class IllegalArgumentException(BVGraphError, ValueError):
    pass


class IllegalStateException(BVGraphError, RuntimeError):
    pass


class UnsupportedOperationException(BVGraphError, NotImplementedError):
    pass


class IOException(BVGraphError, OSError):
    pass


class EOFException(IOException):
    pass


class DeviceError(BVGraphError):
    pass


class NoSuchElementException(StopIteration):
    pass


_EXC = {_abi.E_ARG: IllegalArgumentException, _abi.E_STATE: IllegalStateException, _abi.E_UNSUPPORTED: UnsupportedOperationException,
        _abi.E_IO: IOException, _abi.E_EOF: EOFException, _abi.E_NOMEM: MemoryError, _abi.E_HIP: DeviceError}


def _check(status, what=""):
    if status == 0:
        return
    exc = _EXC.get(status, BVGraphError)
    if exc is MemoryError:
        raise MemoryError("%s: out of host/device memory" % what)
    raise exc(status, what)


def library_path():
    # BVG_HIP_LIB: an alternative build of the same library (e.g. lib/libbvgraph_hip_prof.so, `make prof`: cycle timers compiled in)
    return os.environ.get("BVG_HIP_LIB") or os.path.join(_HERE, "lib", "libbvgraph_hip.so")


def build(force=False):
    """Compiles libbvgraph_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    so = library_path()
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))] + [os.path.join(_HERE, "..", "include", "bvgraph_hip.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", _HERE, "lib/libbvgraph_hip.so"])
    return so


def lib():
    """Loads the HIP library; raises if it is missing (no fallback)."""
    global _LIB
    if _LIB is None:
        so = library_path()
        if not os.path.exists(so):
            raise ImportError("libbvgraph_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        L = C.CDLL(so)
        vp, i64, u64, pp = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p)
        L.bvg_abi_version.restype = C.c_int
        L.bvg_default_params.argtypes = [C.POINTER(Params)]
        L.bvg_parse_properties.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Params)]
        L.bvg_decode_offsets.argtypes = [vp, C.c_size_t, i64, C.c_int, vp]
        L.bvg_open.argtypes = [C.c_char_p, C.c_int, C.c_int, pp]
        L.bvg_open_mem.argtypes = [C.POINTER(Params), vp, u64, vp, C.c_int, pp]
        L.bvg_open_dev.argtypes = [C.POINTER(Params), vp, u64, vp, C.c_int, pp]
        L.bvg_copy.argtypes = [vp, pp]
        L.bvg_close.argtypes = [vp]; L.bvg_close.restype = None
        L.bvg_info.argtypes = [vp, C.POINTER(Params)]
        L.bvg_set_node_base.argtypes = [vp, u64]
        L.bvg_get_offsets.argtypes = [vp, vp]
        L.bvg_outdegrees.argtypes = [vp, i64, i64, vp]
        L.bvg_decode_range.argtypes = [vp, i64, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_decode_range_dev.argtypes = [vp, i64, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_decode_range32.argtypes = [vp, i64, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_scan.argtypes = [vp, i64, i64, C.POINTER(ScanResult)]
        L.bvg_successors_batch.argtypes = [vp, vp, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_host_alloc.argtypes = [C.c_size_t]; L.bvg_host_alloc.restype = vp
        L.bvg_store.argtypes = [C.POINTER(Params), i64, vp, vp, i64, C.c_int, pp, C.POINTER(u64), pp]
        L.bvg_free.argtypes = [vp]; L.bvg_free.restype = None
        L.bvg_host_free.argtypes = [vp]; L.bvg_host_free.restype = None
        L.bvg_split_by_bits.argtypes = [vp, C.c_int, vp]
        L.bvg_split_by_arcs.argtypes = [vp, C.c_int, vp]
        L.bvg_shard_bounds.argtypes = [vp, C.c_int, C.c_int, vp]
        L.bvg_scan_shard.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(ScanResult), C.POINTER(i64), C.POINTER(i64)]
        L.bvg_scan_multi.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ScanResult), vp]
        L.bvg_transpose.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_transpose_dev.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_symmetrize.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_symmetrize_dev.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_labels_parse_spec.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.bvg_labels_read_properties.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.bvg_labels_open_mem.argtypes = [C.c_int, C.c_int, i64, vp, u64, vp, C.c_int, pp]
        L.bvg_labels_open.argtypes = [C.c_char_p, i64, C.c_int, pp, C.c_char_p, C.c_size_t]
        L.bvg_labels_close.argtypes = [vp]; L.bvg_labels_close.restype = None
        L.bvg_labels_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(u64)]
        L.bvg_labels_decode_range.argtypes = [vp, i64, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_labels_decode_range_dev.argtypes = [vp, i64, i64, vp, vp, u64, C.POINTER(u64)]
        L.bvg_labels_decode_range_lists.argtypes = [vp, i64, i64, vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_labels_decode_range_lists64.argtypes = [vp, i64, i64, vp, vp, vp, u64, C.POINTER(u64)]
        L.bvg_tile.argtypes = [vp, i64, pp]
        L.bvg_mosaic.argtypes = [vp, C.c_int, i64, pp]
        L.bvg_set_tuning.argtypes = [vp, C.POINTER(Tuning)]
        L.bvg_strerror.argtypes = [C.c_int]; L.bvg_strerror.restype = C.c_char_p
        L.bvg_arc_mix.argtypes = [u64, u64]; L.bvg_arc_mix.restype = u64
        L.bvg_build_index.argtypes = [vp, i64, i64, C.POINTER(u64), C.POINTER(u64)]
        L.bvg_save_index.argtypes = [vp, C.c_char_p]
        L.bvg_load_index.argtypes = [vp, C.c_char_p]
        if L.bvg_abi_version() != 4:
            raise ImportError("libbvgraph_hip.so ABI mismatch")
        _LIB = L
    return _LIB


def _components_fns():
    """bvg_components / bvg_components_dev, bound on first use: a build of the library without them (the host emulator's) still loads."""
    L = lib()
    if getattr(L, "_cc_bound", False):
        return L
    vp, u64 = C.c_void_p, C.c_uint64
    for name in ("bvg_components", "bvg_components_dev"):
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = [vp, C.c_uint32, vp, vp, u64, C.POINTER(u64)]
    L._cc_bound = True
    return L


def _bfs_fns():
    """The bvg_bfs_* entry points, bound on first use (as _components_fns: a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_bfs_bound", False):
        return L
    sigs = _abi.bfs_signatures()
    for name, args in sigs.items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_bfs_close.restype = None
    L._bfs_bound = True
    return L


def _scc_fns():
    """bvg_scc / bvg_scc_dev, bound on first use (as _components_fns)."""
    L = lib()
    if getattr(L, "_scc_bound", False):
        return L
    for name, args in _abi.scc_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._scc_bound = True
    return L


def _geometric_fns():
    """bvg_geometric / bvg_geometric_dev, bound on first use (as _components_fns)."""
    L = lib()
    if getattr(L, "_geo_bound", False):
        return L
    for name, args in _abi.geometric_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L._geo_bound = True
    return L


def _stats_fns():
    """The bvg_stats_* entry points, bound on first use (as _components_fns: a build of the library without them still loads)."""
    L = lib()
    if getattr(L, "_stats_bound", False):
        return L
    for name, args in _abi.stats_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_stats_close.restype = None
    L._stats_bound = True
    return L


def _geometric_coeffs(coeffs):
    """(kind, param, table or None) of what linear_geometric_centrality takes: "harmonic", ("power", e), ("exp", b) or an array."""
    if isinstance(coeffs, str):
        if coeffs == "harmonic":
            return _abi.GEO_HARMONIC, 0.0, None
        raise IllegalArgumentException(_abi.E_ARG, "unknown coefficients %r" % (coeffs,))
    if isinstance(coeffs, tuple) and len(coeffs) == 2 and isinstance(coeffs[0], str):
        kind = {"power": _abi.GEO_POWER_LAW, "exp": _abi.GEO_EXPONENTIAL}.get(coeffs[0])
        if kind is None:
            raise IllegalArgumentException(_abi.E_ARG, "unknown coefficients %r" % (coeffs,))
        return kind, float(coeffs[1]), None
    table = np.ascontiguousarray(coeffs, dtype=np.float64)
    if table.ndim != 1 or len(table) == 0:
        raise IllegalArgumentException(_abi.E_ARG, "a coefficient table is a non-empty one-dimensional array")
    return _abi.GEO_TABLE, 0.0, table


def _hyperball_fns():
    """The bvg_hyperball_* entry points, bound on first use (as _bfs_fns)."""
    L = lib()
    if getattr(L, "_hb_bound", False):
        return L
    for name, args in _abi.hyperball_signatures().items():
        if not hasattr(L, name):
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, name + " is not in this build of the library")
        getattr(L, name).argtypes = args
    L.bvg_hyperball_close.restype = None
    L.bvg_hyperball_relative_standard_deviation.restype = C.c_double
    L._hb_bound = True
    return L


def store(adj, params=None, chunk_nodes=0, device=0):
    """BVGraph.store on the device (bvg_store): adj = (adj_off uint64[n+1], succ int64[m]) or a list of sorted lists.
    Returns (graph uint8[], offsets uint64[n+1]); byte for byte what the reference's compressor writes.
    UnsupportedOperationException for a window above 127; IllegalArgumentException for offsets that do not start at 0, decrease or pass
    adj_off[n], and for lists that are not strictly increasing or leave [0, n) (include/bvgraph_hip.h: bvg_store)."""
    if isinstance(adj, tuple):
        off = np.ascontiguousarray(adj[0], dtype=np.uint64); succ = np.ascontiguousarray(adj[1], dtype=np.int64)
    else:
        off = np.zeros(len(adj) + 1, dtype=np.uint64)
        if len(adj):
            off[1:] = np.cumsum([len(l) for l in adj], dtype=np.uint64)
        succ = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int64) for l in adj]) if len(adj) and off[-1] else np.empty(0, np.int64), dtype=np.int64)
    n = len(off) - 1
    p = params if params is not None else _abi.default_params()
    g = C.c_void_p(); o = C.c_void_p(); nb = C.c_uint64()
    sb = succ if len(succ) else np.zeros(1, np.int64)
    _check(lib().bvg_store(C.byref(p), n, off.ctypes.data, sb.ctypes.data, chunk_nodes, device, C.byref(g), C.byref(nb), C.byref(o)), "store")
    try:
        graph = np.ctypeslib.as_array(C.cast(g, C.POINTER(C.c_uint8)), shape=(max(int(nb.value), 1),))[:int(nb.value)].copy()
        offsets = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    finally:
        lib().bvg_free(g); lib().bvg_free(o)
    return graph, offsets


def parse_properties(text):
    if isinstance(text, str):
        text = text.encode()
    p = Params()
    _check(lib().bvg_parse_properties(text, len(text), C.byref(p)), "parse_properties")
    return p


def decode_offsets(obytes, nodes, coding=_abi.GAMMA):
    buf = np.frombuffer(bytes(obytes), dtype=np.uint8)
    out = np.empty(nodes + 1, dtype=np.uint64)
    _check(lib().bvg_decode_offsets(buf.ctypes.data if len(buf) else None, len(buf), nodes, coding, out.ctypes.data), "decode_offsets")
    return out


def arc_mix(x, y):
    return int(lib().bvg_arc_mix(x, y))


class LazyLongIterator:
    """LazyLongIterator.java:28-44 over a decoded successor array (LazyLongIterators.wrap, :220-255)."""

    def __init__(self, arr):
        self._a = arr
        self._i = 0

    def next_long(self):
        if self._i >= len(self._a):
            return -1
        v = int(self._a[self._i]); self._i += 1
        return v

    nextLong = next_long

    def skip(self, n):
        k = min(int(n), len(self._a) - self._i)
        self._i += k
        return k

    def __iter__(self):
        while True:
            v = self.next_long()
            if v == -1:
                return
            yield v


class PinnedArray:
    """A numpy view over page-locked host memory (bvg_host_alloc): device -> host copies into it run at the PCIe rate."""

    def __init__(self, count, dtype):
        self.dtype = np.dtype(dtype)
        self.nbytes = max(int(count), 1) * self.dtype.itemsize
        self._p = lib().bvg_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError("bvg_host_alloc(%d)" % self.nbytes)
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(self.nbytes,)).view(self.dtype)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            lib().bvg_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_PIN_CACHE = {}          # nbytes -> [PinnedArray]: page-locking memory costs ~0.3 s per GiB, so iterators hand their buffers on
_PIN_CACHE_LIMIT = 8 << 30
_pin_cached = 0
_PIN_LOCK = threading.Lock()   # iterators recycle buffers from their helper threads too


def _pinned(count, dtype):
    global _pin_cached
    nbytes = max(int(count), 1) * np.dtype(dtype).itemsize
    with _PIN_LOCK:
        lst = _PIN_CACHE.get(nbytes)
        pa = lst.pop() if lst else None
        if pa is not None:
            _pin_cached -= nbytes
    if pa is not None:
        pa.dtype = np.dtype(dtype)
        pa.array = np.ctypeslib.as_array(C.cast(pa._p, C.POINTER(C.c_uint8)), shape=(nbytes,)).view(pa.dtype)
        return pa
    return PinnedArray(count, dtype)


def _unpin(pa):
    """Hands a page-locked buffer back.  Views of it that a caller kept (successor_array(), batch()) are valid only until the
    iterator moves on (NodeIterator.java:80-96: "the returned array may be reused"): copy what must outlive that."""
    global _pin_cached
    if pa is None or not getattr(pa, "_p", None):
        return
    with _PIN_LOCK:
        keep = _pin_cached + pa.nbytes <= _PIN_CACHE_LIMIT
        if keep:
            _PIN_CACHE.setdefault(pa.nbytes, []).append(pa); _pin_cached += pa.nbytes
    if not keep:
        pa.close()


class _BatchSlot:
    """One of the two batch buffers of a NodeIterator: a flyweight handle of its own (so the decode of the next batch can run on
    another host thread, ImmutableGraph.java:187-197) and page-locked outdegree / successor buffers that are reused."""

    def __init__(self, graph, batch_nodes):
        self.g = graph.copy()
        self.deg = _pinned(batch_nodes, np.int32)
        # graphs whose ids fit 32 bits cross PCIe as uint32 (bvg_decode_range32): the transfer bounds this path, so half the bytes is
        # twice the rate; successor_array() widens to the longs of NodeIterator.successorBigArray()
        self.dt = np.uint32 if graph.num_nodes() + graph.node_base() <= 0xFFFFFFFF else np.int64   # (0xFFFFFFFF is never an id on this transport: it stands for -1)
        self.succ = _pinned(max(1024, 32 * batch_nodes), self.dt)
        self.lo = self.hi = 0
        self.n_succ = 0

    def decode(self, lo, hi):
        need = C.c_uint64(0)
        fn = lib().bvg_decode_range32 if self.dt is np.uint32 else lib().bvg_decode_range
        while True:
            st = fn(self.g._h, lo, hi, self.deg.array.ctypes.data, self.succ.array.ctypes.data, len(self.succ.array), C.byref(need))
            if st == _abi.E_CAPACITY:
                _unpin(self.succ)
                self.succ = _pinned(((int(need.value) + int(need.value) // 4) + 0xFFFFF) & ~0xFFFFF, self.dt)
                continue
            _check(st, "decode_range(%d,%d)" % (lo, hi))
            break
        self.lo, self.hi, self.n_succ = lo, hi, int(need.value)
        return self

    def close(self):
        _unpin(self.deg); _unpin(self.succ); self.deg = self.succ = None; self.g.close()


class NodeIterator:
    """BVGraph.BVGraphNodeIterator (BVGraph.java:1100-1245) fed by batched GPU decodes.  Two batch slots: while the caller walks
    batch i, a helper thread decodes batch i+1 (kernels + device -> host copy into page-locked memory) through a flyweight of
    the graph, so the PCIe transfer and the decode overlap with the consumer."""

    def __init__(self, graph, frm, upper_bound=None, batch_nodes=None):
        n = graph.num_nodes()
        if frm < 0 or frm > n:
            raise IllegalArgumentException(_abi.E_ARG, "nodeIterator(%d)" % frm)        # BVG:1128
        self._g = graph
        self._from = frm
        self._curr = frm - 1                                                           # BVG:1147
        self._limit = min(upper_bound if upper_bound is not None else n, n) - 1         # BVG:1148
        self._batch_nodes = batch_nodes or graph.iterator_batch_nodes
        self._b0 = frm; self._b1 = frm
        self._deg = None; self._cum = None; self._succ = None
        self._slots = None; self._pending = []; self._pool = None; self._held = None; self._free = []

    def has_next(self):
        return self._curr < self._limit                                                # BVG:1179-1181

    hasNext = has_next

    _DEPTH = int(os.environ.get("BVG_ITER_DEPTH", "2"))                                                                         # batches decoded ahead of the caller

    def _start(self):
        import concurrent.futures
        bn = max(1, min(self._batch_nodes, self._limit + 1 - self._from))
        nb = -(-(self._limit + 1 - self._from) // bn)
        depth = max(0, min(self._DEPTH, nb - 1))
        self._slots = [_BatchSlot(self._g, bn) for _ in range(depth + 1)]
        self._free = list(range(depth + 1))
        self._pending = []                                                             # [(future, first node, slot index)], in node order
        self._held = None
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, depth)) if depth else None

    def _fill(self, x):
        if self._slots is None:
            self._start()
        if self._held is not None:                                                     # the batch the caller has left: its buffers may be reused
            self._free.append(self._held); self._held = None
        slot = None
        while self._pending:
            fut, plo, si = self._pending.pop(0)
            got = fut.result()                                                         # (raises what the decode raised)
            if plo == x:
                slot = got; self._held = si
                break
            self._free.append(si)                                                      # the caller jumped elsewhere: drop what was decoded ahead
        if slot is None:
            si = self._free.pop()
            slot = self._slots[si].decode(x, min(x + self._batch_nodes, self._limit + 1)); self._held = si
        # keep the pipeline full: the batches behind this one are decoded (kernels + device -> host copy) by helper threads, each
        # through its own flyweight handle and stream, so one batch's copy overlaps the next one's kernels
        nxt = self._pending[-1][1] + self._batch_nodes if self._pending else slot.hi
        while self._pool is not None and self._free and nxt <= self._limit:
            si = self._free.pop()
            self._pending.append((self._pool.submit(self._slots[si].decode, nxt, min(nxt + self._batch_nodes, self._limit + 1)), nxt, si))
            nxt += self._batch_nodes
        self._b0, self._b1 = slot.lo, slot.hi
        self._deg = slot.deg.array[:slot.hi - slot.lo]
        self._cum = np.zeros(len(self._deg) + 1, dtype=np.int64)
        np.cumsum(self._deg, out=self._cum[1:])
        self._succ = slot.succ.array[:slot.n_succ]

    def next_long(self):
        if not self.has_next():
            raise NoSuchElementException()                                             # BVG:1165
        self._curr += 1
        if not (self._b0 <= self._curr < self._b1):
            self._fill(self._curr)
        return self._curr

    nextLong = next_long

    def __iter__(self):
        while self.has_next():
            yield self.next_long()

    def _require_started(self):
        if self._curr == self._from - 1:
            raise IllegalStateException(_abi.E_STATE, "no node fetched yet")            # BVG:1185,1193,1207

    def outdegree(self):
        self._require_started()
        return int(self._deg[self._curr - self._b0])

    def successor_array(self):
        """successorBigArray(): view valid until the next next_long() (NodeIterator.java:80-96)."""
        self._require_started()
        i = self._curr - self._b0
        v = self._succ[self._cum[i]:self._cum[i + 1]]
        if v.dtype == np.int64:
            return v
        w = v.astype(np.int64)                                         # (ids that crossed PCIe as uint32 are widened here)
        w[v == 0xFFFFFFFF] = -1                                        # the stand-in for a missing successor of a malformed stream: -1, as on the int64 transport
        return w

    successorBigArray = successor_array

    def batch(self):
        """The whole current batch at once: (first node, outdeg int32[], cum int64[], succ) — views valid until the next next_long()
        that leaves the batch (what a bulk consumer walks instead of one node at a time).  succ is uint32 for graphs whose ids fit
        32 bits (as it crossed PCIe: 0xFFFFFFFF there stands for the -1 of a malformed stream, never for a node), int64 otherwise."""
        self._require_started()
        return self._b0, self._deg, self._cum, self._succ

    def skip_batch(self):
        """Moves to the last node of the current batch (the next next_long() fetches the following batch)."""
        self._require_started()
        self._curr = self._b1 - 1

    def successors(self):
        return LazyLongIterator(self.successor_array())

    def copy(self, upper_bound=None):
        """NodeIterator.copy(upperBound), BVG:1223-1229: a new iterator positioned after the current node."""
        ub = self._limit + 1 if upper_bound is None else upper_bound
        return NodeIterator(self._g.copy(), self._curr + 1, ub, self._batch_nodes)

    def skip(self, n):
        k = 0
        while k < n and self.has_next():
            self.next_long(); k += 1
        return k

    def close(self):
        for fut, _, _ in self._pending:
            try:
                fut.result()
            except Exception:
                pass
        self._pending = []
        if self._pool is not None:
            self._pool.shutdown(wait=True); self._pool = None
        if self._slots is not None:
            for sl in self._slots:
                sl.close()
            self._slots = None
        self._deg = self._cum = self._succ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BVGraph:
    """ImmutableGraph / BVGraph surface for the decode path, backed by HBM-resident data."""

    iterator_batch_nodes = 1 << 16

    def __init__(self, handle, keep=()):
        self._h = handle
        self._keep = keep
        self._params = Params()
        _check(lib().bvg_info(self._h, C.byref(self._params)), "info")
        self._basename = None

    # ---- loading (BVGraph.java:1345-1464) ----
    @classmethod
    def load(cls, basename, device=0, mode=_abi.LOAD_STANDARD):
        h = C.c_void_p()
        _check(lib().bvg_open(os.fsencode(basename), mode, device, C.byref(h)), "load(%s)" % basename)
        g = cls(h); g._basename = basename
        return g

    @classmethod
    def load_mapped(cls, basename, device=0):
        return cls.load(basename, device, _abi.LOAD_MAPPED)

    @classmethod
    def load_offline(cls, basename, device=0):
        return cls.load(basename, device, _abi.LOAD_OFFLINE)

    @classmethod
    def load_sequential(cls, basename, device=0):
        return cls.load(basename, device, _abi.LOAD_SEQUENTIAL)

    @classmethod
    def from_memory(cls, params, graph_bytes, offsets, device=0):
        g = np.frombuffer(bytes(graph_bytes), dtype=np.uint8) if not isinstance(graph_bytes, np.ndarray) else np.ascontiguousarray(graph_bytes, dtype=np.uint8)
        o = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().bvg_open_mem(C.byref(params), g.ctypes.data if len(g) else None, len(g), None if o is None else o.ctypes.data, device, C.byref(h)), "open_mem")
        return cls(h)

    @classmethod
    def from_device(cls, params, d_graph_ptr, nbytes, d_offsets_ptr, device=0, keep=()):
        """Adopts buffers already resident in HBM (e.g. torch tensors; pass them in `keep`)."""
        h = C.c_void_p()
        _check(lib().bvg_open_dev(C.byref(params), d_graph_ptr, nbytes, d_offsets_ptr, device, C.byref(h)), "open_dev")
        return cls(h, keep=keep)

    def tile(self, copies):
        """Synthetic workload helper: `copies` back-to-back copies of this graph (bvg_tile)."""
        h = C.c_void_p()
        _check(lib().bvg_tile(self._h, copies, C.byref(h)), "tile")
        return BVGraph(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().bvg_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- ImmutableGraph surface ----
    @property
    def params(self):
        return self._params

    def num_nodes(self):
        return int(self._params.nodes)

    def num_arcs(self):
        if self._params.arcs < 0:
            raise UnsupportedOperationException(_abi.E_UNSUPPORTED, "numArcs")           # ImmutableGraph.java:253-258
        return int(self._params.arcs)

    numNodes, numArcs = num_nodes, num_arcs

    def random_access(self):
        return True

    def has_copiable_iterators(self):
        return True

    def basename(self):
        return self._basename

    def window_size(self):
        return int(self._params.window_size)

    def max_ref_count(self):
        return int(self._params.max_ref_count)

    def min_interval_length(self):
        return int(self._params.min_interval_length)

    def copy(self):
        """BVGraph.copy() (BVGraph.java:553-578): shares the device data, own stream/workspace."""
        h = C.c_void_p()
        _check(lib().bvg_copy(self._h, C.byref(h)), "copy")
        g = BVGraph(h); g._basename = self._basename
        if self.node_base():
            g.set_node_base(self.node_base())                               # (a flyweight answers in the same id space)
        return g

    def set_node_base(self, base):
        _check(lib().bvg_set_node_base(self._h, base), "set_node_base")
        self._node_base = int(base)

    def node_base(self):
        return getattr(self, "_node_base", 0)

    def set_tuning(self, block_bits=0, force_wide=False, force_slow=False, stream=False, grab_threshold=0, legacy=False, no_index=False):
        # (no_index: False / True, or 2 = "marks only": the index this handle builds keeps the validation marks and entries for lists of >= 4 096 residuals only)
        """stream=True selects the experimental streaming data-flow kernel (experimental/bvg_stream.hip) as tier 0; no_index=True makes
        this handle scan without the residual skip index (neither built nor read)."""
        t = Tuning(block_bits, int(force_wide), int(force_slow), (2 if stream else (1 if legacy else 0)) | (int(grab_threshold) << 8), int(no_index))
        _check(lib().bvg_set_tuning(self._h, C.byref(t)), "set_tuning")

    def offsets(self):
        out = np.empty(self.num_nodes() + 1, dtype=np.uint64)
        _check(lib().bvg_get_offsets(self._h, out.ctypes.data), "get_offsets")
        return out

    def outdegrees(self, frm=0, to=None):
        to = self.num_nodes() if to is None else to
        out = np.empty(max(to - frm, 0), dtype=np.int32)
        _check(lib().bvg_outdegrees(self._h, frm, to, out.ctypes.data if len(out) else None) if to > frm else (0 if 0 <= frm <= self.num_nodes() else _abi.E_ARG), "outdegrees")
        return out

    def outdegree(self, x):
        if x < 0 or x >= self.num_nodes():
            raise IllegalArgumentException(_abi.E_ARG, "outdegree(%d)" % x)               # BVG:823
        return int(self.outdegrees(x, x + 1)[0])

    def decode_range(self, frm, to):
        """(outdeg int32[to-frm], succ int64[sum]) of nodes [frm,to) — bit-exact with nodeIterator(frm)."""
        if frm < 0 or to > self.num_nodes() or frm > to:
            raise IllegalArgumentException(_abi.E_ARG, "decode_range(%d,%d)" % (frm, to))
        cnt = to - frm
        deg = np.empty(max(cnt, 1), dtype=np.int32)
        need = C.c_uint64(0)
        cap = max(1024, 16 * cnt)
        while True:
            succ = np.empty(cap, dtype=np.int64)
            st = lib().bvg_decode_range(self._h, frm, to, deg.ctypes.data, succ.ctypes.data, cap, C.byref(need))
            if st == _abi.E_CAPACITY:
                cap = int(need.value)
                continue
            _check(st, "decode_range(%d,%d)" % (frm, to))
            return deg[:cnt], succ[:need.value]

    def decode_range32(self, frm, to):
        """decode_range with the successors as uint32 (bvg_decode_range32: graphs whose ids fit 32 bits; half the bytes over PCIe)."""
        if frm < 0 or to > self.num_nodes() or frm > to:
            raise IllegalArgumentException(_abi.E_ARG, "decode_range32(%d,%d)" % (frm, to))
        cnt = to - frm
        deg = np.empty(max(cnt, 1), dtype=np.int32)
        need = C.c_uint64(0)
        cap = max(1024, 16 * cnt)
        while True:
            succ = np.empty(cap, dtype=np.uint32)
            st = lib().bvg_decode_range32(self._h, frm, to, deg.ctypes.data, succ.ctypes.data, cap, C.byref(need))
            if st == _abi.E_CAPACITY:
                cap = int(need.value)
                continue
            _check(st, "decode_range32(%d,%d)" % (frm, to))
            return deg[:cnt], succ[:need.value]

    def successors_batch(self, nodes):
        """successors(x) for a frontier: returns (outdeg int32[len(nodes)], succ int64[sum]) in request order."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        deg = np.empty(max(len(nodes), 1), dtype=np.int32)
        need = C.c_uint64(0)
        cap = max(1024, 16 * len(nodes))
        while True:
            succ = np.empty(cap, dtype=np.int64)
            st = lib().bvg_successors_batch(self._h, nodes.ctypes.data if len(nodes) else None, len(nodes), deg.ctypes.data, succ.ctypes.data, cap, C.byref(need))
            if st == _abi.E_CAPACITY:
                cap = int(need.value)
                continue
            _check(st, "successors_batch")
            return deg[:len(nodes)], succ[:need.value]

    def successor_array(self, x):
        if x < 0 or x >= self.num_nodes():
            raise IllegalArgumentException(_abi.E_ARG, "successors(%d)" % x)              # BVG:863
        return self.decode_range(x, x + 1)[1]

    successorBigArray = successor_array

    def successors(self, x):
        return LazyLongIterator(self.successor_array(x))

    def node_iterator(self, frm=0):
        return NodeIterator(self, frm)

    nodeIterator = node_iterator

    def split_node_iterators(self, how_many):
        """ImmutableGraph.splitNodeIterators (ImmutableGraph.java:405-436): ceil(n/k)-sized ranges."""
        n = self.num_nodes()
        if how_many <= 0:
            raise IllegalArgumentException(_abi.E_ARG, "splitNodeIterators")
        m = -(-n // how_many) if n else 0
        its = []
        for i in range(how_many):
            lo = min(i * m, n)
            hi = min(lo + m, n)
            its.append(NodeIterator(self.copy(), lo, hi) if lo < n else NodeIterator(self, n, n))
        return its

    splitNodeIterators = split_node_iterators

    def split_by_bits(self, k):
        b = np.empty(k + 1, dtype=np.int64)
        _check(lib().bvg_split_by_bits(self._h, k, b.ctypes.data), "split_by_bits")
        return b

    def split_by_arcs(self, k):
        """Node-range split points with ~equal arc counts (HyperBall.java:748-768 over the cumulative outdegrees)."""
        b = np.empty(k + 1, dtype=np.int64)
        _check(lib().bvg_split_by_arcs(self._h, k, b.ctypes.data), "split_by_arcs")
        return b

    def shard_bounds(self, k, balance=None):
        """bounds[0..k] of the k-way node-range split (bvg_shard_bounds): BALANCE_NODES is ImmutableGraph.java:415-433."""
        b = np.empty(k + 1, dtype=np.int64)
        _check(lib().bvg_shard_bounds(self._h, k, BALANCE_ARCS if balance is None else balance, b.ctypes.data), "shard_bounds")
        return b

    def scan_shard(self, k, r, balance=None):
        """The scan of shard r of k (bvg_scan_shard): dict of bvg_scan_result plus 'from' / 'to'."""
        res = ScanResult(); lo = C.c_int64(); hi = C.c_int64()
        _check(lib().bvg_scan_shard(self._h, k, r, BALANCE_ARCS if balance is None else balance, C.byref(res), C.byref(lo), C.byref(hi)), "scan_shard(%d,%d)" % (k, r))
        d = res.as_dict(); d["from"] = lo.value; d["to"] = hi.value
        return d

    def transpose(self):
        """The transpose in CSR form (toffsets uint64[n+1], tsucc int64[arcs]): the decode + sort of Transform.transposeOffline
        (Transform.java:1058-1160) done on the device; sources of every node's incoming arcs in increasing order."""
        n = self.num_nodes()
        toff = np.empty(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        st = lib().bvg_transpose(self._h, toff.ctypes.data, None, 0, C.byref(need))
        if st not in (0, _abi.E_CAPACITY):
            _check(st, "transpose")
        tsucc = np.empty(max(int(need.value), 1), dtype=np.int64)
        _check(lib().bvg_transpose(self._h, toff.ctypes.data, tsucc.ctypes.data, len(tsucc), C.byref(need)), "transpose")
        return toff, tsucc[:int(need.value)]

    def symmetrize(self):
        """The symmetrised graph in CSR form (soffsets uint64[n+1], ssucc int64): Transform.symmetrizeOffline
        (Transform.java:546-575) = union of the graph and its transpose, computed on the device."""
        n = self.num_nodes()
        soff = np.empty(n + 1, dtype=np.uint64)
        need = C.c_uint64(0)
        ssucc = np.empty(max(2 * max(int(self._params.arcs), 0), 1), dtype=np.int64)       # 2 x arcs always suffices
        st = lib().bvg_symmetrize(self._h, soff.ctypes.data, ssucc.ctypes.data, len(ssucc), C.byref(need))
        if st == _abi.E_CAPACITY:                                                          # numArcs unknown in the properties
            ssucc = np.empty(int(need.value), dtype=np.int64)
            st = lib().bvg_symmetrize(self._h, soff.ctypes.data, ssucc.ctypes.data, len(ssucc), C.byref(need))
        _check(st, "symmetrize")
        return soff, ssucc[:int(need.value)]

    def connected_components(self, sizes=False, sort_by_size=False):
        """ConnectedComponents (algo/ConnectedComponents.java) of the graph with its arcs taken in both directions -- the weak
        components; on a symmetric graph exactly compute(g).component -- by a union-find on the device (bvg_components).
        Component c is the one whose smallest node is the c-th smallest among the components' smallest nodes; sort_by_size=True
        renumbers by decreasing size, ties by smallest node (sortBySize).  sizes=True also returns computeSizes()."""
        L = _components_fns()
        n = self.num_nodes()
        comp = np.empty(max(n, 1), dtype=np.int64)
        cnt = C.c_uint64(0)
        flags = CC_SORT_BY_SIZE if sort_by_size else 0
        sz = None
        cap = max(n, 1) if sizes else 0
        if sizes:
            sz = np.empty(cap, dtype=np.int64)
        _check(L.bvg_components(self._h, flags, comp.ctypes.data, None if sz is None else sz.ctypes.data, cap, C.byref(cnt)), "connected_components")
        k = int(cnt.value)
        return ComponentsResult(k, comp[:n], None if sz is None else sz[:k])

    connectedComponents = connected_components

    def connected_components_dev(self, comp_tensor, sizes_tensor=None, sort_by_size=False):
        """bvg_components_dev: labels into comp_tensor (int64, numNodes() elements, on the graph's device) and, when given, sizes
        into sizes_tensor (int64; BVG_E_CAPACITY -> IllegalArgumentException if it holds fewer than the count).  Returns the count."""
        import torch
        L = _components_fns()
        n = self.num_nodes()
        for t, what in ((comp_tensor, "comp"), (sizes_tensor, "sizes")):
            if t is not None and (not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous()):
                raise IllegalArgumentException(_abi.E_ARG, "%s must be a contiguous int64 CUDA tensor" % what)
        if comp_tensor.numel() < n:
            raise IllegalArgumentException(_abi.E_ARG, "comp holds %d elements, the graph %d nodes" % (comp_tensor.numel(), n))
        cnt = C.c_uint64(0)
        st = L.bvg_components_dev(self._h, CC_SORT_BY_SIZE if sort_by_size else 0, comp_tensor.data_ptr() if n else None,
                                  None if sizes_tensor is None else sizes_tensor.data_ptr(), 0 if sizes_tensor is None else sizes_tensor.numel(), C.byref(cnt))
        if st == _abi.E_CAPACITY:
            raise IllegalArgumentException(st, "connected_components_dev: %d components, sizes holds %d" % (int(cnt.value), sizes_tensor.numel()))
        _check(st, "connected_components_dev")
        return int(cnt.value)

    def strongly_connected_components(self, sizes=False, sort_by_size=False, buckets=False):
        """StronglyConnectedComponents.compute (algo/StronglyConnectedComponents.java) on the device (bvg_scc): sweeps of the
        compressed graph over forward arcs only -- trimming, one forward-backward step, colouring rounds.  The partition, the count,
        the sizes and the buckets are the reference's; the numbering is not Tarjan's emission order: component c is the one whose
        smallest node is the c-th smallest among the components' smallest nodes, and sort_by_size=True (sortBySize) renumbers by
        decreasing size, ties by smallest node.  sizes=True also returns computeSizes(); buckets=True the computeBuckets() set as one
        bool per node (its component has an arc and none that leaves it).  Returns an SCCResult."""
        L = _scc_fns()
        n = self.num_nodes()
        comp = np.empty(max(n, 1), dtype=np.int64)
        cnt = C.c_uint64(0)
        flags = (SCC_SORT_BY_SIZE if sort_by_size else 0) | (SCC_BUCKETS if buckets else 0)
        cap = max(n, 1) if sizes else 0
        sz = np.empty(cap, dtype=np.int64) if sizes else None
        bk = np.zeros(max(n, 1), dtype=np.uint8) if buckets else None
        ctr = np.zeros(_abi.SCC_COUNTER_WORDS, dtype=np.uint64)
        _check(L.bvg_scc(self._h, flags, comp.ctypes.data, None if sz is None else sz.ctypes.data, cap, C.byref(cnt),
                         None if bk is None else bk.ctypes.data, ctr.ctypes.data), "strongly_connected_components")
        k = int(cnt.value)
        return SCCResult(k, comp[:n], None if sz is None else sz[:k], None if bk is None else bk[:n].astype(bool),
                         dict(zip(SCC_COUNTERS, (int(v) for v in ctr))))

    stronglyConnectedComponents = strongly_connected_components

    def strongly_connected_components_dev(self, comp_tensor, sizes_tensor=None, buckets_tensor=None, sort_by_size=False):
        """bvg_scc_dev: labels into comp_tensor (int64, numNodes() elements, on the graph's device), when given sizes into
        sizes_tensor (int64; BVG_E_CAPACITY -> IllegalArgumentException if it holds fewer than the count) and the buckets into
        buckets_tensor (uint8, numNodes() elements, 0 / 1).  Returns (count, counters)."""
        import torch
        L = _scc_fns()
        n = self.num_nodes()
        for t, what, dt in ((comp_tensor, "comp", torch.int64), (sizes_tensor, "sizes", torch.int64), (buckets_tensor, "buckets", torch.uint8)):
            if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
                raise IllegalArgumentException(_abi.E_ARG, "%s must be a contiguous %s CUDA tensor" % (what, dt))
        for t, what in ((comp_tensor, "comp"), (buckets_tensor, "buckets")):
            if t is not None and t.numel() < n:
                raise IllegalArgumentException(_abi.E_ARG, "%s holds %d elements, the graph %d nodes" % (what, t.numel(), n))
        cnt = C.c_uint64(0)
        ctr = np.zeros(_abi.SCC_COUNTER_WORDS, dtype=np.uint64)
        flags = (SCC_SORT_BY_SIZE if sort_by_size else 0) | (SCC_BUCKETS if buckets_tensor is not None else 0)
        st = L.bvg_scc_dev(self._h, flags, comp_tensor.data_ptr() if n else None, None if sizes_tensor is None else sizes_tensor.data_ptr(),
                           0 if sizes_tensor is None else sizes_tensor.numel(), C.byref(cnt), None if buckets_tensor is None else buckets_tensor.data_ptr(), ctr.ctypes.data)
        if st == _abi.E_CAPACITY:
            raise IllegalArgumentException(st, "strongly_connected_components_dev: %d components, sizes holds %d" % (int(cnt.value), sizes_tensor.numel()))
        _check(st, "strongly_connected_components_dev")
        return int(cnt.value), dict(zip(SCC_COUNTERS, (int(v) for v in ctr)))

    def stats(self, indegrees=False):
        """Stats.run (Stats.java) on the device (bvg_stats_compute): one sweep of the compressed graph counts arcs, loops, dangling and
        terminal nodes, the degree extremes (ties as the reference breaks them: the smallest node for outdegrees, the largest for
        indegrees), the gap and locality sums (exact Python ints) and the binned gap histogram, and gives both degree distributions.
        indegrees=True also returns the indegree of every node (int64).  Returns a GraphStats."""
        L = _stats_fns()
        h = C.c_void_p()
        _check(L.bvg_stats_compute(self._h, _abi.STATS_KEEP_INDEGREES_FLAG if indegrees else 0, C.byref(h)), "stats")
        try:
            sm = _abi.StatsSummary()
            _check(L.bvg_stats_get(h, C.byref(sm)), "stats_get")
            dists = []
            for which in (_abi.STATS_OUT, _abi.STATS_IN):
                ln = C.c_uint64(0)
                st = L.bvg_stats_distribution(h, which, None, 0, C.byref(ln))
                if st != _abi.E_CAPACITY:
                    _check(st, "stats_distribution")
                d = np.zeros(int(ln.value), dtype=np.uint64)
                _check(L.bvg_stats_distribution(h, which, d.ctypes.data, len(d), C.byref(ln)), "stats_distribution")
                dists.append(d)
            ind = None
            if indegrees:
                n = int(sm.nodes)
                ind = np.zeros(n, dtype=np.int64)
                _check(L.bvg_stats_indegrees(h, 0, n, ind.ctypes.data if n else None), "stats_indegrees")
        finally:
            L.bvg_stats_close(h)
        return GraphStats.from_summary(sm, dists[0], dists[1], ind)

    def _geometric_range(self, sources):
        n = self.num_nodes()
        lo, hi = (0, n) if sources is None else (int(sources[0]), int(sources[1]))
        if lo < 0 or lo > hi or hi > n:
            raise IllegalArgumentException(_abi.E_ARG, "sources [%d, %d) of a graph of %d nodes" % (lo, hi, n))
        return lo, hi

    def linear_geometric_centrality(self, coeffs, sources=None, histogram=False):
        """LinearGeometricCentrality.compute (algo/LinearGeometricCentrality.java) on the device (bvg_geometric): the exact positive
        geometric centrality sum of coeff(d(s, y)) over the nodes y reachable from s, and the number of those nodes (s included), for
        the sources s in `sources` = (from, to) (None: every node), by bit-parallel breadth-first visits: one sweep of the compressed
        graph advances up to 512 sources by one level.  coeffs: "harmonic" (0, 1, 1/2, ...), ("power", e) (d ** e), ("exp", b)
        (b ** d) or an array (coeff(d) = array[d], 0 beyond its end).  The sum is formed in double and rounded to float32 once (the
        reference rounds once per reached node).  histogram=True also returns the number of (source, node) pairs at every distance.
        Returns a GeometricResult."""
        L = _geometric_fns()
        kind, param, table = _geometric_coeffs(coeffs)
        lo, hi = self._geometric_range(sources)
        cen = np.empty(hi - lo, dtype=np.float32); rea = np.empty(hi - lo, dtype=np.int64)
        ctr = np.zeros(_abi.GEO_COUNTER_WORDS, dtype=np.uint64)
        cap = self.num_nodes() + 1 if histogram else 0                      # (distances are below the number of nodes)
        hist = np.zeros(cap, dtype=np.uint64) if histogram else None
        hlen = C.c_uint64(0)
        _check(L.bvg_geometric(self._h, kind, param, None if table is None else table.ctypes.data, 0 if table is None else len(table), lo, hi,
                               cen.ctypes.data if hi > lo else None, rea.ctypes.data if hi > lo else None, None if hist is None else hist.ctypes.data, cap,
                               C.byref(hlen), ctr.ctypes.data), "linear_geometric_centrality")
        return GeometricResult(cen, rea, None if hist is None else hist[:int(hlen.value)].copy(), dict(zip(GEO_COUNTERS, (int(v) for v in ctr))), (lo, hi), (kind, param))

    linearGeometricCentrality = linear_geometric_centrality

    def linear_geometric_centrality_dev(self, coeffs, centrality_tensor=None, reachable_tensor=None, sources=None, histogram=False):
        """bvg_geometric_dev: the centralities into centrality_tensor (float32) and the reachable counts into reachable_tensor (int64),
        each of at least to - from elements on the graph's device; either may be None.  Returns (histogram or None, counters)."""
        import torch
        L = _geometric_fns()
        kind, param, table = _geometric_coeffs(coeffs)
        lo, hi = self._geometric_range(sources)
        for t, what, dt in ((centrality_tensor, "centrality", torch.float32), (reachable_tensor, "reachable", torch.int64)):
            if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
                raise IllegalArgumentException(_abi.E_ARG, "%s must be a contiguous %s CUDA tensor" % (what, dt))
            if t is not None and t.numel() < hi - lo:
                raise IllegalArgumentException(_abi.E_ARG, "%s holds %d elements, the range %d sources" % (what, t.numel(), hi - lo))
        ctr = np.zeros(_abi.GEO_COUNTER_WORDS, dtype=np.uint64)
        cap = self.num_nodes() + 1 if histogram else 0
        hist = np.zeros(cap, dtype=np.uint64) if histogram else None
        hlen = C.c_uint64(0)
        _check(L.bvg_geometric_dev(self._h, kind, param, None if table is None else table.ctypes.data, 0 if table is None else len(table), lo, hi,
                                   None if centrality_tensor is None else centrality_tensor.data_ptr(), None if reachable_tensor is None else reachable_tensor.data_ptr(),
                                   None if hist is None else hist.ctypes.data, cap, C.byref(hlen), ctr.ctypes.data), "linear_geometric_centrality_dev")
        return None if hist is None else hist[:int(hlen.value)].copy(), dict(zip(GEO_COUNTERS, (int(v) for v in ctr)))

    def breadth_first_visit(self, parent=False):
        """ParallelBreadthFirstVisit (algo/ParallelBreadthFirstVisit.java) with its state on the device: see BreadthFirstVisit."""
        return BreadthFirstVisit(self, parent)

    breadthFirstVisit = breadth_first_visit

    def hyperball(self, log2m, seed=0, sum_of_distances=False, harmonic=False):
        """HyperBall (algo/HyperBall.java, non-systolic) with its counters on the device: see HyperBall."""
        return HyperBall(self, log2m, seed, sum_of_distances, harmonic)

    hyperBall = hyperball

    def build_index(self, frm=0, to=None):
        """Builds the residual skip index (and validates the blocks) of nodes [frm, to) now (bvg_build_index) instead of inside
        the first scan; returns (entries, bytes) of the graph's index afterwards."""
        to = self.num_nodes() if to is None else to
        e = C.c_uint64(); b = C.c_uint64()
        _check(lib().bvg_build_index(self._h, frm, to, C.byref(e), C.byref(b)), "build_index(%d,%d)" % (frm, to))
        return int(e.value), int(b.value)

    def save_index(self, path=None):
        """Writes the device index (block plan + residual skip index) to `path` (default: basename.bvgidx, which load() picks up)."""
        path = path or (self._basename + ".bvgidx")
        _check(lib().bvg_save_index(self._h, os.fsencode(path)), "save_index(%s)" % path)
        return path

    def load_index(self, path):
        """Loads an index written by save_index(); IOException if the file does not belong to this graph."""
        _check(lib().bvg_load_index(self._h, os.fsencode(path)), "load_index(%s)" % path)

    def scan(self, frm=0, to=None):
        """Full sequential successor scan consumed on chip (SpeedTest.java:127-141): dict of bvg_scan_result."""
        to = self.num_nodes() if to is None else to
        r = ScanResult()
        _check(lib().bvg_scan(self._h, frm, to, C.byref(r)), "scan(%d,%d)" % (frm, to))
        return r.as_dict()


BALANCE_NODES, BALANCE_BITS, BALANCE_ARCS = 0, 1, 2
CC_SORT_BY_SIZE = 1
BFS_PARENT = 1
SCC_SORT_BY_SIZE, SCC_BUCKETS = 1, 2
SCC_COUNTERS = ("sweeps", "batch_decodes", "trim_passes", "trimmed_nodes", "fwbw_component", "colouring_rounds", "colouring_components", "single_resident_batch")
GEO_COUNTERS = ("passes", "sweeps", "batch_decodes", "words_per_node", "deepest_pass_levels", "levels_skipped", "single_resident_batch", "reserved")
BFS_COUNTERS = ("frontier_levels", "sweep_levels", "deep_requests", "frontier_batches", "sweep_batches", "sorted_levels", "compacted_levels", "first_level_route")


class BreadthFirstVisit:
    """What ParallelBreadthFirstVisit holds (marker, round, queue, cutPoints; ParallelBreadthFirstVisit.java:79-148), kept on the device
    between visits (bvg_bfs_*), plus dist: the level of every node of the last visit, -1 for the others.  Where the reference depends
    on thread timing this is fixed: inside a level the queue is in increasing id, and with parent=True marker[x] is the smallest node
    of the previous level that has x as a successor (the root's parent is itself); otherwise marker[x] is the round that reached x.
    The object holds its own flyweight of the graph.  Usable as a context manager."""

    def __init__(self, graph, parent=False):
        self._L = _bfs_fns()
        self._v = C.c_void_p()
        self._n = graph.num_nodes()
        self.parent = bool(parent)
        _check(self._L.bvg_bfs_create(graph._h, BFS_PARENT if parent else 0, C.byref(self._v)), "breadth_first_visit")

    def close(self):
        if getattr(self, "_v", None):
            self._L.bvg_bfs_close(self._v)
            self._v = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        _check(self._L.bvg_bfs_clear(self._v), "clear")

    def visit(self, start):
        """visit(start): the number of nodes visited (0 when start was marked already: nothing changes then)."""
        k = C.c_uint64(0)
        _check(self._L.bvg_bfs_visit(self._v, start, C.byref(k)), "visit(%d)" % start)
        return int(k.value)

    def visit_all(self):
        _check(self._L.bvg_bfs_visit_all(self._v), "visit_all")

    visitAll = visit_all

    def _info(self):
        r, q, c = C.c_int64(), C.c_uint64(), C.c_uint64()
        _check(self._L.bvg_bfs_info(self._v, C.byref(r), C.byref(q), C.byref(c)), "info")
        return int(r.value), int(q.value), int(c.value)

    @property
    def round(self):
        return self._info()[0]

    @property
    def queue(self):
        q = self._info()[1]
        out = np.empty(q, dtype=np.int64)
        if q:
            _check(self._L.bvg_bfs_get(self._v, None, out.ctypes.data, q, None, 0, None), "queue")
        return out

    @property
    def cut_points(self):
        c = self._info()[2]
        out = np.empty(c, dtype=np.uint64)
        if c:
            _check(self._L.bvg_bfs_get(self._v, None, None, 0, out.ctypes.data, c, None), "cut_points")
        return out.astype(np.int64)

    cutPoints = cut_points

    @property
    def marker(self):
        out = np.empty(self._n, dtype=np.int64)
        if self._n:
            _check(self._L.bvg_bfs_get(self._v, out.ctypes.data, None, 0, None, 0, None), "marker")
        return out

    @property
    def dist(self):
        out = np.empty(self._n, dtype=np.int32)
        if self._n:
            _check(self._L.bvg_bfs_get(self._v, None, None, 0, None, 0, out.ctypes.data), "dist")
        return out

    def get_dev(self, marker=None, queue=None, cut_points=None, dist=None):
        """bvg_bfs_get_dev into contiguous CUDA tensors (marker, queue, cut_points: int64; dist: int32) on the graph's device."""
        ptr = lambda t: None if t is None else t.data_ptr()
        _check(self._L.bvg_bfs_get_dev(self._v, ptr(marker), ptr(queue), 0 if queue is None else queue.numel(), ptr(cut_points),
                                       0 if cut_points is None else cut_points.numel(), ptr(dist)), "get_dev")

    def max_distance(self):
        """maxDistance(): cutPoints.size() - 2 (ParallelBreadthFirstVisit.java:355-357)."""
        return self._info()[2] - 2

    def node_at_max_distance(self):
        """nodeAtMaxDistance(): the last element of the queue (:346-348)."""
        q = self.queue
        if not len(q):
            raise IndexError("node_at_max_distance: the queue is empty")
        return int(q[-1])

    maxDistance, nodeAtMaxDistance = max_distance, node_at_max_distance

    def counters(self):
        """What ran since the object was made (bvg_bfs_counters): levels per route, batches, requests decoded through the block plan, ..."""
        out = np.zeros(len(BFS_COUNTERS), dtype=np.uint64)
        _check(self._L.bvg_bfs_counters(self._v, out.ctypes.data), "counters")
        return dict(zip(BFS_COUNTERS, (int(x) for x in out)))


HB_SUM_OF_DISTANCES, HB_HARMONIC = 1, 2


class HyperBall:
    """What HyperBall holds (one HyperLogLog counter of 2^log2m registers per node, the neighbourhood function, the float32 sums of
    distances and of inverse distances when asked for; HyperBall.java:580-607, 777-919, 1000-1239), kept on the device between
    iterations (bvg_hyperball_*).  Iterations are the reference's standard (non-systolic, in-memory) ones.  The hash behind the
    counters is this library's (include/bvgraph_hip.h), so registers are not those of the Java implementation; the algorithm and the
    estimator are.  The object holds its own flyweight of the graph.  Usable as a context manager."""

    def __init__(self, graph, log2m, seed=0, sum_of_distances=False, harmonic=False):
        self._L = _hyperball_fns()
        self._h = C.c_void_p()
        self._n = graph.num_nodes()
        self.log2m, self.m = int(log2m), 1 << max(int(log2m), 0)
        flags = (HB_SUM_OF_DISTANCES if sum_of_distances else 0) | (HB_HARMONIC if harmonic else 0)
        _check(self._L.bvg_hyperball_create(graph._h, int(log2m), flags, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(self._h)), "hyperball(log2m=%d)" % log2m)

    def close(self):
        if getattr(self, "_h", None):
            self._L.bvg_hyperball_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, seed=0):
        _check(self._L.bvg_hyperball_init(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF), "init")

    def iterate(self):
        _check(self._L.bvg_hyperball_iterate(self._h), "iterate")

    def run(self, upper_bound=-1, threshold=-1.0):
        """run(upperBound, threshold): init with the object's seed, then iterate until nothing is modified, upper_bound (negative: none)
        iterations are done, or (threshold != -1) the relative increment falls below 1 + threshold after the fifth iteration."""
        _check(self._L.bvg_hyperball_run(self._h, int(upper_bound), float(threshold)), "run")

    def _info(self):
        it, mod, rel, k = C.c_int64(), C.c_uint64(), C.c_double(), C.c_uint64()
        _check(self._L.bvg_hyperball_info(self._h, C.byref(it), C.byref(mod), C.byref(rel), C.byref(k)), "info")
        return int(it.value), int(mod.value), float(rel.value), int(k.value)

    @property
    def iteration(self):
        return self._info()[0]

    def modified(self):
        return self._info()[1]

    @property
    def relative_increment(self):
        return self._info()[2]

    @property
    def neighbourhood_function(self):
        k = self._info()[3]
        out = np.empty(k, dtype=np.float64)
        if k:
            _check(self._L.bvg_hyperball_neighbourhood_function(self._h, out.ctypes.data, k), "neighbourhood_function")
        return out

    neighbourhoodFunction = neighbourhood_function

    def registers(self, frm=0, to=None):
        """The registers of counters [frm, to): uint8[to - frm, m]."""
        to = self._n if to is None else to
        out = np.empty((max(to - frm, 0), self.m), dtype=np.uint8)
        _check(self._L.bvg_hyperball_registers(self._h, frm, to, out.ctypes.data if out.size else None), "registers(%d,%d)" % (frm, to))
        return out

    def counts(self, frm=0, to=None):
        to = self._n if to is None else to
        out = np.empty(max(to - frm, 0), dtype=np.float64)
        _check(self._L.bvg_hyperball_counts(self._h, frm, to, out.ctypes.data if out.size else None), "counts(%d,%d)" % (frm, to))
        return out

    def count(self, x):
        return float(self.counts(x, x + 1)[0])

    def counts_dev(self, tensor, frm=0, to=None):
        """bvg_hyperball_counts_dev into a contiguous float64 CUDA tensor of at least to - frm elements."""
        to = self._n if to is None else to
        _check(self._L.bvg_hyperball_counts_dev(self._h, frm, to, tensor.data_ptr()), "counts_dev")

    def _centrality(self, which):
        out = np.empty(self._n, dtype=np.float32)
        _check(self._L.bvg_hyperball_centrality(self._h, _abi.HB_WHICH[which], out.ctypes.data if self._n else None), which)
        return out

    def centrality_dev(self, which, tensor):
        """bvg_hyperball_centrality_dev into a contiguous float32 CUDA tensor of numNodes() elements; which: a key of _abi.HB_WHICH."""
        _check(self._L.bvg_hyperball_centrality_dev(self._h, _abi.HB_WHICH[which], tensor.data_ptr()), which)

    def sum_of_distances(self):
        return self._centrality("sum_of_distances")

    def harmonic_centrality(self):
        return self._centrality("harmonic")

    def closeness(self):
        return self._centrality("closeness")

    def lin(self):
        return self._centrality("lin")

    def nieminen(self):
        return self._centrality("nieminen")

    def reachable(self):
        return self._centrality("reachable")

    sumOfDistances, sumOfInverseDistances = sum_of_distances, harmonic_centrality

    @staticmethod
    def relative_standard_deviation(log2m):
        return float(_hyperball_fns().bvg_hyperball_relative_standard_deviation(int(log2m)))


def _plain_decimal(x):
    """BigDecimal.valueOf(double).toPlainString(): the shortest decimal that reads back as x, never in scientific notation."""
    from decimal import Decimal
    return format(Decimal(repr(float(x))), "f")


def store_floats(values, path):
    """BinIO.storeFloats / DataOutputStream.writeFloat: big-endian float32, no header."""
    np.asarray(values, dtype=">f4").tofile(path)
    return path


def load_floats(path):
    return np.fromfile(path, dtype=">f4").astype(np.float32)


def hyperball_arg_parser():
    """The command line of HyperBall.main, for what is built: the option letters are the reference's."""
    import argparse
    ap = argparse.ArgumentParser(prog="hyperball", add_help=False, description="HyperBall on the device: neighbourhood function and geometric centralities of a BVGraph.")
    ap.add_argument("--help", action="help", help="show this message (-h is the reference's harmonic-centrality option)")
    ap.add_argument("-l", "--log2m", type=int, default=12, help="the logarithm of the number of registers per counter (4..12; default 12, the largest supported)")
    ap.add_argument("-u", "--upper-bound", type=int, default=-1, help="an upper bound to the number of iterations")
    ap.add_argument("-t", "--threshold", default="-1", help="stop when the relative increment falls below 1 + threshold (-1: only at stabilisation)")
    ap.add_argument("-n", "--neighbourhood-function", help="store the neighbourhood function in text format")
    ap.add_argument("-d", "--sum-of-distances", help="store the sum of distances from each node (big-endian floats)")
    ap.add_argument("-h", "--harmonic-centrality", help="store the harmonic centrality of each node (big-endian floats)")
    ap.add_argument("-c", "--closeness-centrality", help="store the closeness centrality of each node (big-endian floats)")
    ap.add_argument("-L", "--lin-centrality", help="store the Lin centrality of each node (big-endian floats)")
    ap.add_argument("-N", "--nieminen-centrality", help="store the Nieminen centrality of each node (big-endian floats)")
    ap.add_argument("-r", "--reachable", help="store the number of nodes reachable from each node (big-endian floats)")
    ap.add_argument("-S", "--seed", type=int, default=0, help="the random seed")
    ap.add_argument("-e", "--external", action="store_true", help="(not built: counters live in device memory)")
    ap.add_argument("-z", "--discounted-gain-centrality", action="append", help="(not built)")
    ap.add_argument("-Z", dest="big_z", action="append", help="(not built)")
    ap.add_argument("--device", type=int, default=0, help="the GPU to run on")
    ap.add_argument("basename", help="the basename of the graph")
    ap.add_argument("basenamet", nargs="?", default=None, help="(not built: the transpose, for systolic iterations)")
    return ap


def hyperball_main(argv=None):
    """HyperBall.main for the standard iterations: loads basename, runs, writes the files asked for.  Returns the HyperBall's
    neighbourhood function."""
    ap = hyperball_arg_parser()
    args = ap.parse_args(argv)
    try:
        threshold = float(args.threshold)
    except ValueError:
        ap.error("-t is the threshold here, and %r is not a number: a transpose basename (systolic iterations) is not supported" % args.threshold)
    if args.basenamet is not None:
        ap.error("a transpose basename (systolic iterations) is not supported: give the graph's basename only")
    if args.external:
        ap.error("-e (external counters) is not supported: the counters live in device memory")
    if args.discounted_gain_centrality or args.big_z:
        ap.error("-z / -Z (discounted gain centralities) are not supported")
    need_sod = bool(args.sum_of_distances or args.closeness_centrality or args.lin_centrality or args.nieminen_centrality)
    g = BVGraph.load(args.basename, device=args.device)
    try:
        with g.hyperball(args.log2m, seed=args.seed, sum_of_distances=need_sod, harmonic=bool(args.harmonic_centrality)) as hb:
            hb.run(args.upper_bound, threshold)
            nf = hb.neighbourhood_function
            if args.neighbourhood_function:
                with open(args.neighbourhood_function, "w") as f:
                    for x in nf:
                        f.write(_plain_decimal(x) + "\n")
            for path, get in ((args.sum_of_distances, hb.sum_of_distances), (args.harmonic_centrality, hb.harmonic_centrality), (args.closeness_centrality, hb.closeness),
                              (args.lin_centrality, hb.lin), (args.nieminen_centrality, hb.nieminen), (args.reachable, hb.reachable)):
                if path:
                    store_floats(get(), path)
    finally:
        g.close()
    return nf


class ComponentsResult:
    """What ConnectedComponents holds after compute(): numberOfComponents (count), component[] (int64 per node) and, when asked
    for, computeSizes() (sizes, int64 per component; None otherwise)."""

    def __init__(self, count, component, sizes=None):
        self.count, self.component, self.sizes = int(count), component, sizes

    numberOfComponents = property(lambda self: self.count)

    def __repr__(self):
        return "ComponentsResult(count=%d, nodes=%d, sizes=%s)" % (self.count, len(self.component), "yes" if self.sizes is not None else "no")


def store_components(result, results_basename):
    """ConnectedComponents.main's output files: results_basename.wcc = the component of every node and, when the result has sizes,
    results_basename.wccsizes = the size of every component, each as BinIO.storeLongs writes them (big-endian int64, no header).
    Returns the paths written."""
    paths = [results_basename + ".wcc"]
    np.asarray(result.component, dtype=">i8").tofile(paths[0])
    if result.sizes is not None:
        paths.append(results_basename + ".wccsizes")
        np.asarray(result.sizes, dtype=">i8").tofile(paths[1])
    return paths


def load_components(results_basename):
    """Reads back what store_components wrote (BinIO.loadLongs): (component, sizes or None) as native int64 arrays."""
    comp = np.fromfile(results_basename + ".wcc", dtype=">i8").astype(np.int64)
    sp = results_basename + ".wccsizes"
    sizes = np.fromfile(sp, dtype=">i8").astype(np.int64) if os.path.exists(sp) else None
    return comp, sizes


def components_arg_parser():
    """The command line of ConnectedComponents.main: basename [resultsBasename], -s/--sizes, -r/--renumber (the weak components
    of the graph are computed directly: no symmetric graph and no -t transpose are needed)."""
    import argparse
    ap = argparse.ArgumentParser(prog="components", description="Weakly connected components of a BVGraph, computed on the device.")
    ap.add_argument("-s", "--sizes", action="store_true", help="also store the component sizes (resultsBasename.wccsizes)")
    ap.add_argument("-r", "--renumber", action="store_true", help="renumber components by decreasing size (ties: smallest node first)")
    ap.add_argument("--device", type=int, default=0, help="the GPU to run on")
    ap.add_argument("basename", help="the basename of the graph")
    ap.add_argument("results_basename", nargs="?", default=None, help="the basename of the result files (default: the graph's basename)")
    return ap


def components_main(argv=None):
    """ConnectedComponents.main: loads basename, computes the components, writes resultsBasename.wcc (and .wccsizes with -s)."""
    args = components_arg_parser().parse_args(argv)
    out = args.results_basename or args.basename
    g = BVGraph.load(args.basename, device=args.device)
    try:
        r = g.connected_components(sizes=args.sizes, sort_by_size=args.renumber)
    finally:
        g.close()
    store_components(r, out)
    print("%d components" % r.count)
    return r


class SCCResult:
    """What StronglyConnectedComponents holds after compute(): numberOfComponents (count), component[] (int64 per node; numbered by
    smallest node, not in Tarjan's emission order), computeSizes() (sizes, or None), the buckets as one bool per node (or None:
    computeBuckets was false) and the counters of bvg_scc by name (SCC_COUNTERS)."""

    def __init__(self, count, component, sizes=None, buckets=None, counters=None):
        self.count, self.component, self.sizes, self.buckets, self.counters = int(count), component, sizes, buckets, counters or {}

    numberOfComponents = property(lambda self: self.count)

    def __repr__(self):
        return "SCCResult(count=%d, nodes=%d, sizes=%s, buckets=%s)" % (self.count, len(self.component), "yes" if self.sizes is not None else "no",
                                                                        "yes" if self.buckets is not None else "no")


def store_scc(result, results_basename):
    """StronglyConnectedComponents.main's output files: results_basename.scc = the component of every node and, when the result has
    sizes, results_basename.sccsizes = the size of every component, each as BinIO.storeLongs writes them (big-endian int64, no header).
    When the result has buckets, results_basename.bucketbits: ceil(n / 8) bytes, bit x & 7 of byte x >> 3 (the least significant bit
    first) set when node x is in a bucket.  The reference's .buckets is a Java-serialised LongArrayBitVector and is NOT written.
    Returns the paths written."""
    paths = [results_basename + ".scc"]
    np.asarray(result.component, dtype=">i8").tofile(paths[0])
    if result.sizes is not None:
        paths.append(results_basename + ".sccsizes")
        np.asarray(result.sizes, dtype=">i8").tofile(paths[-1])
    if result.buckets is not None:
        paths.append(results_basename + ".bucketbits")
        np.packbits(np.asarray(result.buckets, dtype=bool), bitorder="little").tofile(paths[-1])
    return paths


def _load_scc_sizes_buckets(results_basename, nodes):
    """(sizes or None, buckets or None) of results_basename.sccsizes / .bucketbits as store_scc writes them, each when the file exists."""
    sp, bp = results_basename + ".sccsizes", results_basename + ".bucketbits"
    sizes = np.fromfile(sp, dtype=">i8").astype(np.int64) if os.path.exists(sp) else None
    buckets = None
    if os.path.exists(bp):
        buckets = np.unpackbits(np.fromfile(bp, dtype=np.uint8), bitorder="little")[:nodes].astype(bool)
    return sizes, buckets


def load_scc(results_basename, nodes=None):
    """Reads back what store_scc wrote: (component, sizes or None, buckets or None) -- int64 arrays and one bool per node (nodes: the
    length of the bucket array; default: that of the component array)."""
    comp = np.fromfile(results_basename + ".scc", dtype=">i8").astype(np.int64)
    sizes, buckets = _load_scc_sizes_buckets(results_basename, len(comp) if nodes is None else nodes)
    return comp, sizes, buckets


def scc_arg_parser():
    """The command line of StronglyConnectedComponents.main: basename [resultsBasename], -s/--sizes, -r/--renumber, -b/--buckets."""
    import argparse
    ap = argparse.ArgumentParser(prog="scc", description="Strongly connected components of a BVGraph, computed on the device.")
    ap.add_argument("-s", "--sizes", action="store_true", help="also store the component sizes (resultsBasename.sccsizes)")
    ap.add_argument("-r", "--renumber", action="store_true", help="renumber components by decreasing size (ties: smallest node first)")
    ap.add_argument("-b", "--buckets", action="store_true", help="also store the buckets as a bit array (resultsBasename.bucketbits: n bits, LSB first)")
    ap.add_argument("--device", type=int, default=0, help="the GPU to run on")
    ap.add_argument("basename", help="the basename of the graph")
    ap.add_argument("results_basename", nargs="?", default=None, help="the basename of the result files (default: the graph's basename)")
    return ap


def scc_main(argv=None):
    """StronglyConnectedComponents.main: loads basename, computes the components, writes resultsBasename.scc (.sccsizes with -s,
    .bucketbits with -b: see store_scc)."""
    args = scc_arg_parser().parse_args(argv)
    out = args.results_basename or args.basename
    g = BVGraph.load(args.basename, device=args.device)
    try:
        r = g.strongly_connected_components(sizes=args.sizes, sort_by_size=args.renumber, buckets=args.buckets)
    finally:
        g.close()
    store_scc(r, out)
    print("%d components" % r.count)
    return r


def java_double_str(x):
    """Double.toString(x): the shortest digits that read back as x, in Java's layout -- plain decimal with at least one fractional digit
    for 10^-3 <= |x| < 10^7, d.dddE<n> otherwise."""
    from decimal import Decimal
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Infinity" if x > 0 else "-Infinity"
    sign = "-" if str(x).startswith("-") else ""
    a = abs(x)
    if a == 0:
        return sign + "0.0"
    d = Decimal(repr(a))
    ds = "".join(str(c) for c in d.as_tuple().digits).rstrip("0") or "0"
    e = d.adjusted()                                                       # a = d.ddd x 10^e
    if 1e-3 <= a < 1e7:
        if e >= 0:
            ds = ds.ljust(e + 1, "0")
            return sign + ds[:e + 1] + "." + (ds[e + 1:] or "0")
        return sign + "0." + "0" * (-e - 1) + ds
    return sign + ds[0] + "." + (ds[1:] or "0") + "E" + str(e)


def _big_decimal_div3(num, den):
    """new BigDecimal(num).divide(BigDecimal.valueOf(den), 3, RoundingMode.HALF_EVEN).toString() for a non-negative num (an int or a
    float, taken exactly as BigDecimal(double) does) and an int den > 0.  The quotient is formed with 2 400 digits: a tie at scale 3 is
    a terminating quotient (an exact double has at most ~1 075 digits), so it is exact there, and any other quotient of these operands
    lies further than 10^-400 from a tie, so cutting it cannot make one."""
    import decimal
    with decimal.localcontext() as c:
        c.prec = 2400
        return str((decimal.Decimal(num) / decimal.Decimal(den)).quantize(decimal.Decimal("0.001"), rounding=decimal.ROUND_HALF_EVEN))


class GraphStats:
    """What one pass of Stats.run counts (Stats.java:96-240): nodes, arcs, loops, dangling, terminal, num_gaps, tot_gap and tot_loc
    (Python ints), min / max outdegree and indegree with their nodes, log_delta (64 bins), outdegree_distribution and
    indegree_distribution (uint64 arrays of max degree + 1 entries) and, when asked for, indegrees (int64 per node; else None)."""

    FIELDS = ("nodes", "arcs", "loops", "dangling", "terminal", "num_gaps", "tot_gap", "tot_loc", "min_outdegree", "max_outdegree", "min_outdegree_node",
              "max_outdegree_node", "min_indegree", "max_indegree", "min_indegree_node", "max_indegree_node")

    def __init__(self, log_delta=None, outdegree_distribution=None, indegree_distribution=None, indegrees=None, **fields):
        unknown = set(fields) - set(self.FIELDS)
        if unknown:
            raise TypeError("unknown fields: %s" % sorted(unknown))
        for k in self.FIELDS:
            setattr(self, k, int(fields.get(k, (1 << 63) - 1 if k in ("min_outdegree", "min_indegree") else 0)))
        self.log_delta = [int(v) for v in (log_delta if log_delta is not None else [0] * 64)]
        self.log_delta += [0] * (64 - len(self.log_delta))
        self.outdegree_distribution = np.asarray(outdegree_distribution if outdegree_distribution is not None else [0], dtype=np.uint64)
        self.indegree_distribution = np.asarray(indegree_distribution if indegree_distribution is not None else [0], dtype=np.uint64)
        self.indegrees = indegrees

    @classmethod
    def from_summary(cls, sm, outdist, indist, indegrees=None):
        f = {k: int(getattr(sm, k)) for k in cls.FIELDS if k not in ("tot_gap", "tot_loc")}
        f["tot_gap"] = (int(sm.tot_gap_hi) << 64) | int(sm.tot_gap_lo)
        f["tot_loc"] = (int(sm.tot_loc_hi) << 64) | int(sm.tot_loc_lo)
        return cls([int(v) for v in sm.log_delta], outdist, indist, indegrees, **f)

    def __repr__(self):
        return "GraphStats(nodes=%d, arcs=%d, loops=%d, dangling=%d)" % (self.nodes, self.arcs, self.loops, self.dangling)

    def properties(self, buckets=None, scc_sizes=None):
        """The text of resultsBasename.stats: the reference's keys in its order (Stats.java:173-257).  buckets: the number of nodes in
        buckets, or one bool per node; scc_sizes: the size of every strongly connected component."""
        import math
        n = self.nodes
        div = lambda a, b: a / b if b else float("nan")                   # (Java: 0.0 / 0 is NaN)
        out = ["nodes=%d" % n, "arcs=%d" % self.arcs, "loops=%d" % self.loops,
               "successoravggap=" + _big_decimal_div3(self.tot_gap, max(1, self.num_gaps)),
               "avglocality=" + _big_decimal_div3(self.tot_loc, max(1, self.arcs)),
               "minoutdegree=%d" % self.min_outdegree, "maxoutdegree=%d" % self.max_outdegree,
               "minoutdegreenode=%d" % self.min_outdegree_node, "maxoutdegreenode=%d" % self.max_outdegree_node,
               "dangling=%d" % self.dangling, "terminal=%d" % self.terminal,
               "percdangling=" + java_double_str(div(100.0 * self.dangling, n)), "avgoutdegree=" + java_double_str(div(float(self.arcs), n))]
        last = max([i for i in range(64) if self.log_delta[i]], default=-1)
        tot, num, g = 0.0, 0, 1
        for i in range(last + 1):                                          # in double, in bin order (Stats.java:193-200); Fast.log2 is log(x) / log(2)
            num += self.log_delta[i]
            tot += (math.log(g * 2 + g + 1) / 0.6931471805599453 - 1) * self.log_delta[i]
            g *= 2
        out.append("successorlogdeltastats=" + ",".join(str(self.log_delta[i]) for i in range(last + 1)))
        out.append("successoravglogdelta=" + ("0" if num == 0 else _big_decimal_div3(tot, max(1, num * 2))))
        out += ["minindegree=%d" % self.min_indegree, "maxindegree=%d" % self.max_indegree, "minindegreenode=%d" % self.min_indegree_node,
                "maxindegreenode=%d" % self.max_indegree_node, "avgindegree=" + java_double_str(div(float(self.arcs), n))]
        if buckets is not None:
            nb = int(buckets) if np.ndim(buckets) == 0 else int(np.count_nonzero(buckets))
            out += ["buckets=%d" % nb, "percbuckets=" + java_double_str(div(100.0 * nb, n))]
        if scc_sizes is not None and len(scc_sizes):
            sz = np.sort(np.asarray(scc_sizes, dtype=np.int64))
            out += ["sccs=%d" % len(sz), "maxsccsize=%d" % sz[-1], "percmaxscc=" + java_double_str(div(100.0 * int(sz[-1]), n)),
                    "minsccsize=%d" % sz[0], "percminscc=" + java_double_str(div(100.0 * int(sz[0]), n))]
        return "".join(l + "\n" for l in out)


def _store_longs(values, path):
    """TextIO.storeLongs: one decimal per line."""
    with open(path, "w") as f:
        f.write("".join("%d\n" % int(v) for v in values))
    return path


def store_stats(stats, results_basename, buckets=None, scc_sizes=None, save_degrees=False, outdegrees=None):
    """Stats.run's output files: results_basename.stats (GraphStats.properties), .outdegree and .indegree (the distributions, one decimal
    per line, max degree + 1 lines), with scc_sizes .sccdistr (lines size<TAB>count, sizes descending, Stats.java:259-274) and with
    save_degrees .outdegrees (from `outdegrees`) and .indegrees (from stats.indegrees), one decimal per node.  Returns the paths."""
    paths = [results_basename + ".stats"]
    with open(paths[0], "w") as f:
        f.write(stats.properties(buckets=buckets, scc_sizes=scc_sizes))
    paths.append(_store_longs(stats.outdegree_distribution, results_basename + ".outdegree"))
    paths.append(_store_longs(stats.indegree_distribution, results_basename + ".indegree"))
    if scc_sizes is not None and len(scc_sizes):
        size, count = np.unique(np.asarray(scc_sizes, dtype=np.int64), return_counts=True)
        paths.append(results_basename + ".sccdistr")
        with open(paths[-1], "w") as f:
            f.write("".join("%d\t%d\n" % (int(s), int(c)) for s, c in zip(size[::-1], count[::-1])))
    if save_degrees:
        if outdegrees is None or stats.indegrees is None:
            raise IllegalArgumentException(_abi.E_ARG, "save_degrees needs the outdegrees and a GraphStats computed with indegrees=True")
        paths.append(_store_longs(outdegrees, results_basename + ".outdegrees"))
        paths.append(_store_longs(stats.indegrees, results_basename + ".indegrees"))
    return paths


def stats_arg_parser():
    """The command line of Stats.main: [-s] basename [resultsBasename]."""
    import argparse
    ap = argparse.ArgumentParser(prog="stats", description="Statistical data of a BVGraph, computed on the device: basename.stats, .outdegree, .indegree and, "
                                 "when basename.sccsizes exists, .sccdistr.  Buckets are read from basename.bucketbits (as the scc tool writes them): the "
                                 "reference's basename.buckets is a Java-serialised bit vector, which cannot be parsed here and is ignored.")
    ap.add_argument("-s", "--save-degrees", action="store_true", help="save indegrees and outdegrees in text format (resultsBasename.indegrees, .outdegrees)")
    ap.add_argument("--device", type=int, default=0, help="the GPU to run on")
    ap.add_argument("basename", help="the basename of the graph")
    ap.add_argument("results_basename", nargs="?", default=None, help="the basename of the result files (default: the graph's basename)")
    return ap


def stats_main(argv=None):
    """Stats.main: loads basename, makes the pass, writes the files of store_stats; basename.sccsizes and basename.bucketbits are used when
    they exist.  Returns the GraphStats."""
    args = stats_arg_parser().parse_args(argv)
    out = args.results_basename or args.basename
    g = BVGraph.load(args.basename, device=args.device)
    try:
        r = g.stats(indegrees=args.save_degrees)
        outdeg = g.outdegrees() if args.save_degrees else None
        n = g.num_nodes()
    finally:
        g.close()
    sizes, buckets = _load_scc_sizes_buckets(args.basename, n)                 # (load_scc's reader; the .scc labels themselves are not needed)
    store_stats(r, out, buckets=buckets, scc_sizes=sizes, save_degrees=args.save_degrees, outdegrees=outdeg)
    return r


class GeometricResult:
    """What LinearGeometricCentrality holds after compute(), for the sources [from, to): centrality (float32) and reachable (int64) per
    source, the distance histogram over those sources (uint64, or None) and the counters of bvg_geometric by name (GEO_COUNTERS).
    A result computed with ("power", 1) holds the sum of the distances from every source: closeness() and lin() derive the two
    centralities from it by the formulas of bvg_hyperball_centrality (HyperBall.main)."""

    def __init__(self, centrality, reachable, histogram=None, counters=None, sources=None, coefficients=None):
        self.centrality, self.reachable, self.histogram, self.counters = centrality, reachable, histogram, counters or {}
        self.sources = sources if sources is not None else (0, len(centrality))
        self.coefficients = coefficients

    def _sum_of_distances(self):
        if self.coefficients != (_abi.GEO_POWER_LAW, 1.0):
            raise IllegalStateException(_abi.E_STATE, 'closeness and Lin need the sum of distances: coefficients ("power", 1)')
        return np.asarray(self.centrality, dtype=np.float64)

    def closeness(self):
        """1 / (the sum of the distances), 0 where that sum is 0."""
        d = self._sum_of_distances()
        return np.where(d == 0, 0.0, 1.0 / np.where(d == 0, 1.0, d)).astype(np.float32)

    def lin(self):
        """reachable^2 / (the sum of the distances), 1 where that sum is 0."""
        d = self._sum_of_distances()
        r = np.asarray(self.reachable, dtype=np.float64)
        return np.where(d == 0, 1.0, r * r / np.where(d == 0, 1.0, d)).astype(np.float32)

    def neighbourhood_function(self):
        """The running sums of the histogram: the pairs (source, node) at distance at most t."""
        if self.histogram is None:
            raise IllegalStateException(_abi.E_STATE, "computed without histogram=True")
        return np.cumsum(self.histogram.astype(np.uint64))

    def __repr__(self):
        return "GeometricResult(sources=[%d, %d), histogram=%s)" % (self.sources[0], self.sources[1], "yes" if self.histogram is not None else "no")


_GEO_SPEC_PREFIX = "it.unimi.dsi.big.webgraph.algo.LinearGeometricCentrality"


def parse_coefficients_spec(spec):
    """The coefficientsSpec of LinearGeometricCentrality.main -- CLASSNAME or CLASSNAME(arg) -- as what linear_geometric_centrality
    takes: HarmonicCoefficients, PowerLawCoefficients(x), ExponentialCoefficients(x), bare or with the reference's class-name prefix
    (it.unimi.dsi.big.webgraph.algo.LinearGeometricCentrality$ or the same with a dot)."""
    import re
    m = re.fullmatch(r"\s*([A-Za-z_$.][\w$.]*?)\s*(?:\((.*)\))?\s*", spec)
    if not m:
        raise IllegalArgumentException(_abi.E_ARG, "malformed coefficients spec %r" % (spec,))
    name, args = m.group(1), m.group(2)
    for sep in ("$", "."):
        if name.startswith(_GEO_SPEC_PREFIX + sep):
            name = name[len(_GEO_SPEC_PREFIX) + 1:]
    argv = [] if args is None or not args.strip() else [a.strip() for a in args.split(",")]
    try:
        vals = [float(a) for a in argv]
    except ValueError:
        raise IllegalArgumentException(_abi.E_ARG, "malformed coefficients spec %r" % (spec,))
    if name == "HarmonicCoefficients" and not vals:
        return "harmonic"
    if name == "PowerLawCoefficients" and len(vals) == 1:
        return ("power", vals[0])
    if name == "ExponentialCoefficients" and len(vals) == 1:
        return ("exp", vals[0])
    raise IllegalArgumentException(_abi.E_ARG, "unknown coefficients class or arguments in %r" % (spec,))


def store_geometric(result, centrality_filename, reachable_filename):
    """LinearGeometricCentrality.main's output files: the centralities as BinIO.storeFloats writes them (big-endian float32) and the
    reachable counts as BinIO.storeLongs does (big-endian int64), no headers.  Returns the paths written."""
    np.asarray(result.centrality, dtype=">f4").tofile(centrality_filename)
    np.asarray(result.reachable, dtype=">i8").tofile(reachable_filename)
    return [centrality_filename, reachable_filename]


def load_geometric(centrality_filename, reachable_filename):
    """Reads back what store_geometric wrote: (centrality float32, reachable int64)."""
    return np.fromfile(centrality_filename, dtype=">f4").astype(np.float32), np.fromfile(reachable_filename, dtype=">i8").astype(np.int64)


def geometric_arg_parser():
    """The command line of LinearGeometricCentrality.main: [-m] [-T n] graphBasename coefficientsSpec centralityFilename reachableFilename."""
    import argparse
    ap = argparse.ArgumentParser(prog="geometric", description="Exact positive linear geometric centrality of a BVGraph, computed on the device.")
    ap.add_argument("-m", "--mapped", action="store_true", help="(accepted and ignored: the graph lives in device memory)")
    ap.add_argument("-T", "--threads", type=int, default=0, help="(accepted and ignored)")
    ap.add_argument("--device", type=int, default=0, help="the GPU to run on")
    ap.add_argument("graphBasename", help="the basename of the graph")
    ap.add_argument("coefficientsSpec", help="HarmonicCoefficients, PowerLawCoefficients(x) or ExponentialCoefficients(x)")
    ap.add_argument("centralityFilename", help="where the centrality scores are stored (big-endian floats)")
    ap.add_argument("reachableFilename", help="where the numbers of reachable nodes are stored (big-endian longs)")
    return ap


def geometric_main(argv=None):
    """LinearGeometricCentrality.main: loads graphBasename, computes the centrality of every node, writes the two files."""
    ap = geometric_arg_parser()
    args = ap.parse_args(argv)
    try:
        coeffs = parse_coefficients_spec(args.coefficientsSpec)
    except IllegalArgumentException as e:
        ap.error(str(e))
    g = BVGraph.load(args.graphBasename, device=args.device)
    try:
        r = g.linear_geometric_centrality(coeffs)
    finally:
        g.close()
    store_geometric(r, args.centralityFilename, args.reachableFilename)
    return r


def mosaic(graphs, cycles):
    """Synthetic workload helper (bvg_mosaic): the cycle of the given base graphs, back to back, repeated `cycles` times."""
    k = len(graphs)
    hs = (C.c_void_p * k)(*[g._h for g in graphs])
    h = C.c_void_p()
    _check(lib().bvg_mosaic(hs, k, cycles, C.byref(h)), "mosaic")
    return BVGraph(h)


def scan_multi(graphs, balance=BALANCE_ARCS):
    """bvg_scan_multi: graphs[i] scans shard i of len(graphs) on its own device, all at once; returns (total, [per shard])."""
    k = len(graphs)
    hs = (C.c_void_p * k)(*[g._h for g in graphs])
    tot = ScanResult(); per = (ScanResult * k)()
    _check(lib().bvg_scan_multi(hs, k, balance, C.byref(tot), per), "scan_multi")
    return tot.as_dict(), [p.as_dict() for p in per]


LABEL_GAMMA_INT, LABEL_FIXED_INT, LABEL_FIXED_INT_LIST, LABEL_FIXED_LONG_LIST = 1, 2, 3, 4


def parse_label_spec(spec):
    """Label.toSpec() text (e.g. "...labelling.FixedWidthIntLabel(FOO,10)") -> (kind, width)."""
    k, w = C.c_int(), C.c_int()
    _check(lib().bvg_labels_parse_spec(spec.encode() if isinstance(spec, str) else spec, C.byref(k), C.byref(w)), "labelspec %r" % (spec,))
    return k.value, w.value


class LabelledArcIterator(LazyLongIterator):
    """ArcLabelledNodeIterator.LabelledArcIterator (labelling/ArcLabelledNodeIterator.java): successors with label()."""

    def __init__(self, succ, labels):
        LazyLongIterator.__init__(self, succ)
        self._l = labels

    def label(self):
        """The label of the arc returned by the last next_long() (BitStreamArcLabelledImmutableGraph.java:250-252)."""
        if self._i == 0:
            raise IllegalStateException(_abi.E_STATE, "label() before nextLong()")
        return int(self._l[self._i - 1])


class BitStreamArcLabelledImmutableGraph:
    """labelling/BitStreamArcLabelledImmutableGraph.java: an underlying BVGraph plus one int label per arc, both decoded on the
    device (GammaCodedIntLabel / FixedWidthIntLabel)."""

    def __init__(self, graph, handle, keep=()):
        self.g = graph
        self._h = handle
        self._keep = keep

    @classmethod
    def load(cls, basename, device=0):
        """load(basename) (:378-484): basename.properties names the underlying graph and the label class."""
        buf = C.create_string_buffer(4096)
        _check(lib().bvg_labels_read_properties(os.fsencode(basename), None, None, buf, len(buf)), "load(%s)" % basename)
        under = os.fsdecode(buf.value)
        g = BVGraph.load(under, device)
        h = C.c_void_p()
        buf = C.create_string_buffer(4096)
        _check(lib().bvg_labels_open(os.fsencode(basename), g.num_nodes(), device, C.byref(h), buf, len(buf)), "load(%s)" % basename)
        return cls(g, h)

    @classmethod
    def from_memory(cls, graph, kind, width, stream, label_offsets, device=0):
        st = np.frombuffer(bytes(stream), dtype=np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, dtype=np.uint8)
        lo = np.ascontiguousarray(label_offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().bvg_labels_open_mem(kind, width, graph.num_nodes(), st.ctypes.data if len(st) else None, len(st), lo.ctypes.data, device, C.byref(h)), "labels_open_mem")
        return cls(graph, h)

    def close(self):
        if getattr(self, "_h", None):
            lib().bvg_labels_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_nodes(self):
        return self.g.num_nodes()

    def num_arcs(self):
        return self.g.num_arcs()

    def outdegree(self, x):
        return self.g.outdegree(x)

    def decode_range(self, frm, to):
        """(outdeg, successors, labels) of nodes [frm,to): one batch of the labelled node iterator (:565-582).
        EOFException if the label stream does not fit the graph's outdegrees, and if a gamma-coded label is 2^31 or more: the
        reference's readGamma() would wrap such a value to a negative int; it is refused here (include/bvgraph_hip.h)."""
        deg, succ = self.g.decode_range(frm, to)
        lab = np.empty(max(len(succ), 1), dtype=np.int32)
        n = C.c_uint64()
        d32 = np.ascontiguousarray(deg, dtype=np.int32)
        _check(lib().bvg_labels_decode_range(self._h, frm, to, d32.ctypes.data if len(d32) else None, lab.ctypes.data, len(succ), C.byref(n)), "labels(%d,%d)" % (frm, to))
        return deg, succ, lab[:len(succ)]

    def decode_range_lists(self, frm, to):
        """List labels (FixedWidthIntListLabel: int32 values; FixedWidthLongListLabel: int64): (outdeg, successors, list_off[arcs+1], values).
        EOFException as for decode_range; a gamma-coded list length of 2^31 or more is refused in the same way."""
        deg, succ = self.g.decode_range(frm, to)
        d32 = np.ascontiguousarray(deg, dtype=np.int32)
        loff = np.zeros(len(succ) + 1, dtype=np.uint64)
        n = C.c_uint64()
        kind = C.c_int(); width = C.c_int(); nn = C.c_int64(); sb = C.c_uint64()
        _check(lib().bvg_labels_info(self._h, C.byref(kind), C.byref(width), C.byref(nn), C.byref(sb)), "labels_info")
        fn, dt = (lib().bvg_labels_decode_range_lists64, np.int64) if kind.value == LABEL_FIXED_LONG_LIST else (lib().bvg_labels_decode_range_lists, np.int32)
        st = fn(self._h, frm, to, d32.ctypes.data if len(d32) else None, loff.ctypes.data, None, 0, C.byref(n))
        if st != _abi.E_CAPACITY:
            _check(st, "label lists(%d,%d)" % (frm, to))
        vals = np.empty(max(n.value, 1), dtype=dt)
        if n.value:
            _check(fn(self._h, frm, to, d32.ctypes.data, loff.ctypes.data, vals.ctypes.data, n.value, C.byref(n)), "label lists(%d,%d)" % (frm, to))
        return deg, succ, loff, vals[:n.value]

    def successors(self, x):
        """successors(x) (:208-229): a LabelledArcIterator."""
        if x < 0 or x >= self.num_nodes():
            raise IllegalArgumentException(_abi.E_ARG, "successors(%d)" % x)
        _, succ, lab = self.decode_range(x, x + 1)
        return LabelledArcIterator(succ, lab)
