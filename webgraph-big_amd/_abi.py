"""ctypes mirror of include/bvgraph_hip.h (struct layouts + status codes)."""
import ctypes as C


class Params(C.Structure):
    """bvg_params (include/bvgraph_hip.h)."""
    _fields_ = [("nodes", C.c_int64), ("arcs", C.c_int64), ("window_size", C.c_int32), ("max_ref_count", C.c_int32),
                ("min_interval_length", C.c_int32), ("zeta_k", C.c_int32), ("outdegree_coding", C.c_int32),
                ("block_coding", C.c_int32), ("residual_coding", C.c_int32), ("reference_coding", C.c_int32),
                ("block_count_coding", C.c_int32), ("offset_coding", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def clone(self, **kw):
        p = Params()
        C.memmove(C.byref(p), C.byref(self), C.sizeof(Params))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class ScanResult(C.Structure):
    """bvg_scan_result."""
    _fields_ = [("nodes", C.c_uint64), ("arcs", C.c_uint64), ("chk", C.c_uint64), ("graph_bytes", C.c_uint64),
                ("index_bytes", C.c_uint64), ("kernel_ms", C.c_double), ("launches", C.c_uint32), ("slow_blocks", C.c_uint32),
                ("index_entries", C.c_uint64), ("lean_blocks", C.c_uint32), ("reserved0", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Tuning(C.Structure):
    """bvg_tuning."""
    _fields_ = [("block_bits", C.c_uint32), ("force_wide", C.c_uint32), ("force_slow", C.c_uint32), ("reserved", C.c_uint32), ("no_index", C.c_uint32)]


DELTA, GAMMA, GOLOMB, SKEWED_GOLOMB, UNARY, ZETA, NIBBLE = 1, 2, 3, 4, 5, 6, 7
LOAD_OFFLINE, LOAD_SEQUENTIAL, LOAD_STANDARD, LOAD_MAPPED = -1, 0, 1, 2

# bvg_bfs_create flags / the number of words bvg_bfs_counters writes (BVG_BFS_PARENT, BVG_BFS_COUNTERS)
BFS_PARENT_FLAG, BFS_COUNTER_WORDS = 1, 8


def bfs_signatures():
    """argtypes of the bvg_bfs_* entry points (breadth-first visits), by name."""
    vp, i64, u64, pp = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p)
    return {"bvg_bfs_create": [vp, C.c_uint32, pp], "bvg_bfs_close": [vp], "bvg_bfs_clear": [vp], "bvg_bfs_visit": [vp, i64, C.POINTER(u64)],
            "bvg_bfs_visit_all": [vp], "bvg_bfs_info": [vp, C.POINTER(i64), C.POINTER(u64), C.POINTER(u64)],
            "bvg_bfs_get": [vp, vp, vp, u64, vp, u64, vp], "bvg_bfs_get_dev": [vp, vp, vp, u64, vp, u64, vp], "bvg_bfs_counters": [vp, vp]}


# bvg_hyperball_create flags and the `which` of bvg_hyperball_centrality (BVG_HB_*, BVG_HB_WHICH_*)
HB_SUM_OF_DISTANCES_FLAG, HB_HARMONIC_FLAG = 1, 2
HB_WHICH = {"sum_of_distances": 0, "harmonic": 1, "closeness": 2, "lin": 3, "nieminen": 4, "reachable": 5}


def hyperball_signatures():
    """argtypes of the bvg_hyperball_* entry points, by name."""
    vp, i64, u64, pp, dbl = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_double
    return {"bvg_hyperball_create": [vp, C.c_int, C.c_uint32, u64, pp], "bvg_hyperball_close": [vp], "bvg_hyperball_init": [vp, u64],
            "bvg_hyperball_iterate": [vp], "bvg_hyperball_run": [vp, i64, dbl],
            "bvg_hyperball_info": [vp, C.POINTER(i64), C.POINTER(u64), C.POINTER(dbl), C.POINTER(u64)],
            "bvg_hyperball_neighbourhood_function": [vp, vp, u64], "bvg_hyperball_registers": [vp, i64, i64, vp],
            "bvg_hyperball_counts": [vp, i64, i64, vp], "bvg_hyperball_counts_dev": [vp, i64, i64, vp],
            "bvg_hyperball_centrality": [vp, C.c_int, vp], "bvg_hyperball_centrality_dev": [vp, C.c_int, vp],
            "bvg_hyperball_relative_standard_deviation": [C.c_int]}


# bvg_scc flags / the number of words it writes to `counters` (BVG_SCC_SORT_BY_SIZE, BVG_SCC_BUCKETS, BVG_SCC_COUNTERS)
SCC_SORT_BY_SIZE_FLAG, SCC_BUCKETS_FLAG, SCC_COUNTER_WORDS = 1, 2, 8


def scc_signatures():
    """argtypes of bvg_scc / bvg_scc_dev (strongly connected components), by name."""
    vp, u64 = C.c_void_p, C.c_uint64
    args = [vp, C.c_uint32, vp, vp, u64, C.POINTER(u64), vp, vp]
    return {"bvg_scc": list(args), "bvg_scc_dev": list(args)}


# the `kind` of bvg_geometric (BVG_GEO_HARMONIC, ...) / the number of words it writes to `counters` (BVG_GEO_COUNTERS)
GEO_HARMONIC, GEO_POWER_LAW, GEO_EXPONENTIAL, GEO_TABLE, GEO_COUNTER_WORDS = 0, 1, 2, 3, 8


def geometric_signatures():
    """argtypes of bvg_geometric / bvg_geometric_dev (exact geometric centralities), by name."""
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    args = [vp, C.c_int, C.c_double, vp, u64, i64, i64, vp, vp, vp, u64, C.POINTER(u64), vp]
    return {"bvg_geometric": list(args), "bvg_geometric_dev": list(args)}


# bvg_stats_compute flags and the `which` of bvg_stats_distribution (BVG_STATS_KEEP_INDEGREES, BVG_STATS_OUT, BVG_STATS_IN)
STATS_KEEP_INDEGREES_FLAG, STATS_OUT, STATS_IN = 1, 0, 1


class StatsSummary(C.Structure):
    """bvg_stats_summary (82 x 8 = 656 bytes)."""
    _fields_ = ([(k, C.c_uint64) for k in ("nodes", "arcs", "loops", "dangling", "terminal", "num_gaps", "tot_gap_lo", "tot_gap_hi", "tot_loc_lo", "tot_loc_hi")]
                + [(k, C.c_int64) for k in ("min_outdegree", "max_outdegree", "min_outdegree_node", "max_outdegree_node",
                                            "min_indegree", "max_indegree", "min_indegree_node", "max_indegree_node")]
                + [("log_delta", C.c_uint64 * 64)])


def stats_signatures():
    """argtypes of the bvg_stats_* entry points (graph statistics), by name."""
    vp, i64, u64, pp = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p)
    return {"bvg_stats_compute": [vp, C.c_uint32, pp], "bvg_stats_close": [vp], "bvg_stats_get": [vp, C.POINTER(StatsSummary)],
            "bvg_stats_distribution": [vp, C.c_int, vp, u64, C.POINTER(u64)], "bvg_stats_indegrees": [vp, i64, i64, vp],
            "bvg_stats_indegrees_dev": [vp, i64, i64, vp]}


class EFParams(C.Structure):
    """bvg_ef_params (32 bytes)."""
    _fields_ = [("nodes", C.c_int64), ("arcs", C.c_int64), ("upper_bound", C.c_int64), ("log2_quantum", C.c_int32), ("big_endian", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def ef_signatures():
    """argtypes of the bvg_ef_* entry points (EFGraph), by name."""
    vp, i64, u64, pp, ci = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_int
    P = C.POINTER(EFParams)
    return {"bvg_ef_parse_properties": [C.c_char_p, C.c_size_t, P], "bvg_ef_derive_offsets": [P, vp, u64, vp],
            "bvg_ef_open": [C.c_char_p, ci, ci, pp], "bvg_ef_open_mem": [P, vp, u64, vp, ci, pp], "bvg_ef_open_dev": [P, vp, u64, vp, ci, pp],
            "bvg_ef_copy": [vp, pp], "bvg_ef_close": [vp], "bvg_ef_info": [vp, P], "bvg_ef_get_offsets": [vp, vp],
            "bvg_ef_outdegrees": [vp, i64, i64, vp], "bvg_ef_decode_range": [vp, i64, i64, vp, vp, u64, C.POINTER(u64)],
            "bvg_ef_decode_range_dev": [vp, i64, i64, vp, vp, u64, C.POINTER(u64)],
            "bvg_ef_successors_batch": [vp, vp, i64, vp, vp, u64, C.POINTER(u64)], "bvg_ef_scan": [vp, i64, i64, C.POINTER(ScanResult)],
            "bvg_ef_skip_to_batch": [vp, vp, vp, i64, vp], "bvg_ef_last_kernel_ms": [vp, C.POINTER(C.c_double)],
            "bvg_ef_store": [i64, i64, ci, ci, vp, vp, ci, pp, C.POINTER(u64), pp]}


class TextError(C.Structure):
    """bvg_text_error (24 bytes)."""
    _fields_ = [("byte", C.c_uint64), ("line", C.c_int64), ("reason", C.c_int32), ("reserved", C.c_int32)]


# bvg_text_error.reason (BVG_TEXT_BAD_BYTE ...), the `kind` of bvg_text_format_csr and the flags of bvg_text_parse_arcs
TEXT_REASONS = {1: "bad_byte", 2: "bad_header", 3: "too_large", 4: "not_node", 5: "not_increasing", 6: "shift_range", 7: "arc_fields", 8: "eof"}
TEXT_ASCII, TEXT_ARCS = 0, 1
TEXT_SYMMETRIZE_FLAG, TEXT_NO_LOOPS_FLAG = 1, 2


def text_signatures():
    """argtypes of the bvg_text_* entry points (ASCIIGraph and arc lists, both ways), by name."""
    vp, i64, u64, pp, ci, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.c_uint32
    E, N = C.POINTER(TextError), C.POINTER(C.c_uint64)
    return {"bvg_text_parse_ascii": [vp, u64, ci, pp, E], "bvg_text_parse_ascii_dev": [vp, u64, ci, pp, E],
            "bvg_text_parse_arcs": [vp, u64, i64, u32, i64, ci, pp, E], "bvg_text_parse_arcs_dev": [vp, u64, i64, u32, i64, ci, pp, E],
            "bvg_text_close": [vp], "bvg_text_info": [vp, C.POINTER(i64), N], "bvg_text_get": [vp, vp, u64, vp, u64], "bvg_text_get_dev": [vp, vp, u64, vp, u64],
            "bvg_text_store": [vp, C.POINTER(Params), i64, pp, N, pp],
            "bvg_text_format_ascii": [vp, i64, i64, vp, u64, N], "bvg_text_format_ascii_dev": [vp, i64, i64, vp, u64, N],
            "bvg_text_format_arcs": [vp, i64, i64, i64, vp, u64, N], "bvg_text_format_arcs_dev": [vp, i64, i64, i64, vp, u64, N],
            "bvg_text_format_csr": [ci, i64, i64, vp, vp, i64, vp, u64, N]}


class ScatteredReport(C.Structure):
    """bvg_scattered_report (104 bytes): what bvg_scattered_parse saw in the text."""
    _fields_ = ([(k, C.c_uint64) for k in ("lines", "arcs", "bad_source", "bad_target", "no_target", "too_large", "trailing", "unknown_source", "unknown_target",
                                           "dropped_loops", "first_byte")]
                + [("first_line", C.c_int64), ("first_reason", C.c_int32), ("reserved", C.c_int32)])

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["first_reason"] = SCATTERED_REASONS.get(d["first_reason"])
        return d


# bvg_scattered_report.first_reason and, under TEXT_STRICT_FLAG, bvg_text_error.reason (BVG_SCATTERED_BAD_SOURCE ...); the flag itself (BVG_TEXT_STRICT)
SCATTERED_REASONS = {1: "bad_source", 2: "bad_target", 3: "no_target", 4: "too_large", 5: "trailing", 6: "unknown_source", 7: "unknown_target"}
TEXT_STRICT_FLAG = 4


def scattered_signatures():
    """argtypes of the bvg_scattered_* entry points (arc lists of arbitrary identifiers), by name."""
    vp, i64, u64, pp, ci, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.c_uint32
    args = [vp, u64, u32, vp, i64, ci, pp, C.POINTER(ScatteredReport), C.POINTER(TextError)]
    return {"bvg_scattered_parse": list(args), "bvg_scattered_parse_dev": list(args), "bvg_scattered_ids": [vp, vp, u64], "bvg_scattered_ids_dev": [vp, vp, u64]}


class TransformSrc(C.Structure):
    """bvg_transform_src: exactly one of the two handles is set."""
    _fields_ = [("graph", C.c_void_p), ("csr", C.c_void_p)]


# the `kind` of bvg_transform_filter and of bvg_transform_permutation, the flag of bvg_transform_symmetrize / _union
TRANSFORM_NO_LOOPS, TRANSFORM_SAME_CLASS, TRANSFORM_DIFFERENT_CLASS = 0, 1, 2
PERM_LEX, PERM_GRAY, PERM_RANDOM = 0, 1, 2
TRANSFORM_DROP_LOOPS_FLAG = 1


def transform_signatures():
    """argtypes of the bvg_transform_* entry points (Transform), by name."""
    vp, i64, u64, pp, ci, u32 = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.c_uint32
    S = C.POINTER(TransformSrc)
    return {"bvg_transform_from_csr": [i64, vp, vp, ci, pp], "bvg_transform_from_csr_dev": [i64, vp, vp, ci, pp], "bvg_transform_identity": [S, pp],
            "bvg_transform_map": [S, vp, i64, pp], "bvg_transform_map_dev": [S, vp, i64, pp],
            "bvg_transform_filter": [S, ci, vp, i64, pp], "bvg_transform_filter_dev": [S, ci, vp, i64, pp],
            "bvg_transform_transpose": [S, pp], "bvg_transform_symmetrize": [S, u32, pp], "bvg_transform_union": [S, S, u32, pp],
            "bvg_transform_permutation": [S, ci, u64, vp], "bvg_transform_permutation_dev": [S, ci, u64, vp]}


class ComposeReport(C.Structure):
    """bvg_compose_report (64 bytes): what bvg_compose did with the rows."""
    _fields_ = [("products", C.c_uint64), ("arcs", C.c_uint64), ("rows", C.c_uint64 * 3), ("limit", C.c_uint64 * 2), ("batches", C.c_uint64)]

    def as_dict(self):
        return {"products": int(self.products), "arcs": int(self.arcs), "rows": [int(v) for v in self.rows], "limit": [int(v) for v in self.limit], "batches": int(self.batches)}


def compose_signatures():
    """argtypes of bvg_compose, by name (a function of its own: transform_signatures() is the set of the bvg_transform_* names)."""
    S = C.POINTER(TransformSrc)
    return {"bvg_compose": [S, S, C.POINTER(ComposeReport), C.POINTER(C.c_void_p)]}


# the merge strategies of bvg_lgraph_union / _symmetrize and the `kind` of bvg_lgraph_filter (BVG_LMERGE_*, BVG_LFILTER_*)
LMERGE_KEEP_FIRST, LMERGE_MIN, LMERGE_MAX = 0, 1, 2
LFILTER_NO_LOOPS, LFILTER_SAME_CLASS, LFILTER_DIFFERENT_CLASS, LFILTER_LOWER_BOUND = 0, 1, 2, 3


def labelled_signatures():
    """argtypes of the bvg_lgraph_* entry points (arc-labelled graphs on the device), by name."""
    vp, i64, u64, pp, ci = C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p), C.c_int
    N = C.POINTER(u64)
    return {"bvg_lgraph_from_csr": [i64, vp, vp, vp, ci, ci, ci, pp], "bvg_lgraph_from_csr_dev": [i64, vp, vp, vp, ci, ci, ci, pp],
            "bvg_lgraph_from_labelled": [vp, vp, pp], "bvg_lgraph_close": [vp],
            "bvg_lgraph_info": [vp, C.POINTER(i64), N, C.POINTER(ci), C.POINTER(ci)],
            "bvg_lgraph_get": [vp, vp, u64, vp, u64, vp, u64], "bvg_lgraph_get_dev": [vp, vp, u64, vp, u64, vp, u64],
            "bvg_lgraph_underlying": [vp, pp], "bvg_lgraph_transpose": [vp, pp], "bvg_lgraph_union": [vp, vp, ci, pp],
            "bvg_lgraph_symmetrize": [vp, ci, pp], "bvg_lgraph_filter": [vp, ci, vp, i64, i64, pp],
            "bvg_lgraph_store_labels": [vp, pp, N, pp], "bvg_lgraph_store_labels_dev": [vp, vp, u64, N, vp]}


# the semirings of bvg_lcompose (BVG_SEMIRING_<ADD>_<MULTIPLY>)
SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS, SEMIRING_MAX_MIN, SEMIRING_MIN_MAX, SEMIRING_PLUS_TIMES = 0, 1, 2, 3, 4


class LComposeReport(C.Structure):
    """bvg_lcompose_report (88 bytes): bvg_compose_report's fields, then the range refusal's."""
    _fields_ = [("products", C.c_uint64), ("arcs", C.c_uint64), ("rows", C.c_uint64 * 3), ("limit", C.c_uint64 * 2), ("batches", C.c_uint64),
                ("out_of_range", C.c_uint64), ("first_row", C.c_int64), ("first_successor", C.c_int64)]

    def as_dict(self):
        return {"products": int(self.products), "arcs": int(self.arcs), "rows": [int(v) for v in self.rows], "limit": [int(v) for v in self.limit], "batches": int(self.batches),
                "out_of_range": int(self.out_of_range), "first_row": int(self.first_row), "first_successor": int(self.first_successor)}


def lcompose_signatures():
    """argtypes of bvg_lcompose, by name (a group of its own: labelled_signatures() is the set of the bvg_lgraph_* names)."""
    vp, ci = C.c_void_p, C.c_int
    return {"bvg_lcompose": [vp, vp, ci, ci, C.POINTER(LComposeReport), C.POINTER(C.c_void_p)]}


OK, E_ARG, E_STATE, E_UNSUPPORTED, E_IO, E_EOF, E_NOMEM, E_HIP, E_CAPACITY = 0, -1, -2, -3, -4, -5, -6, -7, -8


def default_params(**kw):
    """BVGraph defaults (BVGraph.java:455-473, 527-542)."""
    p = Params(nodes=0, arcs=-1, window_size=7, max_ref_count=3, min_interval_length=4, zeta_k=3,
               outdegree_coding=GAMMA, block_coding=GAMMA, residual_coding=ZETA, reference_coding=UNARY,
               block_count_coding=GAMMA, offset_coding=GAMMA)
    for k, v in kw.items():
        setattr(p, k, v)
    return p
