// bvg_labelled.hip — arc-labelled graphs on the device: Transform.java's labelled half and BitStreamArcLabelledImmutableGraph.store, from a
// labelled CSR in HBM (bvg_lgraph: a bvg_text plus int32 labels[arcs] in successor order and the label class) to a labelled CSR in HBM.
// The contract is the one of include/bvgraph_hip.h ("Arc-labelled graphs").  Scalar int labels only: GammaCodedIntLabel, FixedWidthIntLabel.
//
// Every bvg_lgraph holds a CSR that launch_csr_check has passed (from_csr, from_labelled) or that a call here wrote from such CSRs, and labels
// checked against their class: the kernels below index with successors and never look at a label as anything but a value.
//
//   transpose  ONE stable radix sort by target (rocPRIM) of (target, arc index) over the bits of `nodes` in use; the arcs come in source order, so every
//              list of the result is sorted already.  A gather then writes, for every sorted position, the source (a binary search in the offsets: the
//              offsets are small and stay in L2, an expanded source array would be 8 more bytes written and read per arc) and the label.
//   union      ARC-PARALLEL, two passes, no atomics, no loop over a row.  Pass 1: every arc (x, y) of a finds by binary search in row x of b the
//              absolute position lb of the first successor >= y, and whether it is y; every arc of b does the same in a and is DROPPED when a has
//              it (its label reaches a's slot in pass 2).  An exclusive prefix sum of b's kept flags (kept[j] = kept arcs of b before j) then gives
//              every position in closed form, because a row of the result is all of a's row merged with b's kept arcs:
//                  result offset of x  = aoff[x] + kept[boff[x]]
//                  arc i of a          -> i + kept[lb_b(i)]            (a's arcs before it, b's kept arcs before its successor)
//                  kept arc j of b     -> lb_a(j) + kept[j]
//              so the prefix sum over the rows that Transform's per-node merge needs is the one over b's arcs.  Pass 2 writes successor and label;
//              a common arc gets merge(label_a, label_b), a's label first (UnionArcLabelledImmutableGraph.java:188).  A row of 10^6 arcs costs 10^6
//              binary searches spread over the grid, not one thread's walk.
//   symmetrize union(g, transpose(g)) (Transform.java:633-635).   filter: a keep flag per arc, a prefix sum, a compaction of successors and labels.
//   the label writer (BitStreamArcLabelledImmutableGraph.java:654-684): a code length per arc (gamma: 2 msb(v + 1) + 1 bits, fixed: width), an
//              exclusive 64-bit prefix sum = the bit position of every code, label_offsets[x] = the position of x's first arc.  Emission is by OUTPUT
//              WORD: the thread that owns 64 bits of the stream finds the first code that reaches into them (binary search over the positions),
//              ORs in every code up to the word's end and stores the word once, big-endian.  Deterministic, no atomics; width 1 is a loop of 64.
#include <cstdint>
#include <rocprim/device/device_radix_sort.hpp>

#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

constexpr uint64_t kMaxArcs = 0x7FFFFFFFull;        // what one prefix sum (launch_exclusive_scan) takes; positions below fit 31 bits + a flag
constexpr uint32_t kFound = 0x80000000u;

// the node of arc i: the last x with off[x] <= i (n > 0, i < off[n])
__device__ __forceinline__ int64_t arc_source(const uint64_t* off, int64_t n, uint64_t i) {
    int64_t l = 0, r = n;
    while (r - l > 1) { const int64_t m = (l + r) >> 1; if (off[m] <= i) l = m; else r = m; }
    return l;
}
// the first position of [lo, hi) whose successor is >= y
__device__ __forceinline__ uint64_t lower_bound(const int64_t* adj, uint64_t lo, uint64_t hi, int64_t y) {
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (adj[m] < y) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ int32_t merge_labels(int strategy, int32_t a, int32_t b) {
    return strategy == BVG_LMERGE_KEEP_FIRST ? a : strategy == BVG_LMERGE_MIN ? (a < b ? a : b) : (a > b ? a : b);
}

// ---- labels against their class: gamma >= 0 (GammaCodedIntLabel.java:49), fixed 0 <= v < 2^width (FixedWidthIntLabel.java:41-42, :56); width <= 31
__global__ void check_labels_kernel(const int32_t* lab, uint64_t m, int kind, int width, unsigned* bad) {
    bool b = false;
    BVG_FOR(i, m) { const uint32_t v = (uint32_t)lab[i]; b |= kind == BVG_LABEL_GAMMA_INT ? v > 0x7FFFFFFFu : (v >> width) != 0; }
    if (b) atomicOr(bad, 1u);
}
__global__ void degrees_kernel(const uint64_t* off, int64_t n, int32_t* deg) {
    BVG_FOR(x, n) deg[x] = (int32_t)(off[x + 1] - off[x]);
}

// ---- transpose
__global__ void arc_index_kernel(uint64_t m, uint32_t* idx) { BVG_FOR(i, m) idx[i] = (uint32_t)i; }
__global__ void transpose_gather_kernel(const uint64_t* off, int64_t n, const int32_t* lab, const uint32_t* idx, uint64_t m, int64_t* tadj, int32_t* tlab) {
    BVG_FOR(j, m) { const uint32_t i = idx[j]; tadj[j] = arc_source(off, n, i); tlab[j] = lab[i]; }
}
// toff[y] = the arcs with a target below y: the lower bound of y in the sorted targets
__global__ void transpose_offsets_kernel(const uint64_t* keys, uint64_t m, int64_t n, uint64_t* toff) {
    BVG_FOR(y, n + 1) {
        uint64_t l = 0, r = m;
        while (l < r) { const uint64_t mid = (l + r) >> 1; if (keys[mid] < (uint64_t)y) l = mid + 1; else r = mid; }
        toff[y] = l;
    }
}

// ---- union (file comment).  One side: its offsets and successors, the node count it really has (rows beyond are empty) and its arc count.
struct Side { const uint64_t* off; const int64_t* adj; const int32_t* lab; int64_t n; uint64_t m; };
// pass 1 over the arcs of `s`: lb[i] = the position in `o` of the first successor of the same row that is >= the arc's (o.m when o lacks the row),
// with kFound set when o has the arc; keep (b's side only): 0 for an arc that a has too
__global__ void __launch_bounds__(256) union_search_kernel(Side s, Side o, uint32_t* lb, int32_t* keep) {
    BVG_FOR(i, s.m) {
        const int64_t x = arc_source(s.off, s.n, (uint64_t)i), y = s.adj[i];
        uint64_t p = o.m; bool found = false;
        if (x < o.n) { const uint64_t hi = o.off[x + 1]; p = lower_bound(o.adj, o.off[x], hi, y); found = p < hi && o.adj[p] == y; }
        lb[i] = (uint32_t)p | (found ? kFound : 0u);
        if (keep) keep[i] = !found;
    }
}
__global__ void union_offsets_kernel(Side a, Side b, const uint64_t* kept, int64_t n, uint64_t* out) {
    BVG_FOR(x, n + 1) out[x] = a.off[x < a.n ? x : a.n] + kept[b.off[x < b.n ? x : b.n]];
}
__global__ void __launch_bounds__(256) union_write_a_kernel(Side a, Side b, const uint32_t* lb, const uint64_t* kept, int strategy, int64_t* adj, int32_t* lab) {
    BVG_FOR(i, a.m) {
        const uint32_t w = lb[i], p = w & ~kFound;
        const uint64_t at = (uint64_t)i + kept[p];
        adj[at] = a.adj[i];
        lab[at] = (w & kFound) ? merge_labels(strategy, a.lab[i], b.lab[p]) : a.lab[i];
    }
}
__global__ void __launch_bounds__(256) union_write_b_kernel(Side b, const uint32_t* lb, const uint64_t* kept, int64_t* adj, int32_t* lab) {
    BVG_FOR(j, b.m) {
        const uint32_t w = lb[j];
        if (w & kFound) continue;
        const uint64_t at = (uint64_t)w + kept[j];
        adj[at] = b.adj[j]; lab[at] = b.lab[j];
    }
}

// ---- filter
__global__ void filter_keep_kernel(const uint64_t* off, const int64_t* adj, const int32_t* lab, int64_t n, uint64_t m, int kind, const int64_t* cls, int64_t bound, int32_t* keep) {
    BVG_FOR(i, m) {
        if (kind == BVG_LFILTER_LOWER_BOUND) { keep[i] = (int64_t)lab[i] >= bound; continue; }            // Transform.java:213: >=
        const int64_t x = arc_source(off, n, (uint64_t)i), y = adj[i];
        keep[i] = kind == BVG_LFILTER_NO_LOOPS ? x != y : (cls[x] == cls[y]) == (kind == BVG_LFILTER_SAME_CLASS);
    }
}
__global__ void filter_compact_kernel(const int64_t* adj, const int32_t* lab, const int32_t* keep, const uint64_t* pos, uint64_t m, int64_t* oadj, int32_t* olab) {
    BVG_FOR(i, m) if (keep[i]) { const uint64_t p = pos[i]; oadj[p] = adj[i]; olab[p] = lab[i]; }
}
// out[x] = at[off[x]]: the offsets of a node-wise view of a per-arc prefix sum (the filter's kept arcs, the writer's bit positions)
__global__ void offsets_at_kernel(const uint64_t* off, const uint64_t* at, int64_t n, uint64_t* out) {
    BVG_FOR(x, n + 1) out[x] = at[off[x]];
}

// ---- the label writer
__global__ void code_lengths_kernel(const int32_t* lab, uint64_t m, int kind, int width, int32_t* len) {
    BVG_FOR(i, m) len[i] = kind == BVG_LABEL_GAMMA_INT ? 2 * (31 - __clz((uint32_t)lab[i] + 1u)) + 1 : width;   // label >= 0: label + 1 <= 2^31
}
// word w of the stream = bits [64 w, 64 w + 64), most significant first; pos[m + 1] = the bit position of every code (strictly increasing: every
// code of a stream that has words at all is at least one bit long).  A code is the integer label + 1 (gamma: msb zeros, then msb + 1 bits) or
// the label (fixed) in its pos[k + 1] - pos[k] <= 63 bits.  out holds `words` 64-bit words.
__global__ void __launch_bounds__(256) emit_words_kernel(const int32_t* lab, const uint64_t* pos, uint64_t m, int kind, uint64_t words, uint64_t* out) {
    BVG_FOR(w, words) {
        const uint64_t w0 = (uint64_t)w << 6, w1 = w0 + 64;
        uint64_t l = 0, r = m;                                              // the last k with pos[k] <= w0 (pos[0] = 0)
        while (r - l > 1) { const uint64_t mid = (l + r) >> 1; if (pos[mid] <= w0) l = mid; else r = mid; }
        uint64_t word = 0;
        for (uint64_t k = l; k < m; k++) {
            const uint64_t s = pos[k];
            if (s >= w1) break;
            const unsigned len = (unsigned)(pos[k + 1] - s);                  // 1..63
            const uint64_t code = ((uint64_t)(uint32_t)lab[k] + (kind == BVG_LABEL_GAMMA_INT ? 1u : 0u)) << (64u - len);   // left-aligned
            word |= s >= w0 ? code >> (s - w0) : code << (w0 - s);            // (w0 - s < len <= 63)
        }
        out[w] = __builtin_bswap64(word);
    }
}

bool scalar_kind(int kind) { return kind == BVG_LABEL_GAMMA_INT || kind == BVG_LABEL_FIXED_INT; }
bool list_kind(int kind) { return kind == BVG_LABEL_FIXED_INT_LIST || kind == BVG_LABEL_FIXED_LONG_LIST; }
// the refusals of a label class that need no device: 0, BVG_E_UNSUPPORTED (lists), BVG_E_ARG
int check_class(int kind, int width) {
    if (list_kind(kind)) return BVG_E_UNSUPPORTED;
    if (!scalar_kind(kind)) return BVG_E_ARG;
    if (kind == BVG_LABEL_FIXED_INT && (width < 0 || width > 31)) return BVG_E_ARG;
    return 0;
}

Side side_of(const bvg_lgraph* l) { return Side{l->g->d_off.get(), l->g->d_adj, l->d_lab.get(), l->g->nodes, l->g->arcs}; }

std::unique_ptr<bvg_lgraph> new_lgraph(const bvg_lgraph* like, int device) {
    std::unique_ptr<bvg_lgraph> l(new bvg_lgraph);
    l->g = new_csr(device); l->kind = like->kind; l->width = like->width;
    return l;
}
int finish(std::unique_ptr<bvg_lgraph>& l, bvg_lgraph** out) {
    HIPCHK(hipDeviceSynchronize());
    *out = l.release();
    return 0;
}
int alloc_arcs(bvg_lgraph* l, uint64_t m) {
    if (l->g->adj_base.alloc((size_t)m) || l->d_lab.alloc((size_t)m)) return BVG_E_NOMEM;
    l->g->d_adj = l->g->adj_base; l->g->arcs = m;
    return 0;
}

// 0, or BVG_E_ARG when a label is outside its class
int check_labels(const int32_t* d_lab, uint64_t m, int kind, int width) {
    if (!m) return 0;
    DevArray<unsigned> bad;
    if (bad.alloc(1)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(bad.get(), 0, sizeof(unsigned)));
    hipLaunchKernelGGL(check_labels_kernel, dim3(grid((int64_t)m, 256)), dim3(256), 0, 0, d_lab, m, kind, width, bad.get());
    unsigned hb = 0;
    HIPCHK(hipMemcpy(&hb, bad.get(), sizeof hb, hipMemcpyDeviceToHost));
    return hb ? BVG_E_ARG : 0;
}

int from_csr_entry(int64_t nodes, const void* adj_off, const void* adj, const void* labels, int kind, int width, int device, bvg_lgraph** out, bool dev) {
    if (!out || !adj_off || nodes < 0) return BVG_E_ARG;
    int rc = check_class(kind, width); if (rc) return rc;
    return guarded([&]() -> int {
        bvg_text* raw = nullptr;                                             // the CSR exactly as the unlabelled path takes and refuses it
        int rc = dev ? bvg_transform_from_csr_dev(nodes, adj_off, adj, device, &raw) : bvg_transform_from_csr(nodes, (const uint64_t*)adj_off, (const int64_t*)adj, device, &raw);
        if (rc) return rc;
        std::unique_ptr<bvg_lgraph> l(new bvg_lgraph);
        l->g.reset(raw); l->kind = kind; l->width = kind == BVG_LABEL_FIXED_INT ? width : 0;
        const uint64_t m = raw->arcs;
        if (m > kMaxArcs) return BVG_E_UNSUPPORTED;
        if (m && !labels) return BVG_E_ARG;
        HIPCHK(hipSetDevice(device));
        if (l->d_lab.alloc((size_t)m)) return BVG_E_NOMEM;
        if (m) HIPCHK(hipMemcpy(l->d_lab.get(), labels, (size_t)m * sizeof(int32_t), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        rc = check_labels(l->d_lab.get(), m, l->kind, l->width); if (rc) return rc;
        return finish(l, out);
    });
}

int transpose_lgraph(const bvg_lgraph* src, std::unique_ptr<bvg_lgraph>& out) {
    const Side s = side_of(src);
    if (s.m > kMaxArcs) return BVG_E_UNSUPPORTED;
    std::unique_ptr<bvg_lgraph> t = new_lgraph(src, src->g->device);
    t->g->nodes = s.n;
    if (t->g->d_off.alloc((size_t)s.n + 1)) return BVG_E_NOMEM;
    int rc = alloc_arcs(t.get(), s.m); if (rc) return rc;
    if (!s.m) { HIPCHK(hipMemset(t->g->d_off.get(), 0, ((size_t)s.n + 1) * sizeof(uint64_t))); out = std::move(t); return 0; }
    DevArray<uint64_t> keys; DevArray<uint32_t> idx0, idx1; DevArray<uint8_t> temp;
    if (keys.alloc((size_t)s.m) || idx0.alloc((size_t)s.m) || idx1.alloc((size_t)s.m)) return BVG_E_NOMEM;
    const unsigned bits = s.n > 1 ? 64u - (unsigned)__builtin_clzll((unsigned long long)(s.n - 1)) : 1u;   // the bits of `nodes` in use
    hipLaunchKernelGGL(arc_index_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.m, idx0.get());
    size_t sb = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, sb, (const uint64_t*)s.adj, keys.get(), (const uint32_t*)idx0.get(), idx1.get(), (size_t)s.m, 0u, bits, (hipStream_t)0));
    if (temp.alloc(sb)) return BVG_E_NOMEM;
    HIPCHK(rocprim::radix_sort_pairs(temp.get(), sb, (const uint64_t*)s.adj, keys.get(), (const uint32_t*)idx0.get(), idx1.get(), (size_t)s.m, 0u, bits, (hipStream_t)0));
    hipLaunchKernelGGL(transpose_gather_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.off, s.n, s.lab, (const uint32_t*)idx1.get(), s.m, t->g->d_adj, t->d_lab.get());
    hipLaunchKernelGGL(transpose_offsets_kernel, dim3(grid(s.n + 1, 256)), dim3(256), 0, 0, (const uint64_t*)keys.get(), s.m, s.n, t->g->d_off.get());
    HIPCHK(hipDeviceSynchronize());
    out = std::move(t);
    return 0;
}

int union_lgraph(const bvg_lgraph* la, const bvg_lgraph* lb, int strategy, std::unique_ptr<bvg_lgraph>& out) {
    const Side a = side_of(la), b = side_of(lb);
    if (a.m > kMaxArcs || b.m > kMaxArcs) return BVG_E_UNSUPPORTED;
    const int64_t n = a.n > b.n ? a.n : b.n;
    std::unique_ptr<bvg_lgraph> t = new_lgraph(la, la->g->device);
    t->g->nodes = n;
    DevArray<uint32_t> lba, lbb; DevArray<int32_t> keep; DevArray<uint64_t> kept, tmp;
    const size_t mb = (size_t)(b.m ? b.m : 1);
    if (t->g->d_off.alloc((size_t)n + 1) || lba.alloc((size_t)a.m) || lbb.alloc(mb) || keep.alloc(mb) || kept.alloc(mb + 1) || tmp.alloc(scan_tmp_elems((int64_t)mb))) return BVG_E_NOMEM;
    HIPCHK(hipMemset(kept.get(), 0, (mb + 1) * sizeof(uint64_t)));
    uint64_t kept_b = 0;
    if (a.m) hipLaunchKernelGGL(union_search_kernel, dim3(grid((int64_t)a.m, 256)), dim3(256), 0, 0, a, b, lba.get(), (int32_t*)nullptr);
    if (b.m) {
        hipLaunchKernelGGL(union_search_kernel, dim3(grid((int64_t)b.m, 256)), dim3(256), 0, 0, b, a, lbb.get(), keep.get());
        launch_exclusive_scan(keep.get(), kept.get(), (int64_t)b.m, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&kept_b, kept.get() + b.m, sizeof kept_b, hipMemcpyDeviceToHost));
    }
    const uint64_t total = a.m + kept_b;
    if (total > kMaxArcs) return BVG_E_UNSUPPORTED;
    const int rc = alloc_arcs(t.get(), total); if (rc) return rc;
    hipLaunchKernelGGL(union_offsets_kernel, dim3(grid(n + 1, 256)), dim3(256), 0, 0, a, b, (const uint64_t*)kept.get(), n, t->g->d_off.get());
    if (a.m) hipLaunchKernelGGL(union_write_a_kernel, dim3(grid((int64_t)a.m, 256)), dim3(256), 0, 0, a, b, (const uint32_t*)lba.get(), (const uint64_t*)kept.get(), strategy, t->g->d_adj, t->d_lab.get());
    if (b.m) hipLaunchKernelGGL(union_write_b_kernel, dim3(grid((int64_t)b.m, 256)), dim3(256), 0, 0, b, (const uint32_t*)lbb.get(), (const uint64_t*)kept.get(), t->g->d_adj, t->d_lab.get());
    HIPCHK(hipDeviceSynchronize());
    out = std::move(t);
    return 0;
}

int filter_lgraph(const bvg_lgraph* src, int kind, const int64_t* d_cls, int64_t bound, std::unique_ptr<bvg_lgraph>& out) {
    const Side s = side_of(src);
    if (s.m > kMaxArcs) return BVG_E_UNSUPPORTED;
    std::unique_ptr<bvg_lgraph> t = new_lgraph(src, src->g->device);
    t->g->nodes = s.n;
    DevArray<int32_t> keep; DevArray<uint64_t> pos, tmp;
    const size_t mm = (size_t)(s.m ? s.m : 1);
    if (t->g->d_off.alloc((size_t)s.n + 1) || keep.alloc(mm) || pos.alloc(mm + 1) || tmp.alloc(scan_tmp_elems((int64_t)mm))) return BVG_E_NOMEM;
    HIPCHK(hipMemset(pos.get(), 0, (mm + 1) * sizeof(uint64_t)));
    uint64_t kept = 0;
    if (s.m) {
        hipLaunchKernelGGL(filter_keep_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.off, s.adj, s.lab, s.n, s.m, kind, d_cls, bound, keep.get());
        launch_exclusive_scan(keep.get(), pos.get(), (int64_t)s.m, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&kept, pos.get() + s.m, sizeof kept, hipMemcpyDeviceToHost));
    }
    const int rc = alloc_arcs(t.get(), kept); if (rc) return rc;
    if (s.m) {
        hipLaunchKernelGGL(filter_compact_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.adj, s.lab, (const int32_t*)keep.get(), (const uint64_t*)pos.get(), s.m, t->g->d_adj, t->d_lab.get());
        hipLaunchKernelGGL(offsets_at_kernel, dim3(grid(s.n + 1, 256)), dim3(256), 0, 0, s.off, (const uint64_t*)pos.get(), s.n, t->g->d_off.get());
    } else HIPCHK(hipMemset(t->g->d_off.get(), 0, ((size_t)s.n + 1) * sizeof(uint64_t)));
    HIPCHK(hipDeviceSynchronize());
    out = std::move(t);
    return 0;
}

// the stream (8 * words bytes, the last word zero-padded) and the nodes + 1 label offsets, both on the device; *bits = the length of the stream
int write_labels(const bvg_lgraph* l, DevArray<uint64_t>& stream, DevArray<uint64_t>& loff, uint64_t* bits) {
    const Side s = side_of(l);
    if (s.m > kMaxArcs) return BVG_E_UNSUPPORTED;
    *bits = 0;
    if (loff.alloc((size_t)s.n + 1)) return BVG_E_NOMEM;
    if (!s.m || (l->kind == BVG_LABEL_FIXED_INT && l->width == 0)) {       // no arcs, or codes of no bits: an empty stream, offsets all zero
        HIPCHK(hipMemset(loff.get(), 0, ((size_t)s.n + 1) * sizeof(uint64_t)));
        return stream.alloc(0);
    }
    DevArray<int32_t> len; DevArray<uint64_t> pos, tmp;
    if (len.alloc((size_t)s.m) || pos.alloc((size_t)s.m + 1) || tmp.alloc(scan_tmp_elems((int64_t)s.m))) return BVG_E_NOMEM;
    hipLaunchKernelGGL(code_lengths_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.lab, s.m, l->kind, l->width, len.get());
    launch_exclusive_scan(len.get(), pos.get(), (int64_t)s.m, tmp.get(), nullptr);
    HIPCHK(hipMemcpy(bits, pos.get() + s.m, sizeof *bits, hipMemcpyDeviceToHost));
    const uint64_t words = (*bits + 63) >> 6;
    if (stream.alloc((size_t)words)) return BVG_E_NOMEM;
    hipLaunchKernelGGL(offsets_at_kernel, dim3(grid(s.n + 1, 256)), dim3(256), 0, 0, s.off, (const uint64_t*)pos.get(), s.n, loff.get());
    hipLaunchKernelGGL(emit_words_kernel, dim3(grid((int64_t)words, 256)), dim3(256), 0, 0, s.lab, (const uint64_t*)pos.get(), s.m, l->kind, words, stream.get());
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

template <typename F> int on_lgraph(const bvg_lgraph* l, F&& f) {
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(l->g->device));
        int rc = f();
        if (hipDeviceSynchronize() != hipSuccess && !rc) { (void)hipGetLastError(); rc = BVG_E_HIP; }
        return rc;
    });
}

int lgraph_get(bvg_lgraph* l, void* adj_off, uint64_t off_cap, void* adj, uint64_t adj_cap, void* labels, uint64_t lab_cap, hipMemcpyKind kind) {
    if (!l) return BVG_E_ARG;
    const bvg_text* t = l->g.get();
    if ((adj_off && off_cap < (uint64_t)t->nodes + 1) || (adj && adj_cap < t->arcs) || (labels && lab_cap < t->arcs)) return BVG_E_CAPACITY;   // nothing is written
    HIPCHK(hipSetDevice(t->device));
    if (adj_off) HIPCHK(hipMemcpy(adj_off, t->d_off, ((size_t)t->nodes + 1) * sizeof(uint64_t), kind));
    if (adj && t->arcs) HIPCHK(hipMemcpy(adj, t->d_adj, (size_t)t->arcs * sizeof(int64_t), kind));
    if (labels && t->arcs) HIPCHK(hipMemcpy(labels, l->d_lab.get(), (size_t)t->arcs * sizeof(int32_t), kind));
    return 0;
}

bool strategy_ok(int s) { return s == BVG_LMERGE_KEEP_FIRST || s == BVG_LMERGE_MIN || s == BVG_LMERGE_MAX; }

}  // namespace
}  // namespace bvghost

extern "C" {

int bvg_lgraph_from_csr(int64_t nodes, const uint64_t* adj_off, const int64_t* adj, const int32_t* labels, int kind, int width, int device, bvg_lgraph** out) {
    return from_csr_entry(nodes, adj_off, adj, labels, kind, width, device, out, false);
}
int bvg_lgraph_from_csr_dev(int64_t nodes, const void* d_adj_off, const void* d_adj, const void* d_labels, int kind, int width, int device, bvg_lgraph** out) {
    return from_csr_entry(nodes, d_adj_off, d_adj, d_labels, kind, width, device, out, true);
}

int bvg_lgraph_from_labelled(bvg_graph* g, bvg_labels* labels, bvg_lgraph** out) {
    if (!out || !g || !labels) return BVG_E_ARG;
    if (list_kind(labels->kind)) return BVG_E_UNSUPPORTED;
    if (!scalar_kind(labels->kind)) return BVG_E_ARG;
    if (labels->kind == BVG_LABEL_FIXED_INT && labels->width > 31) return BVG_E_UNSUPPORTED;   // 32 bits: values that are no int >= 0 (FixedWidthIntLabel.java:41-42 stops at 31)
    if (g->sh->device != labels->device || g->sh->p.nodes != labels->nodes || g->node_base != 0) return BVG_E_ARG;
    return guarded([&]() -> int {
        bvg_transform_src src{g, nullptr};
        Source s;
        int rc = resolve(&src, s); if (rc) return rc;                        // decoded once and checked, as the unlabelled transforms take a bvg_graph
        if (s.m > kMaxArcs) return BVG_E_UNSUPPORTED;
        std::unique_ptr<bvg_lgraph> l(new bvg_lgraph);
        l->g = std::move(s.own); l->kind = labels->kind; l->width = labels->kind == BVG_LABEL_FIXED_INT ? labels->width : 0;
        const int64_t n = l->g->nodes; const uint64_t m = l->g->arcs;
        if (l->d_lab.alloc((size_t)m)) return BVG_E_NOMEM;
        if (m) {
            DevArray<int32_t> deg;
            if (deg.alloc((size_t)n)) return BVG_E_NOMEM;
            hipLaunchKernelGGL(degrees_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, (const uint64_t*)l->g->d_off.get(), n, deg.get());
            HIPCHK(hipDeviceSynchronize());
            // bvg_labels_decode_range_dev sums the outdegrees of one call in one prefix sum: ranges of at most 2^30 nodes
            for (int64_t lo = 0; lo < n; lo += kMaxBatchNodes) {
                const int64_t hi = lo + kMaxBatchNodes < n ? lo + kMaxBatchNodes : n;
                uint64_t at = 0, got = 0;
                HIPCHK(hipMemcpy(&at, l->g->d_off.get() + lo, sizeof at, hipMemcpyDeviceToHost));
                rc = bvg_labels_decode_range_dev(labels, lo, hi, deg.get() + lo, l->d_lab.get() + at, m - at, &got); if (rc) return rc;
            }
        }
        return finish(l, out);
    });
}

int bvg_lgraph_info(const bvg_lgraph* l, int64_t* nodes, uint64_t* arcs, int* kind, int* width) {
    if (!l) return BVG_E_ARG;
    if (nodes) *nodes = l->g->nodes;
    if (arcs) *arcs = l->g->arcs;
    if (kind) *kind = l->kind;
    if (width) *width = l->width;
    return 0;
}

int bvg_lgraph_get(bvg_lgraph* l, uint64_t* adj_off, uint64_t off_cap, int64_t* adj, uint64_t adj_cap, int32_t* labels, uint64_t labels_cap) {
    return lgraph_get(l, adj_off, off_cap, adj, adj_cap, labels, labels_cap, hipMemcpyDeviceToHost);
}
int bvg_lgraph_get_dev(bvg_lgraph* l, void* d_adj_off, uint64_t off_cap, void* d_adj, uint64_t adj_cap, void* d_labels, uint64_t labels_cap) {
    return lgraph_get(l, d_adj_off, off_cap, d_adj, adj_cap, d_labels, labels_cap, hipMemcpyDeviceToDevice);
}

int bvg_lgraph_underlying(const bvg_lgraph* l, bvg_text** out) {
    if (!out || !l) return BVG_E_ARG;
    return on_lgraph(l, [&]() -> int {
        const bvg_text* g = l->g.get();
        std::unique_ptr<bvg_text> t = new_csr(g->device);
        t->nodes = g->nodes; t->arcs = g->arcs;
        if (t->d_off.alloc((size_t)g->nodes + 1) || t->adj_base.alloc((size_t)g->arcs)) return BVG_E_NOMEM;
        t->d_adj = t->adj_base;
        HIPCHK(hipMemcpy(t->d_off.get(), g->d_off.get(), ((size_t)g->nodes + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice));
        if (g->arcs) HIPCHK(hipMemcpy(t->d_adj, g->d_adj, (size_t)g->arcs * sizeof(int64_t), hipMemcpyDeviceToDevice));
        return bvghost::finish(t, out);
    });
}

void bvg_lgraph_close(bvg_lgraph* l) { delete l; }

int bvg_lgraph_transpose(const bvg_lgraph* src, bvg_lgraph** out) {
    if (!out || !src) return BVG_E_ARG;
    return on_lgraph(src, [&]() -> int {
        std::unique_ptr<bvg_lgraph> t;
        const int rc = transpose_lgraph(src, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_lgraph_union(const bvg_lgraph* a, const bvg_lgraph* b, int strategy, bvg_lgraph** out) {
    if (!out || !a || !b || !strategy_ok(strategy)) return BVG_E_ARG;
    if (a->kind != b->kind || a->width != b->width || a->g->device != b->g->device) return BVG_E_ARG;
    return on_lgraph(a, [&]() -> int {
        std::unique_ptr<bvg_lgraph> t;
        const int rc = union_lgraph(a, b, strategy, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_lgraph_symmetrize(const bvg_lgraph* src, int strategy, bvg_lgraph** out) {
    if (!out || !src || !strategy_ok(strategy)) return BVG_E_ARG;
    return on_lgraph(src, [&]() -> int {
        std::unique_ptr<bvg_lgraph> tr, t;
        int rc = transpose_lgraph(src, tr); if (rc) return rc;
        rc = union_lgraph(src, tr.get(), strategy, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_lgraph_filter(const bvg_lgraph* src, int kind, const int64_t* node_class, int64_t class_len, int64_t lower_bound, bvg_lgraph** out) {
    if (!out || !src || class_len < 0) return BVG_E_ARG;
    if (kind != BVG_LFILTER_NO_LOOPS && kind != BVG_LFILTER_SAME_CLASS && kind != BVG_LFILTER_DIFFERENT_CLASS && kind != BVG_LFILTER_LOWER_BOUND) return BVG_E_ARG;
    const bool classes = kind == BVG_LFILTER_SAME_CLASS || kind == BVG_LFILTER_DIFFERENT_CLASS;
    if (classes ? (!node_class && class_len) : (node_class != nullptr || class_len != 0)) return BVG_E_ARG;
    if (kind != BVG_LFILTER_LOWER_BOUND && lower_bound != 0) return BVG_E_ARG;
    if (classes && class_len != src->g->nodes) return BVG_E_ARG;
    return on_lgraph(src, [&]() -> int {
        DevArray<int64_t> cls;
        if (classes) {
            if (cls.alloc((size_t)class_len)) return BVG_E_NOMEM;
            if (class_len) HIPCHK(hipMemcpy(cls.get(), node_class, (size_t)class_len * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        std::unique_ptr<bvg_lgraph> t;
        const int rc = filter_lgraph(src, kind, classes ? cls.get() : nullptr, lower_bound, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_lgraph_store_labels(const bvg_lgraph* l, uint8_t** stream, uint64_t* nbytes, uint64_t** label_offsets) {
    if (!l || !stream || !nbytes || !label_offsets) return BVG_E_ARG;
    return on_lgraph(l, [&]() -> int {
        DevArray<uint64_t> d_stream, d_loff; uint64_t bits = 0;
        const int rc = write_labels(l, d_stream, d_loff, &bits); if (rc) return rc;
        const uint64_t nb = (bits + 7) >> 3; const size_t n1 = (size_t)l->g->nodes + 1;
        HostArray<uint8_t> hs((uint8_t*)calloc((size_t)nb + 16, 1)); HostArray<uint64_t> ho((uint64_t*)malloc(n1 * sizeof(uint64_t)));
        if (!hs || !ho) return BVG_E_NOMEM;
        if (nb) HIPCHK(hipMemcpy(hs.get(), d_stream.get(), (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ho.get(), d_loff.get(), n1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
        *stream = hs.release(); *nbytes = nb; *label_offsets = ho.release();
        return 0;
    });
}

int bvg_lgraph_store_labels_dev(const bvg_lgraph* l, void* d_stream, uint64_t cap, uint64_t* nbytes, void* d_label_offsets) {
    if (!l || !nbytes) return BVG_E_ARG;
    return on_lgraph(l, [&]() -> int {
        DevArray<uint64_t> stream, loff; uint64_t bits = 0;
        const int rc = write_labels(l, stream, loff, &bits); if (rc) return rc;
        const uint64_t nb = (bits + 7) >> 3;
        *nbytes = nb;
        if (nb > cap || (nb && !d_stream)) return BVG_E_CAPACITY;            // nothing is written
        if (nb) HIPCHK(hipMemcpy(d_stream, stream.get(), (size_t)nb, hipMemcpyDeviceToDevice));
        if (d_label_offsets) HIPCHK(hipMemcpy(d_label_offsets, loff.get(), ((size_t)l->g->nodes + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice));
        return 0;
    });
}

}  // extern "C"
