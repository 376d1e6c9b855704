// bvg_transform.hip — Transform.java on the device: map, filter, transpose, symmetrise, union and the lex / Gray / random permutations, every
// one from a CSR in HBM to a CSR in HBM (bvg_text, the handle of the text graphs).  The contract is the one of include/bvgraph_hip.h
// ("Transform").
//
// A SOURCE is a bvg_text, used where it lies, or a bvg_graph, decoded once (outdegrees, prefix sum, bvg_decode_range_dev) and checked as
// bvg_store checks its input.  The graph-valued calls are then short:
//   map        one (map[x], map[y]) pair per arc, a deleted end turning the pair into the dropped one, and the pairs -> CSR stage of the
//              arc lists (pairs_to_csr, bvg_text.hip): two stable radix sorts, duplicates flagged, a prefix sum;
//   filter     a keep flag per arc, a prefix sum, a compaction; adj_off[x] = the kept arcs before the first of x;
//   transpose  transpose_pairs (bvg_transpose.hip);  union: the per-node merge of bvg_transpose.hip over offsets padded to the common node
//              count;  symmetrise = union(g, transpose(g)), and DROP_LOOPS is the NO_LOOPS filter behind it.
//
// THE LEX / GRAY ORDER is a sort of the nodes by their successor lists, in two stages:
//   1  a HEAD KEY per node: the first k = 64 / b successors, b = bits of n, one b-bit code each, most significant first.  The code of a
//      position turns the comparator's rule there into an unsigned order -- where a list that ends goes first and otherwise the larger
//      successor, end = 0 and v = n - v; at the odd positions of the Gray order, where the smaller successor goes first and the end last,
//      v = v and end = n; behind the end, zeros.  One stable radix sort of (head, node) over the k b bits that are used orders every pair of
//      nodes whose lists differ inside the head, and leaves nodes with equal heads in node order: when the lists END inside the head they
//      are equal, and node order is the tie rule.
//   2  what is left are runs of equal heads of lists that go on behind position k.  Their positions are compacted and sorted by a merge
//      sort (rocPRIM device_merge_sort) whose comparator looks at the heads first -- so every run stays in its own slots -- then walks the
//      two lists from position k, then compares the node ids.  The sorted nodes go back into the slots in order.
// A comparison costs the common prefix of its two lists behind the head, so the work is (n' log n') comparisons for the n' nodes of stage 2
// times the prefixes they share; nothing depends on the longest prefix in rounds.  DESIGN.md 7j has the reasons and the measurements.
#include <cstdint>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>

#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

constexpr uint64_t kMaxElems = 0x7FFFFFFFull;      // what one prefix sum (launch_exclusive_scan) takes
constexpr int64_t kMaxMapped = 1ll << 40;          // node counts beyond: adj_off alone would not fit any device

unsigned bits_of(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 1u; }

// the node of arc i: the last x with off[x] <= i
__device__ __forceinline__ int64_t arc_source(const uint64_t* off, int64_t n, uint64_t i) {
    int64_t l = 0, r = n;
    while (r - l > 1) { const int64_t m = (l + r) >> 1; if (off[m] <= i) l = m; else r = m; }
    return l;
}

// ---- map
// out[0] = max(map) + 1 (0 when every entry is -1), out[1] != 0 when a value is below -1
__global__ void map_check_kernel(const int64_t* map, int64_t n, unsigned long long* out) {
    unsigned long long top = 0; bool bad = false;
    BVG_FOR(x, n) { const int64_t v = map[x]; if (v < -1) bad = true; else if ((unsigned long long)(v + 1) > top) top = (unsigned long long)(v + 1); }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(top, d, 64); top = o > top ? o : top; }
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(out, top);
    if (bad) atomicOr(out + 1, 1ull);
}
__global__ void map_pairs_kernel(const uint64_t* off, const int64_t* adj, int64_t n, uint64_t m, const int64_t* map, uint64_t drop, uint64_t* src, uint64_t* dst) {
    BVG_FOR(i, m) {
        const int64_t s = map[arc_source(off, n, (uint64_t)i)], t = map[adj[i]];
        const bool gone = s < 0 || t < 0;
        src[i] = gone ? drop : (uint64_t)s; dst[i] = gone ? drop : (uint64_t)t;
    }
}

// ---- filter
__global__ void filter_keep_kernel(const uint64_t* off, const int64_t* adj, int64_t n, uint64_t m, int kind, const int64_t* cls, int32_t* keep) {
    BVG_FOR(i, m) {
        const int64_t x = arc_source(off, n, (uint64_t)i), y = adj[i];
        keep[i] = kind == BVG_TRANSFORM_NO_LOOPS ? x != y : (cls[x] == cls[y]) == (kind == BVG_TRANSFORM_SAME_CLASS);
    }
}
__global__ void filter_compact_kernel(const int64_t* adj, const int32_t* keep, const uint64_t* pos, uint64_t m, int64_t* out) {
    BVG_FOR(i, m) if (keep[i]) out[pos[i]] = adj[i];
}
__global__ void filter_off_kernel(const uint64_t* off, const uint64_t* pos, int64_t n, uint64_t* out) {   // pos[m] = the arcs kept
    BVG_FOR(x, n + 1) out[x] = pos[off[x]];
}

// ---- union: offsets of a graph of n_src nodes as those of one of n >= n_src nodes (the tail nodes have no successors)
__global__ void pad_off_kernel(const uint64_t* off, int64_t n_src, int64_t n, uint64_t* out) {
    BVG_FOR(x, n + 1) out[x] = off[x < n_src ? x : n_src];
}

// ---- permutations
struct ListOrder {
    const uint64_t* off; const int64_t* adj; int64_t n; bool gray; int k; unsigned b;
    // the head key of node x (file comment, stage 1)
    __device__ __forceinline__ uint64_t head(int64_t x) const {
        const uint64_t lo = off[x], len = off[x + 1] - lo;
        uint64_t key = 0;
        for (int p = 0; p < k; p++) {
            const bool parity = gray && (p & 1);
            uint64_t code = 0;
            if ((uint64_t)p < len) { const uint64_t v = (uint64_t)adj[lo + p]; code = parity ? v : (uint64_t)n - v; }
            else if ((uint64_t)p == len) code = parity ? (uint64_t)n : 0;
            key = key << b | code;
        }
        return key;
    }
    // node x before node y, their lists being equal up to position k (Transform.java:1946-1975 and :2017-2032 from there on; equal lists by node id)
    __device__ __forceinline__ bool tail_before(int64_t x, int64_t y) const {
        const uint64_t xo = off[x], yo = off[y], xl = off[x + 1] - xo, yl = off[y + 1] - yo;
        for (uint64_t p = (uint64_t)k;; p++) {
            const bool xe = p >= xl, ye = p >= yl, parity = gray && (p & 1);
            if (xe && ye) return x < y;
            if (xe) return !parity;
            if (ye) return parity;
            const int64_t a = adj[xo + p], c = adj[yo + p];
            if (a != c) return parity ? a < c : a > c;
        }
    }
};
__global__ void perm_heads_kernel(ListOrder o, uint64_t* head, uint32_t* node) {
    BVG_FOR(x, o.n) { head[x] = o.head(x); node[x] = (uint32_t)x; }
}
// position i of the head-sorted order needs stage 2: its list goes on behind the head and a neighbour has the same head
__global__ void perm_open_kernel(ListOrder o, const uint64_t* head, const uint32_t* node, int32_t* open) {
    BVG_FOR(i, o.n) {
        const int64_t x = node[i];
        const bool more = o.off[x + 1] - o.off[x] >= (uint64_t)o.k;
        open[i] = more && ((i > 0 && head[i - 1] == head[i]) || (i + 1 < o.n && head[i + 1] == head[i]));
    }
}
__global__ void perm_slots_kernel(const int32_t* open, const uint64_t* pos, int64_t n, uint32_t* slot) {
    BVG_FOR(i, n) if (open[i]) slot[pos[i]] = (uint32_t)i;
}
// the comparator of stage 2, over positions of the head-sorted order
struct OpenBefore {
    ListOrder o; const uint64_t* head; const uint32_t* node;
    __host__ __device__ __forceinline__ bool operator()(const uint32_t& i, const uint32_t& j) const {
#if defined(__HIP_DEVICE_COMPILE__)
        if (head[i] != head[j]) return head[i] < head[j];
        return o.tail_before((int64_t)node[i], (int64_t)node[j]);
#else
        return i < j;
#endif
    }
};
// sorted[j] (a position) holds the node that belongs at position slot[j]
__global__ void perm_place_kernel(const uint32_t* sorted, const uint32_t* slot, uint64_t count, const uint32_t* node, uint32_t* placed) {
    BVG_FOR(j, count) placed[slot[j]] = node[sorted[j]];
}
__global__ void perm_random_kernel(uint64_t seed, int64_t n, uint64_t* key, uint32_t* node) {
    BVG_FOR(x, n) {
        uint64_t z = seed + ((uint64_t)x + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        key[x] = z ^ (z >> 31); node[x] = (uint32_t)x;
    }
}
__global__ void perm_invert_kernel(const uint32_t* node, int64_t n, int64_t* perm) {   // perm[the node at rank r] = r
    BVG_FOR(r, n) perm[node[r]] = r;
}

}  // namespace

// ---- sources (Source, and the functions outside the unnamed namespaces here, are declared in bvg_host.h: bvg_compose.hip uses them too)
bool one_source(const bvg_transform_src* s) { return s && (s->graph != nullptr) != (s->csr != nullptr); }
int source_device(const bvg_transform_src* s) { return s->csr ? s->csr->device : s->graph->sh->device; }

std::unique_ptr<bvg_text> new_csr(int device) { std::unique_ptr<bvg_text> t(new bvg_text); t->device = device; return t; }

// 0, or `refused` when the CSR is not one bvg_store would take
int check_csr(const uint64_t* d_off, const int64_t* d_adj, int64_t n, int refused) {
    DevArray<unsigned> bad;
    if (bad.alloc(1)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(bad.get(), 0, sizeof(unsigned)));
    launch_csr_check(d_off, d_adj, n, bad.get(), nullptr);
    unsigned hb = 0;
    HIPCHK(hipMemcpy(&hb, bad.get(), sizeof hb, hipMemcpyDeviceToHost));
    return hb ? refused : 0;
}

namespace {

int64_t source_nodes(const bvg_transform_src* s) { return s->csr ? s->csr->nodes : s->graph->sh->p.nodes; }

int decode_graph(bvg_graph* g, std::unique_ptr<bvg_text>& out) {
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range
    const Shared* sh = g->sh;
    const int64_t n = sh->p.nodes;
    HIPCHK(hipSetDevice(sh->device));
    std::unique_ptr<bvg_text> t = new_csr(sh->device);
    t->nodes = n;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    DevArray<int32_t> deg; DevArray<uint64_t> tmp;
    if (deg.alloc(nn) || t->d_off.alloc(nn + 1) || tmp.alloc(scan_tmp_elems((int64_t)nn))) return BVG_E_NOMEM;
    HIPCHK(hipMemsetAsync(t->d_off.get(), 0, (nn + 1) * sizeof(uint64_t), g->stream));
    uint64_t m = 0;
    if (n > 0) {
        outdegrees_of(g, 0, n, deg.get());
        launch_exclusive_scan(deg.get(), t->d_off.get(), n, tmp.get(), g->stream);
        HIPCHK(hipMemcpyAsync(&m, t->d_off.get() + n, sizeof m, hipMemcpyDeviceToHost, g->stream));
    }
    HIPCHK(hipStreamSynchronize(g->stream));
    if (t->adj_base.alloc((size_t)m)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base; t->arcs = m;
    if (m) { uint64_t got = 0; const int rc = bvg_decode_range_dev(g, 0, n, nullptr, t->d_adj, m, &got); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(g->stream));
    const int rc = check_csr(t->d_off, t->d_adj, n, BVG_E_EOF);   // a successor outside [0, n), a list that does not increase: a malformed stream
    if (rc) return rc;
    out = std::move(t);
    return 0;
}

}  // namespace

int resolve(const bvg_transform_src* s, Source& r) {
    if (s->graph) {
        const int rc = decode_graph(s->graph, r.own); if (rc) return rc;
        r.device = r.own->device; r.n = r.own->nodes; r.m = r.own->arcs; r.off = r.own->d_off; r.adj = r.own->d_adj;
    } else {
        const bvg_text* t = s->csr;
        HIPCHK(hipSetDevice(t->device));
        r.device = t->device; r.n = t->nodes; r.m = t->arcs; r.off = t->d_off; r.adj = t->d_adj;
    }
    return 0;
}

int finish(std::unique_ptr<bvg_text>& t, bvg_text** out) {
    HIPCHK(hipDeviceSynchronize());
    *out = t.release();
    return 0;
}

namespace {

// a caller's array of `count` int64 on the device: the array itself (_dev), or a copy
int on_device_i64(const void* p, int64_t count, bool dev, DevArray<int64_t>& hold, const int64_t** out) {
    if (dev) { *out = (const int64_t*)p; return 0; }
    if (hold.alloc((size_t)count)) return BVG_E_NOMEM;
    if (count) HIPCHK(hipMemcpy(hold.get(), p, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice));
    *out = hold.get();
    return 0;
}

// ---- the transforms, CSR to CSR
int copy_csr(int device, int64_t n, uint64_t m, const uint64_t* off, const int64_t* adj, hipMemcpyKind kind, std::unique_ptr<bvg_text>& out) {
    std::unique_ptr<bvg_text> t = new_csr(device);
    t->nodes = n; t->arcs = m;
    if (t->d_off.alloc((size_t)n + 1) || t->adj_base.alloc((size_t)m)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base;
    HIPCHK(hipMemcpy(t->d_off.get(), off, ((size_t)n + 1) * sizeof(uint64_t), kind));
    if (m) HIPCHK(hipMemcpy(t->d_adj, adj, (size_t)m * sizeof(int64_t), kind));
    out = std::move(t);
    return 0;
}

int filter_csr(const Source& s, int kind, const int64_t* d_cls, std::unique_ptr<bvg_text>& out) {
    if (s.m > kMaxElems) return BVG_E_UNSUPPORTED;
    std::unique_ptr<bvg_text> t = new_csr(s.device);
    t->nodes = s.n;
    DevArray<int32_t> keep; DevArray<uint64_t> pos, tmp;
    const size_t mm = (size_t)(s.m ? s.m : 1);
    if (t->d_off.alloc((size_t)s.n + 1) || keep.alloc(mm) || pos.alloc(mm + 1) || tmp.alloc(scan_tmp_elems((int64_t)mm))) return BVG_E_NOMEM;
    HIPCHK(hipMemset(pos.get(), 0, (mm + 1) * sizeof(uint64_t)));
    uint64_t kept = 0;
    if (s.m) {
        hipLaunchKernelGGL(filter_keep_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.off, s.adj, s.n, s.m, kind, d_cls, keep.get());
        launch_exclusive_scan(keep.get(), pos.get(), (int64_t)s.m, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&kept, pos.get() + s.m, sizeof kept, hipMemcpyDeviceToHost));
    }
    if (t->adj_base.alloc((size_t)kept)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base; t->arcs = kept;
    if (s.m) hipLaunchKernelGGL(filter_compact_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.adj, keep.get(), pos.get(), s.m, t->d_adj);
    if (s.m) hipLaunchKernelGGL(filter_off_kernel, dim3(grid(s.n + 1, 256)), dim3(256), 0, 0, s.off, pos.get(), s.n, t->d_off.get());
    else HIPCHK(hipMemset(t->d_off.get(), 0, ((size_t)s.n + 1) * sizeof(uint64_t)));
    HIPCHK(hipDeviceSynchronize());
    out = std::move(t);
    return 0;
}

int transpose_csr(const Source& s, std::unique_ptr<bvg_text>& out) {
    if (s.m > kMaxElems) return BVG_E_UNSUPPORTED;
    std::unique_ptr<bvg_text> t = new_csr(s.device);
    t->nodes = s.n; t->arcs = s.m;
    const size_t mm = (size_t)(s.m ? s.m : 1), temp_b = transpose_temp_bytes(s.m, s.n > 0 ? s.n : 1);
    DevArray<int64_t> src; DevArray<uint64_t> keys; DevArray<uint8_t> temp; DevArray<unsigned> bad;
    if (t->d_off.alloc((size_t)s.n + 1) || t->adj_base.alloc((size_t)s.m) || src.alloc(mm) || keys.alloc(mm) || temp.alloc(temp_b ? temp_b : 16) || bad.alloc(1)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base;
    HIPCHK(hipMemset(bad.get(), 0, sizeof(unsigned)));
    if (transpose_pairs(s.off, s.n, s.m, s.adj, src.get(), keys.get(), temp.get(), temp_b, t->d_off.get(), t->d_adj, bad.get(), nullptr) != hipSuccess) {
        (void)hipGetLastError(); return BVG_E_HIP;
    }
    HIPCHK(hipDeviceSynchronize());
    out = std::move(t);
    return 0;
}

// Transform.union of two CSRs on one device; DROP_LOOPS through the filter
int union_csr(const Source& a, const Source& b, uint32_t flags, std::unique_ptr<bvg_text>& out) {
    const int64_t n = a.n > b.n ? a.n : b.n;
    std::unique_ptr<bvg_text> t = new_csr(a.device);
    t->nodes = n;
    DevArray<uint64_t> pad, tmp; DevArray<int32_t> cnt;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    if (t->d_off.alloc(nn + 1) || cnt.alloc(nn) || tmp.alloc(scan_tmp_elems((int64_t)nn))) return BVG_E_NOMEM;
    HIPCHK(hipMemset(t->d_off.get(), 0, (nn + 1) * sizeof(uint64_t)));
    const uint64_t* aoff = a.off; const uint64_t* boff = b.off;
    if (a.n != b.n) {
        const Source& shorter = a.n < b.n ? a : b;
        if (pad.alloc(nn + 1)) return BVG_E_NOMEM;
        hipLaunchKernelGGL(pad_off_kernel, dim3(grid(n + 1, 256)), dim3(256), 0, 0, shorter.off, shorter.n, n, pad.get());
        (a.n < b.n ? aoff : boff) = pad.get();
    }
    uint64_t total = 0;
    if (n > 0) {
        launch_union_count(aoff, a.adj, boff, b.adj, n, cnt.get(), nullptr);
        launch_exclusive_scan(cnt.get(), t->d_off.get(), n, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&total, t->d_off.get() + n, sizeof total, hipMemcpyDeviceToHost));
    }
    if (t->adj_base.alloc((size_t)total)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base; t->arcs = total;
    launch_union_write(aoff, a.adj, boff, b.adj, n, t->d_off.get(), t->d_adj, nullptr);
    HIPCHK(hipDeviceSynchronize());
    if (flags & BVG_TRANSFORM_DROP_LOOPS) {
        Source u; u.device = t->device; u.n = t->nodes; u.m = t->arcs; u.off = t->d_off; u.adj = t->d_adj;
        return filter_csr(u, BVG_TRANSFORM_NO_LOOPS, nullptr, out);
    }
    out = std::move(t);
    return 0;
}

int map_csr(const Source& s, const int64_t* d_map, std::unique_ptr<bvg_text>& out) {
    if (s.m > kMaxElems) return BVG_E_UNSUPPORTED;
    DevArray<unsigned long long> scal;
    if (scal.alloc(2)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(scal.get(), 0, 2 * sizeof(unsigned long long)));
    if (s.n) hipLaunchKernelGGL(map_check_kernel, dim3(grid(s.n, 256)), dim3(256), 0, 0, d_map, s.n, scal.get());
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpy(h, scal.get(), sizeof h, hipMemcpyDeviceToHost));
    if (h[1]) return BVG_E_ARG;
    if (h[0] > (unsigned long long)kMaxMapped) return BVG_E_NOMEM;
    const int64_t nodes = (int64_t)h[0];
    std::unique_ptr<bvg_text> t = new_csr(s.device);
    DevArray<uint64_t> s0, d0;
    if (s.m) {
        if (s0.alloc((size_t)s.m) || d0.alloc((size_t)s.m)) return BVG_E_NOMEM;
        hipLaunchKernelGGL(map_pairs_kernel, dim3(grid((int64_t)s.m, 256)), dim3(256), 0, 0, s.off, s.adj, s.n, s.m, d_map, (uint64_t)nodes, s0.get(), d0.get());
    }
    const int rc = pairs_to_csr(s0, d0, s.m, nodes, t.get()); if (rc) return rc;
    out = std::move(t);
    return 0;
}

int permutation_csr(const Source& s, int kind, uint64_t seed, int64_t* d_perm) {
    const int64_t n = s.n;
    if (n == 0) return 0;
    if ((uint64_t)n > kMaxElems) return BVG_E_UNSUPPORTED;
    DevArray<uint64_t> key0, key1; DevArray<uint32_t> node0, node1; DevArray<uint8_t> temp;
    if (key0.alloc((size_t)n) || key1.alloc((size_t)n) || node0.alloc((size_t)n) || node1.alloc((size_t)n)) return BVG_E_NOMEM;
    ListOrder o{s.off, s.adj, n, kind == BVG_PERM_GRAY, 0, bits_of((uint64_t)n)};
    o.k = (int)(64u / o.b);                                             // n < 2^31: at least two positions
    unsigned key_bits = 64;
    const bool dbgt = dbg_on();                                         // BVG_DEBUG: the wall clock of every stage (a synchronisation each)
    Stopwatch sw; double ms_head = 0, ms_open = 0, ms_merge = 0; uint64_t open_count = 0;
    if (kind == BVG_PERM_RANDOM) hipLaunchKernelGGL(perm_random_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, seed, n, key0.get(), node0.get());
    else { key_bits = (unsigned)o.k * o.b; hipLaunchKernelGGL(perm_heads_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, o, key0.get(), node0.get()); }
    size_t sb = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, sb, (const uint64_t*)key0.get(), key1.get(), (const uint32_t*)node0.get(), node1.get(), (size_t)n, 0u, key_bits, (hipStream_t)0));
    if (temp.alloc(sb)) return BVG_E_NOMEM;
    HIPCHK(rocprim::radix_sort_pairs(temp.get(), sb, (const uint64_t*)key0.get(), key1.get(), (const uint32_t*)node0.get(), node1.get(), (size_t)n, 0u, key_bits, (hipStream_t)0));
    // key1 / node1: the head-sorted order (RANDOM: the order)
    if (dbgt) { HIPCHK(hipDeviceSynchronize()); ms_head = sw.lap(); }
    if (kind != BVG_PERM_RANDOM) {
        DevArray<int32_t> open; DevArray<uint64_t> pos, tmp;
        if (open.alloc((size_t)n) || pos.alloc((size_t)n + 1) || tmp.alloc(scan_tmp_elems(n))) return BVG_E_NOMEM;
        hipLaunchKernelGGL(perm_open_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, o, (const uint64_t*)key1.get(), (const uint32_t*)node1.get(), open.get());
        launch_exclusive_scan(open.get(), pos.get(), n, tmp.get(), nullptr);
        uint64_t count = 0;
        HIPCHK(hipMemcpy(&count, pos.get() + n, sizeof count, hipMemcpyDeviceToHost));
        open_count = count;
        if (dbgt) ms_open = sw.lap();
        if (count) {
            DevArray<uint32_t> slot, sorted;
            if (slot.alloc((size_t)count) || sorted.alloc((size_t)count)) return BVG_E_NOMEM;
            hipLaunchKernelGGL(perm_slots_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, open.get(), pos.get(), n, slot.get());
            OpenBefore before{o, key1.get(), node1.get()};
            size_t mb = 0;
            HIPCHK(rocprim::merge_sort(nullptr, mb, (const uint32_t*)slot.get(), sorted.get(), (size_t)count, before, (hipStream_t)0));
            if (temp.alloc(mb)) return BVG_E_NOMEM;
            HIPCHK(rocprim::merge_sort(temp.get(), mb, (const uint32_t*)slot.get(), sorted.get(), (size_t)count, before, (hipStream_t)0));
            if (dbgt) { HIPCHK(hipDeviceSynchronize()); ms_merge = sw.lap(); }
            HIPCHK(hipMemcpy(node0.get(), node1.get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(perm_place_kernel, dim3(grid((int64_t)count, 256)), dim3(256), 0, 0, (const uint32_t*)sorted.get(), (const uint32_t*)slot.get(), count,
                               (const uint32_t*)node1.get(), node0.get());
            HIPCHK(hipDeviceSynchronize());
            std::swap(node0, node1);
        }
    }
    hipLaunchKernelGGL(perm_invert_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, (const uint32_t*)node1.get(), n, d_perm);
    HIPCHK(hipDeviceSynchronize());
    if (dbgt) fprintf(stderr, "[bvg] permutation kind %d: keys + radix sort %.3f ms, open runs (%llu of %lld nodes) %.3f ms, merge sort %.3f ms, place + invert %.3f ms\n", kind,
                      ms_head, (unsigned long long)open_count, (long long)n, ms_open, ms_merge, sw.lap());
    return 0;
}

// ---- entry points behind their argument checks
template <typename F> int with_source(const bvg_transform_src* src, F&& f) {
    return guarded([&]() -> int {
        Source s;
        int rc = resolve(src, s); if (rc) return rc;
        rc = f(s);
        if (hipDeviceSynchronize() != hipSuccess && !rc) { (void)hipGetLastError(); rc = BVG_E_HIP; }
        return rc;
    });
}

int from_csr_entry(int64_t nodes, const void* adj_off, const void* adj, int device, bvg_text** out, bool dev) {
    if (!out || !adj_off || nodes < 0) return BVG_E_ARG;
    return guarded([&]() -> int {
        int rc = ensure_device(device); if (rc) return rc;
        uint64_t m = 0;
        if (nodes && !dev) m = ((const uint64_t*)adj_off)[nodes];
        if (nodes && dev) HIPCHK(hipMemcpy(&m, (const uint64_t*)adj_off + nodes, sizeof m, hipMemcpyDeviceToHost));
        if (m && !adj) return BVG_E_ARG;
        if (nodes > kMaxMapped) return BVG_E_NOMEM;
        if (dev) { rc = check_csr((const uint64_t*)adj_off, (const int64_t*)adj, nodes, BVG_E_ARG); if (rc) return rc; }   // before adj_off[nodes] sizes anything
        std::unique_ptr<bvg_text> t;
        rc = copy_csr(device, nodes, m, (const uint64_t*)adj_off, (const int64_t*)adj, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, t); if (rc) return rc;
        if (!nodes) HIPCHK(hipMemset(t->d_off.get(), 0, sizeof(uint64_t)));
        if (!dev) { rc = check_csr(t->d_off, t->d_adj, nodes, BVG_E_ARG); if (rc) return rc; }
        return finish(t, out);
    });
}

int map_entry(const bvg_transform_src* src, const void* map, int64_t map_len, bvg_text** out, bool dev) {
    if (!out || !one_source(src) || map_len < 0 || (!map && map_len)) return BVG_E_ARG;
    if (map_len != source_nodes(src)) return BVG_E_ARG;
    return with_source(src, [&](const Source& s) -> int {
        DevArray<int64_t> hold; const int64_t* d_map = nullptr;
        int rc = on_device_i64(map, map_len, dev, hold, &d_map); if (rc) return rc;
        std::unique_ptr<bvg_text> t;
        rc = map_csr(s, d_map, t); if (rc) return rc;
        return finish(t, out);
    });
}

int filter_entry(const bvg_transform_src* src, int kind, const void* node_class, int64_t class_len, bvg_text** out, bool dev) {
    if (!out || !one_source(src) || class_len < 0) return BVG_E_ARG;
    if (kind != BVG_TRANSFORM_NO_LOOPS && kind != BVG_TRANSFORM_SAME_CLASS && kind != BVG_TRANSFORM_DIFFERENT_CLASS) return BVG_E_ARG;
    if (kind == BVG_TRANSFORM_NO_LOOPS ? (node_class != nullptr || class_len != 0) : (!node_class && class_len)) return BVG_E_ARG;
    if (kind != BVG_TRANSFORM_NO_LOOPS && class_len != source_nodes(src)) return BVG_E_ARG;
    return with_source(src, [&](const Source& s) -> int {
        DevArray<int64_t> hold; const int64_t* d_cls = nullptr;
        int rc = 0;
        if (kind != BVG_TRANSFORM_NO_LOOPS) { rc = on_device_i64(node_class, class_len, dev, hold, &d_cls); if (rc) return rc; }
        std::unique_ptr<bvg_text> t;
        rc = filter_csr(s, kind, d_cls, t); if (rc) return rc;
        return finish(t, out);
    });
}

int permutation_entry(const bvg_transform_src* src, int kind, uint64_t seed, void* perm, bool dev) {
    if (!one_source(src) || (kind != BVG_PERM_LEX && kind != BVG_PERM_GRAY && kind != BVG_PERM_RANDOM)) return BVG_E_ARG;
    if (!perm && source_nodes(src)) return BVG_E_ARG;
    return with_source(src, [&](const Source& s) -> int {
        DevArray<int64_t> hold; int64_t* d_perm = (int64_t*)perm;
        if (!dev) { if (hold.alloc((size_t)s.n)) return BVG_E_NOMEM; d_perm = hold.get(); }
        const int rc = permutation_csr(s, kind, seed, d_perm); if (rc) return rc;
        if (!dev && s.n) HIPCHK(hipMemcpy(perm, d_perm, (size_t)s.n * sizeof(int64_t), hipMemcpyDeviceToHost));
        return 0;
    });
}

}  // namespace
}  // namespace bvghost

extern "C" {

int bvg_transform_from_csr(int64_t nodes, const uint64_t* adj_off, const int64_t* adj, int device, bvg_text** out) { return from_csr_entry(nodes, adj_off, adj, device, out, false); }
int bvg_transform_from_csr_dev(int64_t nodes, const void* d_adj_off, const void* d_adj, int device, bvg_text** out) { return from_csr_entry(nodes, d_adj_off, d_adj, device, out, true); }

int bvg_transform_identity(const bvg_transform_src* src, bvg_text** out) {
    if (!out || !one_source(src)) return BVG_E_ARG;
    return with_source(src, [&](Source& s) -> int {
        std::unique_ptr<bvg_text> t;
        if (s.own) t = std::move(s.own);
        else { const int rc = copy_csr(s.device, s.n, s.m, s.off, s.adj, hipMemcpyDeviceToDevice, t); if (rc) return rc; }
        return finish(t, out);
    });
}

int bvg_transform_map(const bvg_transform_src* src, const int64_t* map, int64_t map_len, bvg_text** out) { return map_entry(src, map, map_len, out, false); }
int bvg_transform_map_dev(const bvg_transform_src* src, const void* d_map, int64_t map_len, bvg_text** out) { return map_entry(src, d_map, map_len, out, true); }

int bvg_transform_filter(const bvg_transform_src* src, int kind, const int64_t* node_class, int64_t class_len, bvg_text** out) { return filter_entry(src, kind, node_class, class_len, out, false); }
int bvg_transform_filter_dev(const bvg_transform_src* src, int kind, const void* d_node_class, int64_t class_len, bvg_text** out) { return filter_entry(src, kind, d_node_class, class_len, out, true); }

int bvg_transform_transpose(const bvg_transform_src* src, bvg_text** out) {
    if (!out || !one_source(src)) return BVG_E_ARG;
    return with_source(src, [&](const Source& s) -> int {
        std::unique_ptr<bvg_text> t;
        const int rc = transpose_csr(s, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_transform_symmetrize(const bvg_transform_src* src, uint32_t flags, bvg_text** out) {
    if (!out || !one_source(src) || (flags & ~(uint32_t)BVG_TRANSFORM_DROP_LOOPS)) return BVG_E_ARG;
    return with_source(src, [&](const Source& s) -> int {
        std::unique_ptr<bvg_text> tr, t;
        int rc = transpose_csr(s, tr); if (rc) return rc;
        Source b; b.device = tr->device; b.n = tr->nodes; b.m = tr->arcs; b.off = tr->d_off; b.adj = tr->d_adj;
        rc = union_csr(s, b, flags, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_transform_union(const bvg_transform_src* a, const bvg_transform_src* b, uint32_t flags, bvg_text** out) {
    if (!out || !one_source(a) || !one_source(b) || (flags & ~(uint32_t)BVG_TRANSFORM_DROP_LOOPS)) return BVG_E_ARG;
    if (source_device(a) != source_device(b)) return BVG_E_ARG;
    return with_source(a, [&](const Source& sa) -> int {
        Source sb;
        int rc = resolve(b, sb); if (rc) return rc;
        std::unique_ptr<bvg_text> t;
        rc = union_csr(sa, sb, flags, t); if (rc) return rc;
        return finish(t, out);
    });
}

int bvg_transform_permutation(const bvg_transform_src* src, int kind, uint64_t seed, int64_t* perm) { return permutation_entry(src, kind, seed, perm, false); }
int bvg_transform_permutation_dev(const bvg_transform_src* src, int kind, uint64_t seed, void* d_perm) { return permutation_entry(src, kind, seed, d_perm, true); }

}  // extern "C"
