// bvg_ef.hip — EFGraph on the device: load, outdegrees, decode, random access, scan, skipTo, store (include/bvgraph_hip.h, "EFGraph";
// reference: src/it/unimi/dsi/big/webgraph/EFGraph.java, "EF" below; the record layout is in bvg_ef.h).
//
// A quasi-succinct list has no chain of codes: element i is (select1(upper, i) - i) << l | lower[i], lower[i] sits at a computable
// address and the length of a record is a closed form of its outdegree.  So the unit of work of the decode is ONE 64-BIT WORD of an
// upper-bits region (~32 successors), not a list:
//   ef_header_kernel   one lane per node: gamma(d) at offsets[x], the geometry, the length check (offsets[x + 1] - offsets[x] must be the
//                      closed form, and the record must end inside the stream), the number of words of the upper region
//   (the shared prefix sum turns outdegrees into arc positions and word counts into flat work positions)
//   ef_packed_kernel   the words of all lists of up to kEfLongWords words laid end to end, 64 per wavefront: a lane finds the list of its
//                      word by a binary search in the prefix sums, popcounts it, a segmented prefix sum over the lanes of the same list
//                      ranks its first one, and the lane peels its ones.  A list cut by the wavefront's edge gets the ones of its words
//                      before the edge by a cooperative popcount (at most kEfLongWords - 1 words: one coalesced load)
//   ef_chunked_kernel  one wavefront per longer list, 64 words at a time, the running count carried from chunk to chunk
// Both consume on chip for bvg_ef_scan (one multiply-add per produced successor, bvg_arc_mix) or write int64 successors.
// No write leaves a list's own d slots: a lane drops every element of index >= d, and the slots of ones that a damaged region lacks are
// written as -1 by the lane that holds the region's last word.
#include "bvg_host.h"
#include "bvg_ef.h"
#include "../../include/bvgraph_hip.h"

using namespace bvgef;

namespace {

constexpr uint32_t kEfLongWords = 64;             // upper regions of more words than this take the chunked kernel (one wavefront's words)
constexpr int64_t kEfChunkNodes = 1ll << 28;      // nodes per pass: flat indices of the long-list table stay 32-bit
constexpr uint32_t kEfStripes = 1024;             // checksum accumulators of a scan, summed on the host
enum : unsigned { kEfErrEof = 1u, kEfErrUnsupported = 2u };
enum { kEfPathAuto = 0, kEfPathPacked = 1, kEfPathChunked = 2 };

struct EfView {
    const uint64_t* words; uint64_t nwords;
    const uint64_t* offsets;
    int64_t n; uint64_t U; uint32_t q;
};

struct EfShared {
    int device = 0;
    bvg_ef_params p{};
    const uint64_t* d_words = nullptr; uint64_t nwords = 0; DevArray<uint64_t> own_words;   // d_words: what the kernels read; own_words holds it unless it is the caller's
    DevArray<uint64_t> d_offsets;
    uint64_t total_bits = 0;
    std::atomic<int> refs{1};
    ~EfShared() { (void)hipSetDevice(device); }
};

}  // namespace

struct bvg_efgraph {
    EfShared* sh = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevWorkspace ws;                              // per-call arrays (below), grown on demand
    DevWorkspace out_ws;                          // successors of a host-buffer call
    ~bvg_efgraph() {
        if (sh) (void)hipSetDevice(sh->device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace {

// ---------------------------------------------------------------- kernels

// words of the upper region of a list of outdegree d > 0
__device__ __forceinline__ uint64_t ef_upper_words(const EfGeom& g) { return ((g.upper + g.upper_len - 1) >> 6) - (g.upper >> 6) + 1; }

// word j of the upper region, with the bits outside the region cleared
__device__ __forceinline__ uint64_t ef_upper_word(const EfView& v, const EfGeom& g, uint64_t j) {
    const uint64_t aw = (g.upper >> 6) + j;
    uint64_t w = ef_word(v.words, v.nwords, aw);
    const uint64_t lo = aw << 6, end = g.upper + g.upper_len;
    if (lo < g.upper) w &= ~0ull << (g.upper - lo);
    if (end < lo + 64) w &= end > lo ? ~0ull >> (lo + 64 - end) : 0ull;
    return w;
}

__global__ __launch_bounds__(256) void ef_header_kernel(EfView v, const int64_t* nodes, int64_t from, int64_t count, int32_t* deg, int32_t* pw,
                                                        uint32_t* longlist, unsigned* flags, int path) {
    BVG_FOR(i, count) {
        const int64_t x = nodes ? nodes[i] : from + i;
        const uint64_t off = v.offsets[x], nxt = v.offsets[x + 1];
        uint64_t d = 0;
        const int r = ef_read_gamma(v.words, v.nwords, off, &d);
        bool bad = r != 0;
        EfGeom g{};
        if (!bad) {
            g = ef_geom(off, d, v.U, v.q);
            bad = nxt != g.end || g.end > v.nwords * 64;          // the offsets must be the closed form; the record must lie inside the stream
            if (bad) atomicOr(&flags[0], kEfErrEof);
        } else atomicOr(&flags[0], r == 2 ? kEfErrUnsupported : kEfErrEof);
        deg[i] = bad ? 0 : (int32_t)d;
        if (!pw) continue;
        uint64_t nw = bad || d == 0 ? 0 : ef_upper_words(g);      // an empty list has nothing to produce
        const bool lng = path == kEfPathChunked || (path == kEfPathAuto && nw > kEfLongWords);
        if (nw && lng) { longlist[atomicAdd(&flags[1], 1u)] = (uint32_t)i; nw = 0; }
        pw[i] = (int32_t)nw;
    }
}

// The ones of one word: element i = rank, rank + 1, ... has high part (position in the region) - i and its lower field at lower + l i.
// MAT: out[i] = the successor; else sum += k1 * successor (the scan's one multiply-add per produced successor).
template <bool MAT>
__device__ __forceinline__ void ef_peel(const EfView& v, const EfGeom& g, uint64_t d, uint64_t w, uint64_t j, uint64_t rank, bool last,
                                        int64_t* out, uint32_t k1, uint64_t& sum, unsigned* flags) {
    const uint32_t cnt = (uint32_t)__popcll(w);
    const int64_t bit0 = (int64_t)(((g.upper >> 6) + j) << 6) - (int64_t)g.upper;   // region position of the word's bit 0
    uint64_t i = rank;
    while (w && i < d) {                                                              // the terminator and anything behind it is dropped
        const int tz = __builtin_ctzll(w);
        w &= w - 1;
        const uint64_t high = (uint64_t)(bit0 + tz) - i;
        const uint64_t y = (high << g.l) | ef_bits(v.words, v.nwords, g.lower + (uint64_t)g.l * i, g.l);
        if (MAT) out[i] = (int64_t)y; else sum += (uint64_t)k1 * y;
        i++;
    }
    if (last && rank + cnt != d + 1) {                                                // a region holds exactly d + 1 ones
        atomicOr(&flags[0], kEfErrEof);
        for (uint64_t m = rank + cnt; m < d; m++) { if (MAT) out[m] = -1; else sum += (uint64_t)k1 * ~0ull; }
    }
}

template <bool MAT>
__global__ __launch_bounds__(256) void ef_packed_kernel(EfView v, const int64_t* nodes, int64_t from, int64_t count, const int32_t* deg,
                                                        const uint64_t* wcum, const uint64_t* acum, int64_t* out, unsigned long long* acc, unsigned* flags) {
    const uint32_t lane = lane_id();
    const uint64_t W = wcum[count];
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint64_t sum = 0;
    for (uint64_t base = wave * 64; base < W; base += nwaves * 64) {                  // (wave-uniform: every lane takes part in the cross-lane steps)
        const uint64_t gi = base + lane;
        const bool active = gi < W;
        int64_t lo = 0, hi = count;                                                   // the list of this word: wcum[lo] <= gi < wcum[lo + 1]
        if (active) while (hi - lo > 1) { const int64_t mid = lo + ((hi - lo) >> 1); if (wcum[mid] <= gi) lo = mid; else hi = mid; }
        const int64_t k = lo;
        const uint64_t j = active ? gi - wcum[k] : 0;
        const int64_t x = nodes ? nodes[k] : from + k;
        const uint64_t d = (uint64_t)deg[k];
        const EfGeom g = ef_geom(v.offsets[x], d, v.U, v.q);
        const uint64_t w = active ? ef_upper_word(v, g, j) : 0;
        const uint32_t cnt = (uint32_t)__popcll(w);
        const uint32_t excl = wave_incl_scan(cnt) - cnt;
        const uint32_t first = j > lane ? 0 : lane - (uint32_t)j;                     // the lane of the list's first word in this wavefront
        uint64_t rank = excl - (uint32_t)__shfl((int)excl, (int)first, 64);
        // the list that an earlier wavefront began: the ones of its words before this one's, counted by all lanes together
        const uint64_t j0 = lane_get64(j, 0);
        if (j0) {
            const uint64_t off0 = lane_get64(v.offsets[x], 0), d0 = lane_get64(d, 0);
            const EfGeom g0 = ef_geom(off0, d0, v.U, v.q);
            uint32_t c = 0;
            for (uint64_t t = lane; t < j0; t += 64) c += (uint32_t)__popcll(ef_upper_word(v, g0, t));
            const uint64_t carry = wave_sum64(c);
            if (j > lane) rank += carry;
        }
        if (active) {
            uint32_t k0, k1; node_key((uint64_t)x, k0, k1);
            const bool last = j + 1 == ef_upper_words(g);
            ef_peel<MAT>(v, g, d, w, j, rank, last, MAT ? out + acum[k] : nullptr, k1, sum, flags);
            if (!MAT && last) sum += d * (uint64_t)k0;
        }
    }
    if (!MAT) { sum = wave_sum64(sum); if (lane == 0 && sum) atomicAdd(&acc[wave & (kEfStripes - 1)], (unsigned long long)sum); }
}

template <bool MAT>
__global__ __launch_bounds__(256) void ef_chunked_kernel(EfView v, const int64_t* nodes, int64_t from, const int32_t* deg, const uint64_t* acum,
                                                         const uint32_t* longlist, uint32_t nlong, int64_t* out, unsigned long long* acc, unsigned* flags) {
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    uint64_t sum = 0;
    for (uint32_t li = wave; li < nlong; li += nwaves) {
        const int64_t k = longlist[li];
        const int64_t x = nodes ? nodes[k] : from + k;
        const uint64_t d = (uint64_t)deg[k];
        const EfGeom g = ef_geom(v.offsets[x], d, v.U, v.q);
        const uint64_t nw = ef_upper_words(g);
        uint32_t k0, k1; node_key((uint64_t)x, k0, k1);
        uint64_t carry = 0;
        for (uint64_t c = 0; c < nw; c += 64) {
            const uint64_t j = c + lane;
            const uint64_t w = j < nw ? ef_upper_word(v, g, j) : 0;
            const uint32_t cnt = (uint32_t)__popcll(w);
            const uint32_t incl = wave_incl_scan(cnt);
            if (j < nw) ef_peel<MAT>(v, g, d, w, j, carry + incl - cnt, j + 1 == nw, MAT ? out + acum[k] : nullptr, k1, sum, flags);
            carry += lane_get(incl, 63);
        }
        if (!MAT && lane == 0) sum += d * (uint64_t)k0;
    }
    if (!MAT) { sum = wave_sum64(sum); if (lane == 0 && sum) atomicAdd(&acc[wave & (kEfStripes - 1)], (unsigned long long)sum); }
}

// skipTo(b) from a fresh iterator (EF:1098-1160), one lane per query: the smallest successor >= b among the d real ones, or -1.
// With z = b >> l zeros to pass and z > quantum, pointer (z >> q) gives the position just past the ((z >> q) << q)-th zero and the
// index of the next element; whole words are passed by their zero count, then elements are read forward.
__global__ __launch_bounds__(256) void ef_skip_kernel(EfView v, const int64_t* nodes, const int64_t* bounds, int64_t count, int64_t* out,
                                                      unsigned* flags, int use_pointers) {
    BVG_FOR(t, count) {
        const int64_t x = nodes[t];
        const uint64_t off = v.offsets[x];
        uint64_t d = 0;
        const int r = ef_read_gamma(v.words, v.nwords, off, &d);
        if (r) { atomicOr(&flags[0], r == 2 ? kEfErrUnsupported : kEfErrEof); out[t] = -1; continue; }
        const EfGeom g = ef_geom(off, d, v.U, v.q);
        if (v.offsets[x + 1] != g.end || g.end > v.nwords * 64) { atomicOr(&flags[0], kEfErrEof); out[t] = -1; continue; }
        const uint64_t b = bounds[t] < 0 ? 0 : (uint64_t)bounds[t];
        int64_t res = -1;
        if (d && b <= v.U) {
            const uint64_t z = b >> g.l;
            uint64_t pos = 0, idx = 0;                            // position in the region; index of the first element at or behind it
            if (use_pointers && g.P && z > (1ull << v.q)) {
                uint64_t block = z >> v.q; if (block > g.P) block = g.P;
                const uint64_t skip = ef_bits(v.words, v.nwords, g.ptr + (block - 1) * g.ps, g.ps), zeros = block << v.q;
                if (skip < zeros || skip > g.upper_len || skip - zeros > d + 1) { atomicOr(&flags[0], kEfErrEof); out[t] = -1; continue; }
                pos = skip; idx = skip - zeros;
            }
            bool done = false;
            while (!done && pos < g.upper_len && idx < d) {
                const uint64_t a = g.upper + pos, j = (a >> 6) - (g.upper >> 6);
                uint64_t w = ef_upper_word(v, g, j) & (~0ull << (a & 63));
                uint64_t word_end = (((a >> 6) + 1) << 6) - g.upper; if (word_end > g.upper_len) word_end = g.upper_len;
                const uint64_t ones = (uint64_t)__popcll(w), zeros_after = (word_end - idx - ones);   // zeros before word_end
                if (zeros_after < z) { pos = word_end; idx += ones; continue; }                        // every element of this word has a high part below z
                const int64_t bit0 = (int64_t)((a >> 6) << 6) - (int64_t)g.upper;
                while (w && idx < d) {
                    const uint64_t high = (uint64_t)(bit0 + __builtin_ctzll(w)) - idx;
                    w &= w - 1;
                    if (high >= z) {
                        const uint64_t y = (high << g.l) | ef_bits(v.words, v.nwords, g.lower + (uint64_t)g.l * idx, g.l);
                        if (y >= b) { res = (int64_t)y; done = true; break; }
                    }
                    idx++;
                }
                pos = word_end;
            }
            if (!done && idx < d) atomicOr(&flags[0], kEfErrEof);                                      // the region ended before its d-th one
        }
        out[t] = res;
    }
}

// ---------------------------------------------------------------- store kernels (EF:773-820 around Accumulator.add / dump, EF:501-532)

__device__ __forceinline__ void ef_put(unsigned long long* words, uint64_t pos, uint64_t value, uint32_t width) {
    if (!width || !value) return;
    const uint32_t s = (uint32_t)(pos & 63);
    atomicOr(&words[pos >> 6], (unsigned long long)(value << s));
    if (s + width > 64 && (value >> (64 - s))) atomicOr(&words[(pos >> 6) + 1], (unsigned long long)(value >> (64 - s)));
}

__global__ __launch_bounds__(256) void ef_store_check_kernel(const uint64_t* adj_off, const int64_t* adj, int64_t n, unsigned* bad) {
    BVG_FOR(x, n) {
        const uint64_t a = adj_off[x], b = adj_off[x + 1];
        for (uint64_t i = a; i < b; i++) { const int64_t y = adj[i]; if (y < 0 || y >= n || (i > a && adj[i - 1] >= y)) { atomicOr(bad, 1u); break; } }
    }
}

// One lane per ELEMENT (the successors of every list and its terminator): its lower field, its upper bit, the pointers of the quanta of
// zeros that end between the element before it and itself, and, for element 0, gamma(d).  Records share words, so every field is OR-ed
// into zeroed words.
__global__ __launch_bounds__(256) void ef_store_write_kernel(uint64_t U, uint32_t q, const uint64_t* adj_off, const int64_t* adj, int64_t n,
                                                             const uint64_t* offsets, unsigned long long* words) {
    const uint64_t total = adj_off[n] + (uint64_t)n;
    BVG_FOR(e, total) {
        int64_t lo = 0, hi = n;                                                       // adj_off[lo] + lo <= e < adj_off[lo + 1] + lo + 1
        while (hi - lo > 1) { const int64_t mid = lo + ((hi - lo) >> 1); if (adj_off[mid] + (uint64_t)mid <= (uint64_t)e) lo = mid; else hi = mid; }
        const int64_t x = lo;
        const uint64_t a = adj_off[x], d = adj_off[x + 1] - a, i = (uint64_t)e - (a + (uint64_t)x);
        const EfGeom g = ef_geom(offsets[x], d, U, q);
        if (i == 0) {
            const uint64_t val = d + 1; const int m = ef_msb(val);
            ef_put(words, offsets[x], 1ull << m, (uint32_t)m + 1);
            ef_put(words, offsets[x] + m + 1, val ^ (1ull << m), (uint32_t)m);
        }
        const uint64_t y = i < d ? (uint64_t)adj[a + i] : U;
        const uint64_t high = y >> g.l, prev_high = i ? (uint64_t)adj[a + i - 1] >> g.l : 0;
        if (g.l) ef_put(words, g.lower + (uint64_t)g.l * i, y & ((1ull << g.l) - 1), g.l);
        ef_put(words, g.upper + high + i, 1, 1);
        for (uint64_t kq = ((prev_high >> q) + 1) << q; kq <= high; kq += 1ull << q)  // pointer k = kq >> q: kq + the elements with a high part below kq (EF:511-513)
            ef_put(words, g.ptr + ((kq >> q) - 1) * g.ps, kq + i, g.ps);
    }
}

__global__ __launch_bounds__(256) void ef_bswap_kernel(unsigned long long* words, uint64_t nwords) {
    BVG_FOR(i, nwords) words[i] = __builtin_bswap64(words[i]);
}

// ---------------------------------------------------------------- host

int ef_check_params(const bvg_ef_params& p) {
    if (p.nodes < 0 || p.upper_bound < p.nodes || p.log2_quantum < 0 || p.log2_quantum > 62) return BVG_E_ARG;
    return 0;
}

// offsets[0..n] by one host walk: gamma, the closed-form length, repeat (a few operations per node)
int ef_derive_host(const bvg_ef_params& p, const uint64_t* words, uint64_t nwords, uint64_t* out) {
    uint64_t pos = 0;
    for (int64_t x = 0; x < p.nodes; x++) {
        out[x] = pos;
        uint64_t d = 0;
        const int r = ef_read_gamma(words, nwords, pos, &d);
        if (r) return r == 2 ? BVG_E_UNSUPPORTED : BVG_E_EOF;
        const EfGeom g = ef_geom(pos, d, (uint64_t)p.upper_bound, (uint32_t)p.log2_quantum);
        if (g.end > nwords * 64) return BVG_E_EOF;
        pos = g.end;
    }
    out[p.nodes] = pos;
    return 0;
}

// the stream as little-endian words (a big-endian file is swapped once, here)
void ef_host_words(const uint8_t* bytes, uint64_t nbytes, bool big_endian, std::vector<uint64_t>& out) {
    out.assign((size_t)((nbytes + 7) / 8), 0);
    if (nbytes) memcpy(out.data(), bytes, (size_t)nbytes);
    if (big_endian) for (auto& w : out) w = __builtin_bswap64(w);
}

int ef_make_handle(EfShared* sh, bvg_efgraph** out) {
    std::unique_ptr<bvg_efgraph> g(new bvg_efgraph());
    g->sh = sh;
    if (hipSetDevice(sh->device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess) { (void)hipGetLastError(); return BVG_E_HIP; }
    *out = g.release();
    return 0;
}

void ef_release(EfShared* sh) {
    if (sh->refs.fetch_sub(1) == 1) delete sh;
}

// words: host (copied) or device (adopted); offsets: host or device (copied), one of them non-null
int ef_open_common(const bvg_ef_params& p, const uint64_t* h_words, const void* d_words_in, uint64_t nwords, const uint64_t* h_offsets,
                   const void* d_offsets_in, int device, bvg_efgraph** out) {
    int r = ef_check_params(p); if (r) return r;
    r = ensure_device(device); if (r) return r;
    struct Release { void operator()(EfShared* s) const { ef_release(s); } };
    std::unique_ptr<EfShared, Release> owner(new EfShared());   // released on every return but the last
    EfShared* sh = owner.get();
    sh->device = device; sh->p = p; sh->nwords = nwords;
    const size_t n1 = (size_t)p.nodes + 1;
    if (d_words_in) sh->d_words = (const uint64_t*)d_words_in;
    else {
        if (sh->own_words.alloc((size_t)nwords)) return BVG_E_NOMEM;
        sh->d_words = sh->own_words;
        if (nwords && hipMemcpy(sh->own_words, h_words, (size_t)nwords * 8, hipMemcpyHostToDevice) != hipSuccess) return BVG_E_HIP;
    }
    if (sh->d_offsets.alloc(n1)) return BVG_E_NOMEM;
    if (hipMemcpy(sh->d_offsets, h_offsets ? (const void*)h_offsets : d_offsets_in, n1 * 8, h_offsets ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice) != hipSuccess) return BVG_E_HIP;
    if (hipMemcpy(&sh->total_bits, sh->d_offsets + p.nodes, 8, hipMemcpyDeviceToHost) != hipSuccess) return BVG_E_HIP;
    r = ef_make_handle(sh, out); if (r) return r;
    (void)owner.release();
    return 0;
}

int ef_path() { const char* k = knob("BVG_EF_PATH"); const int v = k ? atoi(k) : 0; return v == kEfPathPacked || v == kEfPathChunked ? v : kEfPathAuto; }
bool ef_no_pointers() { const char* k = knob("BVG_EF_NOPTR"); return k && atoi(k) != 0; }

// the per-call arrays of `count` nodes, in the handle's workspace
struct EfBufs {
    int32_t* deg; int32_t* pw; uint64_t* acum; uint64_t* wcum; uint64_t* tmp; uint32_t* longlist; unsigned* flags; unsigned long long* acc; int64_t* nodes;
};
size_t ef_align(size_t b) { return (b + 255) & ~(size_t)255; }
int ef_bufs(bvg_efgraph* g, int64_t count, bool with_nodes, EfBufs& b) {
    const size_t c = (size_t)count;
    const size_t s_deg = ef_align((c + 1) * 4), s_cum = ef_align((c + 1) * 8), s_tmp = ef_align(scan_tmp_elems(count) * 8 + 8), s_long = ef_align(c * 4 + 4),
                 s_flags = 256, s_acc = ef_align(kEfStripes * 8), s_nodes = with_nodes ? ef_align(c * 8 + 8) : 0;
    const size_t total = 2 * s_deg + 2 * s_cum + s_tmp + s_long + s_flags + s_acc + s_nodes;
    const int r = g->ws.reserve(total); if (r) return r;
    char* p = g->ws.at(0);
    b.deg = (int32_t*)p; p += s_deg; b.pw = (int32_t*)p; p += s_deg; b.acum = (uint64_t*)p; p += s_cum; b.wcum = (uint64_t*)p; p += s_cum;
    b.tmp = (uint64_t*)p; p += s_tmp; b.longlist = (uint32_t*)p; p += s_long; b.flags = (unsigned*)p; p += s_flags; b.acc = (unsigned long long*)p; p += s_acc;
    b.nodes = with_nodes ? (int64_t*)p : nullptr;
    return 0;
}

EfView ef_view(const EfShared* sh) { return EfView{sh->d_words, sh->nwords, sh->d_offsets, sh->p.nodes, (uint64_t)sh->p.upper_bound, (uint32_t)sh->p.log2_quantum}; }

int ef_status(unsigned flags) { return flags & kEfErrUnsupported ? BVG_E_UNSUPPORTED : flags & kEfErrEof ? BVG_E_EOF : 0; }

// header pass over nodes [from, from + count) (or d_nodes[0..count)): outdegrees, the length check, and with `work` the prefix sums
// the decode kernels need.  Synchronises; *arcs / *nwork / *nlong are what the host needs to size and launch the rest.
int ef_header(bvg_efgraph* g, const EfBufs& b, const int64_t* d_nodes, int64_t from, int64_t count, bool work, uint64_t* arcs, uint64_t* nwork, uint32_t* nlong) {
    hipStream_t s = g->stream;
    HIPCHK(hipMemsetAsync(b.flags, 0, 256, s));
    hipLaunchKernelGGL(ef_header_kernel, dim3(grid(count, 256)), dim3(256), 0, s, ef_view(g->sh), d_nodes, from, count, b.deg, work ? b.pw : nullptr, b.longlist, b.flags, ef_path());
    launch_exclusive_scan(b.deg, b.acum, count, b.tmp, s);
    if (work) launch_exclusive_scan(b.pw, b.wcum, count, b.tmp, s);
    unsigned hf[2] = {0, 0}; uint64_t ha = 0, hw = 0;
    HIPCHK(hipMemcpyAsync(hf, b.flags, sizeof hf, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&ha, b.acum + count, 8, hipMemcpyDeviceToHost, s));
    if (work) HIPCHK(hipMemcpyAsync(&hw, b.wcum + count, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (arcs) *arcs = ha;
    if (nwork) *nwork = hw;
    if (nlong) *nlong = hf[1];
    return ef_status(hf[0]);
}

// the decode kernels over a header pass's arrays: successors to d_out (int64, acum-indexed) or, d_out == nullptr, the checksum into b.acc
void ef_emit(bvg_efgraph* g, const EfBufs& b, const int64_t* d_nodes, int64_t from, int64_t count, uint64_t nwork, uint32_t nlong, int64_t* d_out) {
    hipStream_t s = g->stream;
    const EfView v = ef_view(g->sh);
    if (nwork) {
        const unsigned blocks = grid((int64_t)((nwork + 63) / 64), 4) > 8192u ? 8192u : grid((int64_t)((nwork + 63) / 64), 4);
        if (d_out) hipLaunchKernelGGL(ef_packed_kernel<true>, dim3(blocks), dim3(256), 0, s, v, d_nodes, from, count, b.deg, b.wcum, b.acum, d_out, b.acc, b.flags);
        else hipLaunchKernelGGL(ef_packed_kernel<false>, dim3(blocks), dim3(256), 0, s, v, d_nodes, from, count, b.deg, b.wcum, b.acum, d_out, b.acc, b.flags);
    }
    if (nlong) {
        const unsigned blocks = grid((int64_t)nlong, 4) > 8192u ? 8192u : grid((int64_t)nlong, 4);
        if (d_out) hipLaunchKernelGGL(ef_chunked_kernel<true>, dim3(blocks), dim3(256), 0, s, v, d_nodes, from, b.deg, b.acum, b.longlist, nlong, d_out, b.acc, b.flags);
        else hipLaunchKernelGGL(ef_chunked_kernel<false>, dim3(blocks), dim3(256), 0, s, v, d_nodes, from, b.deg, b.acum, b.longlist, nlong, d_out, b.acc, b.flags);
    }
}

int ef_flags_after(bvg_efgraph* g, const EfBufs& b) {
    unsigned hf = 0;
    HIPCHK(hipMemcpyAsync(&hf, b.flags, sizeof hf, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipGetLastError());
    return ef_status(hf);
}

// bvg_ef_decode_range / _dev and, with h_nodes, bvg_ef_successors_batch.  Nothing is written unless every record of the call passes the
// header's checks and the buffer is large enough; a region that then lacks ones is BVG_E_EOF with its missing slots written as -1.
int ef_decode_impl(bvg_efgraph* g, const int64_t* h_nodes, int64_t from, int64_t count, int32_t* outdeg, int64_t* succ, uint64_t cap, uint64_t* n_succ, bool dev) {
    EfShared* sh = g->sh;
    HIPCHK(hipSetDevice(sh->device));
    if (count == 0) { *n_succ = 0; return 0; }
    hipStream_t s = g->stream;
    const int64_t chunk = h_nodes ? count : kEfChunkNodes;
    const int64_t nchunks = (count + chunk - 1) / chunk;
    EfBufs b;
    int r = ef_bufs(g, std::min(count, chunk), h_nodes != nullptr, b); if (r) return r;
    if (h_nodes) HIPCHK(hipMemcpyAsync(b.nodes, h_nodes, (size_t)count * 8, hipMemcpyHostToDevice, s));
    uint64_t total = 0, arcs = 0, nwork = 0; uint32_t nlong = 0;
    for (int64_t c = 0; c < nchunks; c++) {                      // every record is checked, and the size known, before anything is written
        const int64_t lo = c * chunk, cnt = std::min(chunk, count - lo);
        r = ef_header(g, b, b.nodes, from + lo, cnt, true, &arcs, &nwork, &nlong); if (r) return r;
        total += arcs;
    }
    *n_succ = total;
    if (total > cap || (!succ && total)) return BVG_E_CAPACITY;
    int64_t* d_out = succ;
    if (!dev) { r = g->out_ws.reserve((size_t)(total ? total : 1) * 8); if (r) return r; d_out = (int64_t*)g->out_ws.get(); }
    int status = 0; uint64_t at = 0;
    for (int64_t c = 0; c < nchunks; c++) {
        const int64_t lo = c * chunk, cnt = std::min(chunk, count - lo);
        if (nchunks > 1) { r = ef_header(g, b, b.nodes, from + lo, cnt, true, &arcs, &nwork, &nlong); if (r) return r; }
        ef_emit(g, b, b.nodes, from + lo, cnt, nwork, nlong, d_out + at);
        if (outdeg) HIPCHK(hipMemcpyAsync(outdeg + lo, b.deg, (size_t)cnt * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        r = ef_flags_after(g, b); if (r) status = r;
        at += arcs;
    }
    if (!dev && total) HIPCHK(hipMemcpy(succ, d_out, (size_t)total * 8, hipMemcpyDeviceToHost));
    return status;
}

int ef_scan_impl(bvg_efgraph* g, int64_t from, int64_t to, bvg_scan_result* out) {
    EfShared* sh = g->sh;
    memset(out, 0, sizeof *out);
    if (from == to) return 0;
    HIPCHK(hipSetDevice(sh->device));
    hipStream_t s = g->stream;
    const int64_t count = to - from, nchunks = (count + kEfChunkNodes - 1) / kEfChunkNodes;
    EfBufs b;
    int r = ef_bufs(g, std::min(count, kEfChunkNodes), false, b); if (r) return r;
    int status = 0; double ms = 0;
    for (int64_t c = 0; c < nchunks; c++) {
        const int64_t lo = from + c * kEfChunkNodes, cnt = std::min(kEfChunkNodes, to - lo);
        uint64_t arcs = 0, nwork = 0; uint32_t nlong = 0;
        HIPCHK(hipEventRecord(g->ev0, s));
        r = ef_header(g, b, nullptr, lo, cnt, true, &arcs, &nwork, &nlong); if (r) return r;
        HIPCHK(hipMemsetAsync(b.acc, 0, kEfStripes * 8, s));
        ef_emit(g, b, nullptr, lo, cnt, nwork, nlong, nullptr);
        HIPCHK(hipEventRecord(g->ev1, s));
        unsigned long long acc[kEfStripes];
        HIPCHK(hipMemcpyAsync(acc, b.acc, sizeof acc, hipMemcpyDeviceToHost, s));
        r = ef_flags_after(g, b); if (r) status = r;
        float t = 0; HIPCHK(hipEventElapsedTime(&t, g->ev0, g->ev1)); ms += t;
        for (uint32_t i = 0; i < kEfStripes; i++) out->chk += acc[i];
        out->arcs += arcs; out->launches += 3 + (nwork ? 1 : 0) + (nlong ? 1 : 0);
    }
    uint64_t o[2];
    HIPCHK(hipMemcpy(&o[0], sh->d_offsets + from, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&o[1], sh->d_offsets + to, 8, hipMemcpyDeviceToHost));
    out->nodes = (uint64_t)count;
    out->graph_bytes = o[1] > o[0] ? (((o[1] - 1) >> 6) - (o[0] >> 6) + 1) * 8 : 0;
    out->index_bytes = ((uint64_t)count + 1) * 8;
    out->kernel_ms = ms;
    return status;
}

}  // namespace

extern "C" {

int bvg_ef_parse_properties(const char* text, size_t len, bvg_ef_params* out) {
    if (!text || !out) return BVG_E_ARG;
    return guarded([&]() -> int {
        bvg_ef_params p{}; p.arcs = -1; p.upper_bound = -1;
        bool have_nodes = false, have_class = false, have_version = false, have_quantum = false, have_order = false; long version = 0; long long quantum = 0;
        std::string t(text, len);
        auto trim = [](std::string s) {
            size_t a = 0, b = s.size();
            while (a < b && isspace((unsigned char)s[a])) a++;
            while (b > a && isspace((unsigned char)s[b - 1])) b--;
            return s.substr(a, b - a);
        };
        size_t i = 0;
        while (i < t.size()) {
            size_t e = t.find_first_of("\r\n", i); if (e == std::string::npos) e = t.size();
            std::string line = trim(t.substr(i, e - i));
            i = e + 1;
            if (line.empty() || line[0] == '#' || line[0] == '!') continue;
            const size_t sep = line.find_first_of("=:");
            const std::string key = trim(sep == std::string::npos ? line : line.substr(0, sep));
            std::string val = sep == std::string::npos ? "" : trim(line.substr(sep + 1));
            if (key == "nodes") { p.nodes = strtoll(val.c_str(), nullptr, 10); have_nodes = true; }
            else if (key == "arcs") p.arcs = strtoll(val.c_str(), nullptr, 10);
            else if (key == "upperbound") p.upper_bound = strtoll(val.c_str(), nullptr, 10);
            else if (key == "quantum") { quantum = strtoll(val.c_str(), nullptr, 10); have_quantum = true; }
            else if (key == "version") { version = strtol(val.c_str(), nullptr, 10); have_version = true; }
            else if (key == "byteorder") {
                if (val == "BIG_ENDIAN") p.big_endian = 1; else if (val == "LITTLE_ENDIAN") p.big_endian = 0; else return BVG_E_ARG;   // EF:696-698
                have_order = true;
            } else if (key == "graphclass") {
                if (val.rfind("class ", 0) == 0) val = val.substr(6);
                if (val != "it.unimi.dsi.big.webgraph.EFGraph" && val != "it.unimi.dsi.webgraph.EFGraph") return BVG_E_IO;            // EF:683-684
                have_class = true;
            }
        }
        if (!have_class || !have_version || version > 0 || !have_nodes || !have_quantum || !have_order) return BVG_E_IO;              // EF:686-691
        if (quantum <= 0 || (quantum & (quantum - 1))) return BVG_E_ARG;                                                              // EF:693
        p.log2_quantum = ef_msb((uint64_t)quantum);
        if (p.upper_bound < 0) p.upper_bound = p.nodes;                                                                               // EF:690
        const int r = ef_check_params(p); if (r) return r;
        *out = p;
        return 0;
    });
}

// (host only) the offsets of a bare stream: what a load without basename.offsets derives
int bvg_ef_derive_offsets(const bvg_ef_params* p, const uint8_t* bytes, uint64_t nbytes, uint64_t* out) {
    if (!p || !out || (!bytes && nbytes)) return BVG_E_ARG;
    return guarded([&]() -> int {
        int r = ef_check_params(*p); if (r) return r;
        std::vector<uint64_t> words; ef_host_words(bytes, nbytes, p->big_endian != 0, words);
        return ef_derive_host(*p, words.data(), words.size(), out);
    });
}

int bvg_ef_open_mem(const bvg_ef_params* p, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, int device, bvg_efgraph** out) {
    if (!p || !out || (!bytes && nbytes)) return BVG_E_ARG;
    return guarded([&]() -> int {
        int r = ef_check_params(*p); if (r) return r;
        if ((uint64_t)p->nodes > nbytes * 8) return BVG_E_EOF;                       // every record takes at least two bits
        std::vector<uint64_t> words; ef_host_words(bytes, nbytes, p->big_endian != 0, words);
        std::vector<uint64_t> derived;
        if (!offsets) {
            derived.resize((size_t)p->nodes + 1);
            r = ef_derive_host(*p, words.data(), words.size(), derived.data()); if (r) return r;
            offsets = derived.data();
        }
        return ef_open_common(*p, words.data(), nullptr, words.size(), offsets, nullptr, device, out);
    });
}

int bvg_ef_open(const char* basename, int load_mode, int device, bvg_efgraph** out) {
    if (!basename || !out) return BVG_E_ARG;
    if (load_mode < BVG_LOAD_OFFLINE || load_mode > BVG_LOAD_MAPPED) return BVG_E_ARG;
    return guarded([&]() -> int {
        const std::string base(basename);
        std::vector<uint8_t> props, graph, offs;
        int r = read_file(base + ".properties", props); if (r) return r;
        bvg_ef_params p;
        r = bvg_ef_parse_properties((const char*)props.data(), props.size(), &p); if (r) return r;
        r = read_file(base + ".graph", graph); if (r) return r;
        if (load_mode < BVG_LOAD_STANDARD) return bvg_ef_open_mem(&p, graph.data(), graph.size(), nullptr, device, out);
        r = read_file(base + ".offsets", offs); if (r) return r;
        if ((uint64_t)p.nodes > (uint64_t)offs.size() * 8) return BVG_E_EOF;         // every gap takes at least one bit
        std::vector<uint64_t> offsets((size_t)p.nodes + 1);
        r = bvg_decode_offsets(offs.data(), offs.size(), p.nodes, BVG_DELTA, offsets.data()); if (r) return r;   // EF:738-740, EF:785, EF:812
        return bvg_ef_open_mem(&p, graph.data(), graph.size(), offsets.data(), device, out);
    });
}

int bvg_ef_open_dev(const bvg_ef_params* p, const void* d_words, uint64_t nbytes, const void* d_offsets, int device, bvg_efgraph** out) {
    if (!p || !out || !d_words || !d_offsets || p->big_endian || (nbytes & 7)) return BVG_E_ARG;
    return guarded([&]() -> int { return ef_open_common(*p, nullptr, d_words, nbytes / 8, nullptr, d_offsets, device, out); });
}

int bvg_ef_copy(const bvg_efgraph* g, bvg_efgraph** out) {
    if (!g || !out) return BVG_E_ARG;
    g->sh->refs.fetch_add(1);
    const int r = ef_make_handle(g->sh, out);
    if (r) ef_release(g->sh);
    return r;
}

void bvg_ef_close(bvg_efgraph* g) {
    if (!g) return;
    EfShared* const sh = g->sh;
    delete g;
    ef_release(sh);
}

int bvg_ef_info(const bvg_efgraph* g, bvg_ef_params* out) { if (!g || !out) return BVG_E_ARG; *out = g->sh->p; return 0; }

int bvg_ef_get_offsets(bvg_efgraph* g, uint64_t* out) {
    if (!g || !out) return BVG_E_ARG;
    HIPCHK(hipSetDevice(g->sh->device));
    HIPCHK(hipMemcpy(out, g->sh->d_offsets, ((size_t)g->sh->p.nodes + 1) * 8, hipMemcpyDeviceToHost));
    return 0;
}

int bvg_ef_outdegrees(bvg_efgraph* g, int64_t from, int64_t to, int32_t* out) {
    if (!g || from < 0 || to > g->sh->p.nodes || from > to || (!out && to > from)) return BVG_E_ARG;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(g->sh->device));
        for (int64_t lo = from; lo < to; lo += kEfChunkNodes) {
            const int64_t cnt = std::min(kEfChunkNodes, to - lo);
            EfBufs b;
            int r = ef_bufs(g, cnt, false, b); if (r) return r;
            r = ef_header(g, b, nullptr, lo, cnt, false, nullptr, nullptr, nullptr); if (r) return r;
            HIPCHK(hipMemcpy(out + (lo - from), b.deg, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        }
        return 0;
    });
}

int bvg_ef_decode_range(bvg_efgraph* g, int64_t from, int64_t to, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ) {
    if (!g || !n_succ || from < 0 || to > g->sh->p.nodes || from > to) return BVG_E_ARG;
    return guarded([&] { return ef_decode_impl(g, nullptr, from, to - from, outdeg, succ, succ_cap, n_succ, false); });
}

int bvg_ef_decode_range_dev(bvg_efgraph* g, int64_t from, int64_t to, void* d_outdeg, void* d_succ, uint64_t succ_cap, uint64_t* n_succ) {
    if (!g || !n_succ || from < 0 || to > g->sh->p.nodes || from > to) return BVG_E_ARG;
    return guarded([&] { return ef_decode_impl(g, nullptr, from, to - from, (int32_t*)d_outdeg, (int64_t*)d_succ, succ_cap, n_succ, true); });
}

int bvg_ef_successors_batch(bvg_efgraph* g, const int64_t* nodes, int64_t count, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ) {
    if (!g || !n_succ || count < 0 || count > kMaxBatchRequests || (!nodes && count)) return BVG_E_ARG;
    for (int64_t i = 0; i < count; i++) if (nodes[i] < 0 || nodes[i] >= g->sh->p.nodes) return BVG_E_ARG;
    return guarded([&] { return ef_decode_impl(g, nodes, 0, count, outdeg, succ, succ_cap, n_succ, false); });
}

int bvg_ef_scan(bvg_efgraph* g, int64_t from, int64_t to, bvg_scan_result* out) {
    if (!g || !out || from < 0 || to > g->sh->p.nodes || from > to) return BVG_E_ARG;
    return guarded([&] { return ef_scan_impl(g, from, to, out); });
}

int bvg_ef_skip_to_batch(bvg_efgraph* g, const int64_t* nodes, const int64_t* bounds, int64_t count, int64_t* out) {
    if (!g || count < 0 || count > kMaxBatchRequests || (count && (!nodes || !bounds || !out))) return BVG_E_ARG;
    for (int64_t i = 0; i < count; i++) if (nodes[i] < 0 || nodes[i] >= g->sh->p.nodes) return BVG_E_ARG;
    if (count == 0) return 0;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(g->sh->device));
        hipStream_t s = g->stream;
        const size_t c8 = ef_align((size_t)count * 8);
        int r = g->out_ws.reserve(3 * c8 + 256); if (r) return r;
        int64_t* dn = (int64_t*)g->out_ws.at(0); int64_t* db = (int64_t*)g->out_ws.at(c8); int64_t* dout = (int64_t*)g->out_ws.at(2 * c8);
        unsigned* flags = (unsigned*)g->out_ws.at(3 * c8);
        HIPCHK(hipMemsetAsync(flags, 0, 256, s));
        HIPCHK(hipMemcpyAsync(dn, nodes, (size_t)count * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(db, bounds, (size_t)count * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(g->ev0, s));
        hipLaunchKernelGGL(ef_skip_kernel, dim3(grid(count, 256)), dim3(256), 0, s, ef_view(g->sh), dn, db, count, dout, flags, ef_no_pointers() ? 0 : 1);
        HIPCHK(hipEventRecord(g->ev1, s));
        unsigned hf = 0;
        HIPCHK(hipMemcpyAsync(&hf, flags, sizeof hf, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        r = ef_status(hf); if (r) return r;
        HIPCHK(hipMemcpy(out, dout, (size_t)count * 8, hipMemcpyDeviceToHost));
        return 0;
    });
}

// hipEvent time of the kernels of the last bvg_ef_skip_to_batch on this handle (measurements)
int bvg_ef_last_kernel_ms(bvg_efgraph* g, double* ms) {
    if (!g || !ms) return BVG_E_ARG;
    float t = 0;
    if (hipEventElapsedTime(&t, g->ev0, g->ev1) != hipSuccess) { (void)hipGetLastError(); return BVG_E_STATE; }
    *ms = t;
    return 0;
}

// EFGraph.store (EF:773-820) on the device: host CSR in, malloc'ed host buffers out (bvg_free)
int bvg_ef_store(int64_t nodes, int64_t upper_bound, int log2_quantum, int big_endian, const uint64_t* adj_off, const int64_t* adj, int device,
                 uint8_t** graph, uint64_t* graph_bytes, uint64_t** offsets) {
    if (!adj_off || !graph || !graph_bytes || !offsets || nodes < 0 || upper_bound < nodes || log2_quantum < 0 || log2_quantum > 62) return BVG_E_ARG;
    return guarded([&]() -> int {
        // the offsets of adj must describe adj[0 .. adj_off[nodes]): start at 0, never decrease, at most 2^31 - 1 successors per list
        if (adj_off[0] != 0) return BVG_E_ARG;
        for (int64_t x = 0; x < nodes; x++) if (adj_off[x + 1] < adj_off[x] || adj_off[x + 1] - adj_off[x] > 0x7FFFFFFFull) return BVG_E_ARG;
        const uint64_t m = adj_off[nodes];
        if (m && !adj) return BVG_E_ARG;
        int r = ensure_device(device); if (r) return r;
        // sizes from outdegrees -> prefix sum: record lengths exceed 32 bits long before outdegrees do, and the CSR offsets are host memory
        // already, so this serial sum (a few operations per node, as the derivation at load) runs on the host
        HostArray<uint64_t> ho((uint64_t*)malloc(((size_t)nodes + 1) * 8));
        if (!ho) return BVG_E_NOMEM;
        ho[0] = 0;
        for (int64_t x = 0; x < nodes; x++) ho[x + 1] = ef_geom(ho[x], adj_off[x + 1] - adj_off[x], (uint64_t)upper_bound, (uint32_t)log2_quantum).end;
        const uint64_t nwords = ho[nodes] / 64 + 1;                                   // close() always writes the current word (EF:408-413)
        DevArray<uint64_t> d_off, d_offsets; DevArray<int64_t> d_adj; DevArray<unsigned long long> d_words; DevArray<unsigned> d_bad;
        if (d_off.alloc((size_t)nodes + 1) || d_adj.alloc((size_t)m) || d_offsets.alloc((size_t)nodes + 1) || d_words.alloc((size_t)nwords) || d_bad.alloc(1)) return BVG_E_NOMEM;
        if (hipMemcpy(d_off, adj_off, ((size_t)nodes + 1) * 8, hipMemcpyHostToDevice) != hipSuccess || (m && hipMemcpy(d_adj, adj, (size_t)m * 8, hipMemcpyHostToDevice) != hipSuccess) ||
            hipMemcpy(d_offsets, ho.get(), ((size_t)nodes + 1) * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_bad, 0, 4) != hipSuccess || hipMemset(d_words, 0, (size_t)nwords * 8) != hipSuccess) return BVG_E_HIP;
        const uint64_t* p_off = d_off; const int64_t* p_adj = d_adj; const uint64_t* p_offsets = d_offsets;
        unsigned long long* p_words = d_words; unsigned* p_bad = d_bad;
        const uint64_t ub = (uint64_t)upper_bound; const uint32_t q = (uint32_t)log2_quantum;
        unsigned hb = 0;
        if (nodes) hipLaunchKernelGGL(ef_store_check_kernel, dim3(grid(nodes, 256)), dim3(256), 0, 0, p_off, p_adj, nodes, p_bad);
        if (hipMemcpy(&hb, p_bad, 4, hipMemcpyDeviceToHost) != hipSuccess) return BVG_E_HIP;
        if (hb) return BVG_E_ARG;
        if (nodes) hipLaunchKernelGGL(ef_store_write_kernel, dim3(grid((int64_t)(m + (uint64_t)nodes), 256)), dim3(256), 0, 0, ub, q, p_off, p_adj, nodes, p_offsets, p_words);
        if (big_endian) hipLaunchKernelGGL(ef_bswap_kernel, dim3(grid((int64_t)nwords, 256)), dim3(256), 0, 0, p_words, nwords);
        HostArray<uint8_t> hg((uint8_t*)malloc((size_t)nwords * 8));
        if (!hg) return BVG_E_NOMEM;
        if (hipMemcpy(hg.get(), p_words, (size_t)nwords * 8, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return BVG_E_HIP;
        *graph = hg.release(); *graph_bytes = nwords * 8; *offsets = ho.release();
        return 0;
    });
}

}  // extern "C"
