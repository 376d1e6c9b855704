// bvg_hyperball.hip — HyperBall on the device (algo/HyperBall.java: non-systolic, in-memory iterations).
//
// One HyperLogLog counter of m = 2^log2m registers per node; iteration k makes counter x the register-wise maximum of itself and of the
// counters of its successors, so after it counter x estimates the nodes within distance k + 1 of x.  The sum of the estimates is a term of the
// neighbourhood function; the increments of a node's estimate, weighted by the distance, are its sum of distances and its harmonic centrality.
// The graph stays compressed: an iteration decodes it in arc-bounded node ranges (SweepPlan, bvg_plan.hip) and consumes each batch at once.
//
// Hash (ours: the reference's comes from a library that is not part of it; include/bvgraph_hip.h has the definition):
//   x = mix64(v + (seed + 1) * 0x9E3779B97F4A7C15), j = x & (m - 1), r = ctz((x >> log2m) | 1 << (64 - log2m)) + 1, reg[j] = max(reg[j], r).
// r <= 65 - log2m <= 61: a register is a byte with its top bit clear, a counter is m bytes, aligned to m, register j at byte j.
//
//   hb_init_kernel      every 16-byte piece of the current buffer: zeroes, and the one register of its node where it falls into the piece
//   hb_iterate_kernel   one wavefront per 64 consecutive lists of a batch (four per workgroup, no workgroup barrier).  A counter lies on
//                       G = clamp(m / 16, 1, 64) lanes of K = m / (16 G) pieces each, so a gather is whole 64- or 128-byte lines and the 64 / G
//                       groups of a wavefront walk 64 / G lists at a time, the accumulator in registers.  Per arc: bounds check (outside
//                       [0, n): flagged, never an index), s == x skipped, the modified bit of s (a bitmap of n / 8 bytes), and only then the
//                       gather.  Lists of kLong arcs and more (all lists when a counter takes the whole wavefront) are walked by the whole
//                       wavefront: 64 arcs are tested at once, the ones that pass are compacted (LDS) and dealt to the groups, and the
//                       groups' partial maxima are combined with cross-lane moves and the same bytewise maximum.  The count of the new
//                       value, the centrality increments, the modified bit and the neighbourhood-function partial are done in the same
//                       kernel: the counter is in registers there, a second kernel would read n m bytes again.
//   hb_reduce_kernel    the per-wavefront partial sums of a batch added, in a fixed order, to the iteration's term (one workgroup)
//
// Bytewise maximum: gfx950 has no packed 8-bit maximum; with the top bits clear, (a | 0x80808080) - b leaves bit 7 of every byte set exactly where
// a >= b with no borrow between bytes, and the select is one three-input bit operation: seven VALU operations per 32-bit word (v_or, v_sub,
// v_and, v_lshrrev, v_sub, v_or, v_bitop3 in the ISA hipcc emits for gfx950), against an extract / v_max / pack sequence of about three per
// BYTE for the plain loop over unsigned chars.  The count's tally is the larger part of the kernel's registers (about 150 VGPRs, no scratch).
//
// Count.  sum 2^-reg is taken exactly: registers <= 30 add 2^(30 - reg) to one 64-bit integer, the others 2^(61 - reg) to a second; both stay
// below 2^53, so the sum is (double)hi 2^-30 + (double)lo 2^-61 with ONE rounding whatever the order of lanes: the value of the histogram sum
// taken from the largest register value down, less its intermediate roundings.
//
// Memory model.  An iteration reads cur[] and the current modified bitmap, which no kernel of the iteration writes, and writes next[] (each
// counter by the one group that owns its list) and the next bitmap (atomic OR: two wavefronts may share a word): no atomics on counters, no
// read of a value written in the same iteration.  A node that is unmodified now and was unmodified by the previous iteration is not rewritten
// (the reference's `unwritten`): at the start of every iteration next[x] == cur[x] for every x whose bit is clear -- all bits are set after
// init, and an unmodified x leaves cur[x] (its value) in what becomes next[] and the same value, written or already there, in the new cur[].
//
// Determinism.  Registers are exact (a maximum has no order).  A wavefront adds the estimates of its 64 lists in a fixed order, the partials of
// a batch are added by one workgroup in a fixed tree, batches in order: no floating-point atomics, and the same batch plan gives the same bits.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

enum : int { kCtlBad = 0, kCtlModified = 1, kCtlPassed = 2, kCtlWords = 4 };   // control words (unsigned long long) the host reads back
constexpr uint64_t kLong = 256;                    // lists of this many arcs and more are walked by the whole wavefront

__host__ __device__ inline uint64_t hb_mix64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b) {              // bytes below 128
    const uint32_t ge = ((a | 0x80808080u) - b) & 0x80808080u;                       // bit 7 of a byte: a >= b there
    const uint32_t mask = ge | (ge - (ge >> 7));
    return (a & mask) | (b & ~mask);
}
__device__ __forceinline__ uint4 max_u8x16(uint4 a, uint4 b) { return make_uint4(max_u8x4(a.x, b.x), max_u8x4(a.y, b.y), max_u8x4(a.z, b.z), max_u8x4(a.w, b.w)); }

template <int K> struct Regs { uint4 v[K]; };

// sum 2^-reg of 4 registers into the two integers described above; the registers that are 0
__device__ __forceinline__ void tally4(uint32_t w, uint64_t& hi, uint64_t& lo, uint32_t& zeros) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t r = (w >> (8 * i)) & 0xFFu;
        const bool big = r <= 30;
        const uint64_t one = 1ull << ((big ? 30u : 61u) - (r > 61 ? 61u : r));
        hi += big ? one : 0; lo += big ? 0 : one; zeros += r == 0;
    }
}

__device__ __forceinline__ double hb_estimate(uint64_t hi, uint64_t lo, uint32_t zeros, double m, double alpha_mm) {
    const double s = (double)hi * 0x1p-30 + (double)lo * 0x1p-61;                    // (both products exact)
    double e = alpha_mm / s;
    if (zeros != 0 && e < 2.5 * m) e = m * log(m / (double)zeros);
    return e;
}

template <int LOG2M> struct Shape {
    static constexpr int M = 1 << LOG2M;
    static constexpr int G = M / 16 < 1 ? 1 : (M / 16 > 64 ? 64 : M / 16);          // lanes of a counter
    static constexpr int K = M / (16 * G);                                           // 16-byte pieces per lane
    static constexpr int P = 64 / G;                                                 // counters a wavefront holds
};

template <int LOG2M> __device__ __forceinline__ Regs<Shape<LOG2M>::K> load_counter(const uint8_t* buf, int64_t x, unsigned q) {
    using S = Shape<LOG2M>;
    Regs<S::K> r;
    const uint4* p = (const uint4*)(buf + ((uint64_t)x << LOG2M)) + q;
#pragma unroll
    for (int k = 0; k < S::K; k++) r.v[k] = p[k * S::G];
    return r;
}

// the estimate of a counter held by a group of G lanes (every lane of the group gets it); all 64 lanes call
template <int LOG2M> __device__ __forceinline__ double count_regs(const Regs<Shape<LOG2M>::K>& t, double alpha_mm) {
    using S = Shape<LOG2M>;
    uint64_t hi = 0, lo = 0; uint32_t zeros = 0;
#pragma unroll
    for (int k = 0; k < S::K; k++) { tally4(t.v[k].x, hi, lo, zeros); tally4(t.v[k].y, hi, lo, zeros); tally4(t.v[k].z, hi, lo, zeros); tally4(t.v[k].w, hi, lo, zeros); }
#pragma unroll
    for (int o = 1; o < S::G; o <<= 1) { hi += __shfl_xor(hi, o, 64); lo += __shfl_xor(lo, o, 64); zeros += __shfl_xor(zeros, o, 64); }
    return hb_estimate(hi, lo, zeros, (double)S::M, alpha_mm);
}

template <int LOG2M> __global__ void hb_init_kernel(uint8_t* cur, int64_t n, uint64_t seed) {
    using S = Shape<LOG2M>;
    constexpr int PIECES = S::M / 16;
    BVG_FOR(i, n * PIECES) {
        const int64_t x = i / PIECES; const unsigned piece = (unsigned)(i % PIECES);
        const uint64_t h = hb_mix64((uint64_t)x + (seed + 1) * 0x9E3779B97F4A7C15ull);
        const unsigned j = (unsigned)(h & (uint64_t)(S::M - 1));
        const uint32_t r = (uint32_t)__builtin_ctzll((h >> LOG2M) | (1ull << (64 - LOG2M))) + 1;
        uint32_t w[4] = {0, 0, 0, 0};
        if ((j >> 4) == piece) w[(j & 15) >> 2] = r << (8 * (j & 3));
        ((uint4*)cur)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

struct IterArgs {
    const uint64_t* cum; const int64_t* succ; int64_t lo, cnt, n;
    const uint8_t* cur; uint8_t* next; const uint32_t* cur_mod; uint32_t* next_mod;
    float* sod; float* sid; double dist;            // dist = iteration + 1
    double alpha_mm; double* partial; unsigned long long* ctl;
};

template <int LOG2M> struct Finish {
    using S = Shape<LOG2M>;
    // The list of node x is done: t = its new counter, c = the current one, both on the lanes of a group.  act: the group holds a list; own: it is the
    // one that records it (after a walk by the whole wavefront every group holds the same t).  Every lane of the wavefront calls.  Returns modified.
    static __device__ __forceinline__ bool run(const IterArgs& a, bool act, bool own, int64_t x, unsigned q, unsigned grp, const Regs<S::K>& c, const Regs<S::K>& t, double& nf) {
        bool diff = false;
#pragma unroll
        for (int k = 0; k < S::K; k++) diff |= (t.v[k].x != c.v[k].x) | (t.v[k].y != c.v[k].y) | (t.v[k].z != c.v[k].z) | (t.v[k].w != c.v[k].w);
        const uint64_t dm = __ballot(act && diff);
        const uint64_t gmask = S::G == 64 ? ~0ull : ((1ull << S::G) - 1) << (grp * S::G);
        const bool modified = act && (dm & gmask) != 0;
        const double post = count_regs<LOG2M>(t, a.alpha_mm);
        if (act && own && q == 0) nf += post;
        if ((a.sod || a.sid) && __ballot(modified)) {                                // (uniform)
            const double pre = count_regs<LOG2M>(c, a.alpha_mm);
            const double delta = post - pre;
            if (modified && own && q == 0 && delta > 0) {
                if (a.sod) a.sod[x] += (float)(delta * a.dist);
                if (a.sid) a.sid[x] += (float)(delta / a.dist);
            }
        }
        if (act && own && (modified || ((a.cur_mod[x >> 5] >> (x & 31)) & 1u))) {
            uint4* p = (uint4*)(a.next + ((uint64_t)x << LOG2M)) + q;
#pragma unroll
            for (int k = 0; k < S::K; k++) p[k * S::G] = t.v[k];
        }
        return modified && own;
    }
};

template <int LOG2M> __global__ void __launch_bounds__(256) hb_iterate_kernel(const IterArgs a) {
    using S = Shape<LOG2M>;
    __shared__ int64_t pass_s[4][64];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned grp = lane / S::G, q = lane % S::G;
    int64_t* const passed_y = pass_s[w];
    bool oob = false;
    uint64_t n_passed = 0, n_modified = 0;
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < a.cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const bool valid = x0 + lane < a.cnt;
        const uint64_t bq = valid ? a.cum[x0 + lane] : 0, eq = valid ? a.cum[x0 + lane + 1] : 0;   // lane i: the arcs of list i
        const bool wide = valid && (S::P == 1 || eq - bq >= kLong);
        double nf = 0;
        uint64_t modmask = 0;                                                        // bit i: list i modified (kept by the lane that recorded it)
        if (S::P > 1) {
            for (int r0 = 0; r0 < 64; r0 += S::P) {                                  // the short lists, P at a time: one per group
                const int li = r0 + (int)grp;
                const uint64_t b = __shfl(bq, li, 64), e = __shfl(eq, li, 64);
                const bool act = x0 + li < a.cnt && e - b < kLong;
                if (!__ballot(act)) continue;                                        // (uniform)
                const int64_t x = a.lo + x0 + li;
                Regs<S::K> c, t;
#pragma unroll
                for (int k = 0; k < S::K; k++) c.v[k] = make_uint4(0, 0, 0, 0);
                if (act) c = load_counter<LOG2M>(a.cur, x, q);
                t = c;
                if (act) for (uint64_t i = b; i < e; i++) {
                    const int64_t s = a.succ[i];
                    if ((uint64_t)s >= (uint64_t)a.n) { oob = true; continue; }      // malformed stream: flagged, never used as an index
                    if (s == x || !((a.cur_mod[s >> 5] >> (s & 31)) & 1u)) continue;
                    if (q == 0) n_passed++;
                    const Regs<S::K> u = load_counter<LOG2M>(a.cur, s, q);
#pragma unroll
                    for (int k = 0; k < S::K; k++) t.v[k] = max_u8x16(t.v[k], u.v[k]);
                }
                if (Finish<LOG2M>::run(a, act, true, x, q, grp, c, t, nf) && q == 0) modmask |= 1ull << li;
            }
        }
        uint64_t todo = __ballot(wide);
        while (todo) {                                                               // (uniform) one list on the whole wavefront
            const int li = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t b = __shfl(bq, li, 64), e = __shfl(eq, li, 64);
            const int64_t x = a.lo + x0 + li;
            Regs<S::K> t;
#pragma unroll
            for (int k = 0; k < S::K; k++) t.v[k] = make_uint4(0, 0, 0, 0);
            for (uint64_t i0 = b; i0 < e; i0 += 64) {                                // (uniform trip count)
                const uint64_t i = i0 + lane;
                bool pass = false; int64_t s = 0;
                if (i < e) {
                    s = a.succ[i];
                    if ((uint64_t)s >= (uint64_t)a.n) oob = true;
                    else pass = s != x && ((a.cur_mod[s >> 5] >> (s & 31)) & 1u);
                }
                const uint64_t pm = __ballot(pass);
                if (!pm) continue;
                const unsigned np = (unsigned)__builtin_popcountll(pm);
                if (pass) passed_y[__builtin_popcountll(pm & ((1ull << lane) - 1))] = s;
                __builtin_amdgcn_wave_barrier();                                     // (LDS operations of one wavefront complete in order)
                for (unsigned k = grp; k < np; k += S::P) {
                    const Regs<S::K> u = load_counter<LOG2M>(a.cur, passed_y[k], q);
#pragma unroll
                    for (int kk = 0; kk < S::K; kk++) t.v[kk] = max_u8x16(t.v[kk], u.v[kk]);
                }
                __builtin_amdgcn_wave_barrier();                                     // (the next chunk's LDS writes after every lane's reads)
                if (lane == 0) n_passed += np;
            }
#pragma unroll
            for (int o = S::G; o < 64; o <<= 1) {                                    // the groups' maxima combined: every group ends with all of it
#pragma unroll
                for (int k = 0; k < S::K; k++) {
                    const uint4 v = t.v[k];
                    const uint4 u = make_uint4(__shfl_xor(v.x, o, 64), __shfl_xor(v.y, o, 64), __shfl_xor(v.z, o, 64), __shfl_xor(v.w, o, 64));
                    t.v[k] = max_u8x16(v, u);
                }
            }
            const Regs<S::K> c = load_counter<LOG2M>(a.cur, x, q);
#pragma unroll
            for (int k = 0; k < S::K; k++) t.v[k] = max_u8x16(t.v[k], c.v[k]);
            if (Finish<LOG2M>::run(a, true, grp == 0, x, q, grp, c, t, nf) && q == 0) modmask |= 1ull << li;
        }
        // the wavefront's results: its partial of the neighbourhood function (fixed tree), its modified bits
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { nf += __shfl_xor(nf, o, 64); modmask |= __shfl_xor(modmask, o, 64); }
        if (lane == 0) { a.partial[x0 >> 6] = nf; n_modified += (uint64_t)__builtin_popcountll(modmask); }
        if (lane < 3 && modmask) {                                                   // bit (lo + x0 + i) of the bitmap, words shared with the neighbours
            const uint64_t first = (uint64_t)(a.lo + x0);
            const unsigned sh = (unsigned)(first & 31);
            const uint32_t word = lane == 0 ? (uint32_t)(modmask << sh) : lane == 1 ? (uint32_t)(modmask >> (32 - sh)) : (sh ? (uint32_t)(modmask >> (64 - sh)) : 0u);
            if (word) atomicOr(a.next_mod + (first >> 5) + lane, word);
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) n_passed += __shfl_xor(n_passed, o, 64);
    if (lane == 0) {
        if (n_passed) atomicAdd(a.ctl + kCtlPassed, (unsigned long long)n_passed);
        if (n_modified) atomicAdd(a.ctl + kCtlModified, (unsigned long long)n_modified);
    }
    if (oob) atomicOr(a.ctl + kCtlBad, 1ull);
}

// *total += the partials, in a fixed order: thread i takes partials i, i + 256, ..., then a tree over the 256 sums
__global__ void __launch_bounds__(256) hb_reduce_kernel(const double* partial, int64_t count, double* total) {
    __shared__ double s[256];
    double acc = 0;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total += s[0];
}

__global__ void hb_fill_mod_kernel(uint32_t* mod, int64_t n, int64_t words) {
    BVG_FOR(i, words) {
        const int64_t first = i * 32;
        mod[i] = first + 32 <= n ? 0xFFFFFFFFu : first >= n ? 0u : (1u << (unsigned)(n - first)) - 1u;
    }
}

// the estimates of counters [from, to): one thread per counter (not a hot path)
__global__ void hb_counts_kernel(const uint8_t* cur, int64_t from, int64_t to, int log2m, double alpha_mm, double* out) {
    BVG_FOR(i, to - from) {
        const uint32_t* p = (const uint32_t*)(cur + ((uint64_t)(from + i) << log2m));
        uint64_t hi = 0, lo = 0; uint32_t zeros = 0;
        for (int k = 0; k < (1 << log2m) / 4; k++) tally4(p[k], hi, lo, zeros);
        out[i] = hb_estimate(hi, lo, zeros, (double)(1 << log2m), alpha_mm);
    }
}

// the centralities of HyperBall.main (HyperBall.java:1349-1388)
__global__ void hb_centrality_kernel(int which, const float* sod, const float* sid, const double* count, int64_t n, float* out) {
    BVG_FOR(x, n) {
        float r = 0;
        switch (which) {
            case BVG_HB_WHICH_SUM_OF_DISTANCES: r = sod[x]; break;
            case BVG_HB_WHICH_HARMONIC: r = sid[x]; break;
            case BVG_HB_WHICH_CLOSENESS: { const float d = sod[x]; r = d == 0 ? 0.0f : 1.0f / d; break; }
            case BVG_HB_WHICH_LIN: { const float d = sod[x]; r = d == 0 ? 1.0f : (float)(count[x] * count[x] / (double)d); break; }
            case BVG_HB_WHICH_NIEMINEN: r = (float)(count[x] * count[x] - (double)sod[x]); break;
            default: r = (float)count[x]; break;
        }
        out[x] = r;
    }
}

}  // namespace

}  // namespace bvg

using bvghost::Batch;

namespace {

double alpha_mm_of(int log2m) {
    const double m = (double)(1 << log2m);
    const double alpha = log2m == 4 ? 0.673 : log2m == 5 ? 0.697 : log2m == 6 ? 0.709 : 0.7213 / (1 + 1.079 / m);
    return alpha * m * m;
}

}  // namespace

struct bvg_hyperball {
    bvg_graph* g = nullptr;                        // a bvg_copy() flyweight: own stream and workspaces
    int log2m = 0; uint32_t flags = 0; uint64_t seed = 0;
    int64_t n = 0, mod_words = 0;
    DevArray<uint8_t> buf[2], ws; DevArray<uint32_t> mod[2]; DevArray<float> sod, sid; DevArray<unsigned long long> ctl;
    int cur = 0;                                   // buf[cur] / mod[cur]: the current counters and their modified bits
    bool inited = false;
    int64_t iteration = -1; uint64_t modified = 0; double relative_increment = 0;
    std::vector<double> nf;
    // the graph in arc-bounded node ranges, planned at the first iteration; its extra region: one partial sum per wavefront of the widest batch
    bool planned = false; bvghost::SweepPlan sweep;
    ~bvg_hyperball() { if (g) { (void)hipSetDevice(g->sh->device); bvg_close(g); } }
};

namespace {

int ensure_plan(bvg_hyperball* h) {
    if (h->planned) return 0;
    bvg_graph* g = h->g;
    index_first(g);
    uint64_t per = 0;                                                            // (of what is free with the counters in place)
    int rc = arc_budget(h->n, kMaxBatchArcs, "BVG_HB_BATCH_ARCS", &per); if (rc) return rc;
    bvghost::SweepPlan sp;
    rc = sp.build(g, per, true); if (rc) return rc;                              // every node has a counter to carry over and to count, its list empty or not
    sp.layout(((size_t)sp.maxn / 64 + 1) * 8);
    if (h->ws.alloc(sp.bytes)) return BVG_E_NOMEM;                               // counters + the largest batch: does not fit
    sp.bind(h->ws.get());
    h->sweep = std::move(sp); h->planned = true;
    return 0;
}

template <int LOG2M> void launch_init(bvg_hyperball* h) {
    hipLaunchKernelGGL((hb_init_kernel<LOG2M>), dim3(grid(h->n * (int64_t)((1 << LOG2M) / 16), 256)), dim3(256), 0, h->g->stream, h->buf[h->cur].get(), h->n, h->seed);
}
template <int LOG2M> void launch_iterate(bvg_hyperball* h, const IterArgs& a) {
    hipLaunchKernelGGL((hb_iterate_kernel<LOG2M>), dim3(grid(a.cnt, 256)), dim3(256), 0, h->g->stream, a);
}
#define HB_DISPATCH(FN, ...)                                                                  \
    switch (h->log2m) {                                                                       \
        case 4: FN<4>(__VA_ARGS__); break;   case 5: FN<5>(__VA_ARGS__); break;   case 6: FN<6>(__VA_ARGS__); break;   \
        case 7: FN<7>(__VA_ARGS__); break;   case 8: FN<8>(__VA_ARGS__); break;   case 9: FN<9>(__VA_ARGS__); break;   \
        case 10: FN<10>(__VA_ARGS__); break; case 11: FN<11>(__VA_ARGS__); break; default: FN<12>(__VA_ARGS__); break; \
    }

int init_impl(bvg_hyperball* h, uint64_t seed) {
    bvg_graph* g = h->g;
    h->seed = seed; h->cur = 0; h->inited = false;
    if (h->n) {
        HB_DISPATCH(launch_init, h);
        hipLaunchKernelGGL(hb_fill_mod_kernel, dim3(grid(h->mod_words, 256)), dim3(256), 0, g->stream, h->mod[0].get(), h->n, h->mod_words);
        if (h->sod.get()) HIPCHK(hipMemsetAsync(h->sod.get(), 0, (size_t)h->n * 4, g->stream));
        if (h->sid.get()) HIPCHK(hipMemsetAsync(h->sid.get(), 0, (size_t)h->n * 4, g->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));
    h->iteration = -1; h->modified = (uint64_t)h->n; h->relative_increment = 0;
    h->nf.assign(1, (double)h->n);
    h->inited = true;
    return 0;
}

int iterate_impl(bvg_hyperball* h) {
    if (!h->inited) return BVG_E_STATE;
    bvg_graph* g = h->g;
    int rc = ensure_plan(h); if (rc) return rc;
    const bool dbgt = dbg_on();
    Stopwatch sw;
    double t_dec = 0, t_it = 0;
    unsigned long long* const ctl = h->ctl.get();
    double* const d_total = (double*)(ctl + kCtlWords);
    const int nxt = h->cur ^ 1;
    HIPCHK(hipMemsetAsync(ctl, 0, (kCtlWords + 1) * 8, g->stream));
    HIPCHK(hipMemsetAsync(h->mod[nxt].get(), 0, (size_t)h->mod_words * 4, g->stream));
    const bvghost::SweepPlan& sp = h->sweep;
    double* const b_part = (double*)sp.extra();
    h->inited = false;                                                       // (an error below leaves half an iteration: init first)
    for (const Batch& b : sp.batches) {
        const int64_t cnt = b.hi - b.lo;
        sw.lap();
        rc = sp.decode(g, b); if (rc) return rc;
        if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_dec += sw.lap(); }
        IterArgs a;
        a.cum = sp.cum(); a.succ = sp.succ(); a.lo = b.lo; a.cnt = cnt; a.n = h->n;
        a.cur = h->buf[h->cur].get(); a.next = h->buf[nxt].get();
        a.cur_mod = h->mod[h->cur].get(); a.next_mod = h->mod[nxt].get();
        a.sod = h->sod.get(); a.sid = h->sid.get(); a.dist = (double)(h->iteration + 2);
        a.alpha_mm = alpha_mm_of(h->log2m); a.partial = b_part; a.ctl = ctl;
        HB_DISPATCH(launch_iterate, h, a);
        hipLaunchKernelGGL(hb_reduce_kernel, dim3(1), dim3(256), 0, g->stream, (const double*)b_part, (cnt + 63) / 64, d_total);
        HIPCHK(hipGetLastError());
        if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_it += sw.lap(); }
    }
    unsigned long long hc[kCtlWords + 1] = {};
    HIPCHK(hipMemcpyAsync(hc, ctl, sizeof hc, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (hc[kCtlBad]) return BVG_E_EOF;                                       // a successor outside [0, n): malformed stream
    double current; memcpy(&current, hc + kCtlWords, 8);
    h->cur = nxt; h->iteration++; h->modified = hc[kCtlModified];
    const double last = h->nf.back();
    if (current < last) current = last;                                      // monotone (HyperBall.java:1165)
    h->relative_increment = current / last;
    h->nf.push_back(current);
    h->inited = true;
    if (dbgt) fprintf(stderr, "[bvg] hyperball: iteration %lld: %zu batches, decode %.3f ms, iterate %.3f ms, arcs %llu, passed %llu, modified %llu\n", (long long)h->iteration,
                      sp.batches.size(), t_dec, t_it, (unsigned long long)sp.arcs, hc[kCtlPassed], hc[kCtlModified]);
    return 0;
}

int counts_impl(bvg_hyperball* h, int64_t from, int64_t to, double* out, bool dev) {
    if (!h->inited) return BVG_E_STATE;
    if (from < 0 || to < from || to > h->n || (!out && to > from)) return BVG_E_ARG;
    if (to == from) return 0;
    bvg_graph* g = h->g;
    double* d_out = out;
    DevArray<double> tmp;
    if (!dev) { if (tmp.alloc((size_t)(to - from))) return BVG_E_NOMEM; d_out = tmp; }
    hipLaunchKernelGGL(hb_counts_kernel, dim3(grid(to - from, 256)), dim3(256), 0, g->stream, h->buf[h->cur].get(), from, to, h->log2m, alpha_mm_of(h->log2m), d_out);
    HIPCHK(hipGetLastError());
    if (!dev) HIPCHK(hipMemcpyAsync(out, d_out, (size_t)(to - from) * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

int centrality_impl(bvg_hyperball* h, int which, float* out, bool dev) {
    if (which < BVG_HB_WHICH_SUM_OF_DISTANCES || which > BVG_HB_WHICH_REACHABLE || (!out && h->n)) return BVG_E_ARG;
    const bool need_sod = which == BVG_HB_WHICH_SUM_OF_DISTANCES || which == BVG_HB_WHICH_CLOSENESS || which == BVG_HB_WHICH_LIN || which == BVG_HB_WHICH_NIEMINEN;
    if ((need_sod && !h->sod.get()) || (which == BVG_HB_WHICH_HARMONIC && !h->sid.get()) || !h->inited) return BVG_E_STATE;
    if (!h->n) return 0;
    bvg_graph* g = h->g;
    const bool need_count = which == BVG_HB_WHICH_LIN || which == BVG_HB_WHICH_NIEMINEN || which == BVG_HB_WHICH_REACHABLE;
    DevArray<double> cnt; DevArray<float> tmp;
    if (need_count) {
        if (cnt.alloc((size_t)h->n)) return BVG_E_NOMEM;
        const int rc = counts_impl(h, 0, h->n, cnt.get(), true); if (rc) return rc;
    }
    float* d_out = out;
    if (!dev) { if (tmp.alloc((size_t)h->n)) return BVG_E_NOMEM; d_out = tmp; }
    hipLaunchKernelGGL(hb_centrality_kernel, dim3(grid(h->n, 256)), dim3(256), 0, g->stream, which, h->sod.get(), h->sid.get(), cnt.get(), h->n, d_out);
    HIPCHK(hipGetLastError());
    if (!dev) HIPCHK(hipMemcpyAsync(out, d_out, (size_t)h->n * 4, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

}  // namespace

extern "C" {

int bvg_hyperball_create(bvg_graph* g, int log2m, uint32_t flags, uint64_t seed, bvg_hyperball** out) {
    if (!g || !out || log2m < 4 || (flags & ~(uint32_t)(BVG_HB_SUM_OF_DISTANCES | BVG_HB_HARMONIC))) return BVG_E_ARG;
    *out = nullptr;
    if (log2m > 12) return BVG_E_UNSUPPORTED;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    return bvghost::guarded([&]() -> int {
        HIPCHK(hipSetDevice(g->sh->device));
        std::unique_ptr<bvg_hyperball> h(new bvg_hyperball);
        int rc = bvg_copy(g, &h->g); if (rc) { h->g = nullptr; return rc; }
        h->log2m = log2m; h->flags = flags; h->seed = seed;
        h->n = g->sh->p.nodes;
        h->mod_words = (h->n + 31) / 32 + 3;                 // (a wavefront's 64 bits may reach into the third word from its first)
        const size_t bytes = (size_t)std::max<int64_t>(h->n, 1) << log2m;
        if (h->buf[0].alloc(bytes) || h->buf[1].alloc(bytes) || h->mod[0].alloc((size_t)h->mod_words) || h->mod[1].alloc((size_t)h->mod_words) || h->ctl.alloc(32)) return BVG_E_NOMEM;
        if ((flags & BVG_HB_SUM_OF_DISTANCES) && h->sod.alloc((size_t)std::max<int64_t>(h->n, 1))) return BVG_E_NOMEM;
        if ((flags & BVG_HB_HARMONIC) && h->sid.alloc((size_t)std::max<int64_t>(h->n, 1))) return BVG_E_NOMEM;
        *out = h.release();
        return 0;
    });
}

void bvg_hyperball_close(bvg_hyperball* h) { delete h; }

int bvg_hyperball_init(bvg_hyperball* h, uint64_t seed) { return on_device(h, [&] { return init_impl(h, seed); }); }

int bvg_hyperball_iterate(bvg_hyperball* h) { return on_device(h, [&] { return iterate_impl(h); }); }

int bvg_hyperball_run(bvg_hyperball* h, int64_t upper_bound, double threshold) {
    return on_device(h, [&]() -> int {
        if (upper_bound < 0 || upper_bound > h->n) upper_bound = h->n;       // (negative: no bound)
        int rc = init_impl(h, h->seed); if (rc) return rc;
        for (int64_t i = 0; i < upper_bound; i++) {
            rc = iterate_impl(h); if (rc) return rc;
            if (h->modified == 0) break;
            if (i > 3 && h->relative_increment < 1 + threshold) break;
        }
        return 0;
    });
}

int bvg_hyperball_info(const bvg_hyperball* h, int64_t* iteration, uint64_t* modified, double* relative_increment, uint64_t* nf_len) {
    if (!h) return BVG_E_ARG;
    if (iteration) *iteration = h->iteration;
    if (modified) *modified = h->modified;
    if (relative_increment) *relative_increment = h->relative_increment;
    if (nf_len) *nf_len = h->nf.size();
    return 0;
}

int bvg_hyperball_neighbourhood_function(const bvg_hyperball* h, double* out, uint64_t cap) {
    if (!h || (!out && !h->nf.empty())) return BVG_E_ARG;
    if (cap < h->nf.size()) return BVG_E_CAPACITY;
    if (!h->nf.empty()) memcpy(out, h->nf.data(), h->nf.size() * 8);
    return 0;
}

int bvg_hyperball_registers(bvg_hyperball* h, int64_t from, int64_t to, uint8_t* out) {
    if (!h || from < 0 || to < from || to > h->n || (!out && to > from)) return BVG_E_ARG;
    return on_device(h, [&]() -> int {
        if (!h->inited) return BVG_E_STATE;
        if (to > from) HIPCHK(hipMemcpy(out, h->buf[h->cur].get() + ((size_t)from << h->log2m), (size_t)(to - from) << h->log2m, hipMemcpyDeviceToHost));
        return 0;
    });
}

int bvg_hyperball_counts(bvg_hyperball* h, int64_t from, int64_t to, double* out) { return on_device(h, [&] { return counts_impl(h, from, to, out, false); }); }
int bvg_hyperball_counts_dev(bvg_hyperball* h, int64_t from, int64_t to, void* d_out) { return on_device(h, [&] { return counts_impl(h, from, to, (double*)d_out, true); }); }

int bvg_hyperball_centrality(bvg_hyperball* h, int which, float* out) { return on_device(h, [&] { return centrality_impl(h, which, out, false); }); }
int bvg_hyperball_centrality_dev(bvg_hyperball* h, int which, void* d_out) { return on_device(h, [&] { return centrality_impl(h, which, (float*)d_out, true); }); }

double bvg_hyperball_relative_standard_deviation(int log2m) {
    static const double beta[] = {1.106, 1.070, 1.054, 1.046};
    if (log2m < 1 || log2m > 62) return 0;
    return (log2m >= 4 && log2m <= 7 ? beta[log2m - 4] : 1.04) / sqrt((double)(1ull << log2m));
}

}  // extern "C"
