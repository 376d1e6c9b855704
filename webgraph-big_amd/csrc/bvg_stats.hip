// bvg_stats.hip — graph statistics on the device (Stats.java): degree distributions, gaps, locality, in one sweep of the compressed graph.
//
// The reference makes one sequential pass over all successor lists (Stats.run, Stats.java:96-281).  Here the same numbers come from
//   degrees   the outdegrees of all nodes (one code each, no list decoded): dangling nodes, min / max outdegree and their nodes, the
//             outdegree distribution.  Every node is seen here, also those the batch plan of the sweep leaves out (runs of empty lists);
//   sweep     the arc-bounded sweep of bvg_plan.hip; per batch one kernel with the lane-to-arc mapping of bvg_arcwalk.h: per list the
//             gap terms and the d == 1 self-loops (terminal nodes), per arc (x, y) indegree[y] += 1, |y - x| into the locality sum, a
//             loop or bin msb(|y - x|) of the 64-bin histogram;
//   indegrees min / max with their nodes and the indegree distribution from the per-node counters.
//
// Ties.  The reference scans outdegrees in increasing node order and indegrees from node n - 1 downwards, both with strict comparisons
// (Stats.java:145-153, 212-228): the smallest node wins min and max outdegree, the largest node wins min and max indegree.
//
// Sums.  tot_gap and tot_loc are 128-bit: every level adds with carry -- a lane keeps two words, the wavefront reduction and the
// workgroup's sum in LDS carry, and the global accumulator is two words: the low word's atomic add returns the old value, the adder
// that wraps it is the one that adds the carry to the high word.  All other counters are bounded by the arc count.
//
// Scalar counters never cost a global atomic per arc: they are folded per lane, per wavefront (the 64 bins by ballots: lane b counts
// the arcs of bin b), per workgroup in LDS, then one global atomic per counter and workgroup.  The indegree scatter has two forms
// (DESIGN.md 7g): one relaxed agent-scope atomic per arc, or lanes of a wavefront that hold the same target elect one adder.
#include <cstdint>
#include <cstring>
#include <vector>

#include "bvg_arcwalk.h"
#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

// words of the global accumulator
enum : int { kLoops = 0, kTerm1, kNumGaps, kGapLo, kGapHi, kLocLo, kLocHi, kBad, kBins, kAccWords = kBins + 64 };
constexpr int kPartWords = 7;                     // kLoops .. kLocHi: what a wavefront hands to its workgroup

struct U128 {
    unsigned long long lo, hi;
    __device__ __forceinline__ void add(unsigned long long v) { lo += v; hi += lo < v ? 1ull : 0ull; }
    __device__ __forceinline__ void add(const U128& o) { lo += o.lo; hi += o.hi + (lo < o.lo ? 1ull : 0ull); }
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ U128 wave_sum(U128 v) {
    for (int s = 32; s; s >>= 1) { U128 o; o.lo = __shfl_xor(v.lo, s, 64); o.hi = __shfl_xor(v.hi, s, 64); v.add(o); }
    return v;
}

// acc[lo_word .. lo_word + 1] += v: the add that wraps the low word carries into the high word
__device__ __forceinline__ void global_add128(unsigned long long* acc, int lo_word, const U128& v) {
    unsigned long long carry = 0;
    if (v.lo) { const unsigned long long old = atomicAdd(acc + lo_word, v.lo); carry = old + v.lo < old ? 1ull : 0ull; }
    if (v.hi + carry) atomicAdd(acc + lo_word + 1, v.hi + carry);           // (v.hi + carry < 2^64: v.hi counts wraps of sums of fewer than 2^64 terms)
}

// indegree[y] += 1 for the lanes with `ok`.  ELECT: the lanes of the wavefront that hold the same y add once, their number (all 64
// lanes are here: the caller's loop is uniform)
template <typename T, bool ELECT> __device__ __forceinline__ void scatter(T* indeg, int64_t y, bool ok, unsigned lane) {
    if (!ELECT) {
        if (ok) (void)__hip_atomic_fetch_add(indeg + y, (T)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    uint64_t rem = __ballot(ok);
    while (rem) {
        const int leader = __builtin_ctzll(rem);
        const int64_t v = __shfl(y, leader, 64);
        const uint64_t same = __ballot(ok && y == v);
        if ((int)lane == leader) (void)__hip_atomic_fetch_add(indeg + v, (T)__builtin_popcountll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rem &= ~same;
    }
}

// One wavefront per 64 consecutive nodes of the batch [lo, lo + cnt) (four per workgroup): first the 64 lists' own terms (one lane each),
// then the lists' arcs, walked as bvg_arcwalk.h describes.  The walk is the uniform one (a lane without an arc stays in it), so the
// ballots see all 64 lanes.  A target outside [0, n) is a malformed stream: flagged in acc[kBad] and not counted anywhere.
template <typename T, bool ELECT> __global__ void __launch_bounds__(256) stats_sweep_kernel(const uint64_t* cum, int64_t lo, int64_t cnt, const int64_t* succ, int64_t n,
                                                                                            T* indeg, unsigned long long* acc) {
    __shared__ ArcWalk walk_s[4];
    __shared__ unsigned long long part_s[4][kPartWords + 1];
    __shared__ unsigned long long bins_s[64];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ArcWalk& walk = walk_s[w];
    if (threadIdx.x < 64) bins_s[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long loops = 0, term1 = 0, ngaps = 0, bin = 0;           // bin: the arcs of histogram bin `lane`
    U128 gap{0, 0}, loc{0, 0};
    bool oob = false;
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const int64_t i = x0 + lane;
        const bool valid = i < cnt;
        const uint64_t b = valid ? cum[i] : 0, e = valid ? cum[i + 1] : 0;
        const uint64_t d = e - b;
        if (d) {
            const int64_t x = lo + i, first = succ[b];
            if (d == 1) term1 += first == x ? 1 : 0;
            else {                                                          // Stats.java:124-128: d, not d - 1; a list of one arc adds nothing
                const int64_t last = succ[e - 1], v = first - x;
                ngaps += d;
                gap.add((unsigned long long)(last - first));
                gap.add(v >= 0 ? (unsigned long long)v << 1 : (((unsigned long long)(-(v + 1))) << 1) + 1);   // Fast.int2nat
            }
        }
        const uint64_t total = walk.begin(lane, d != 0, b, e, [] {});
        if (total == 0) continue;                                            // (uniform: no list of this group has an arc)
        walk.for_each_chunk(lane, total, [&](bool has, int l, uint64_t at) {
            const int64_t x = lo + x0 + l;
            const int64_t y = has ? succ[at] : 0;
            const bool ok = has && y >= 0 && y < n;
            oob |= has && !ok;
            scatter<T, ELECT>(indeg, y, ok, lane);
            const unsigned long long dist = ok ? (unsigned long long)(y > x ? y - x : x - y) : 0ull;
            loc.add(dist);
            loops += ok && dist == 0 ? 1 : 0;
            const bool nl = ok && dist != 0;
            const unsigned bn = nl ? 63u - (unsigned)__builtin_clzll(dist) : 0u;
            uint64_t mine = __ballot(nl);                                    // the lanes whose arc falls into bin `lane`
            for (int k = 0; k < 6; k++) {
                const uint64_t mk = __ballot(nl && ((bn >> k) & 1u));
                mine &= (lane >> k) & 1u ? mk : ~mk;
            }
            bin += (unsigned long long)__builtin_popcountll(mine);
        });
        walk.end();
    }
    // wavefront -> workgroup (LDS) -> one global atomic per counter
    loops = wave_sum(loops); term1 = wave_sum(term1); ngaps = wave_sum(ngaps);
    gap = wave_sum(gap); loc = wave_sum(loc);
    const uint64_t any_oob = __ballot(oob);
    if (lane == 0) {
        unsigned long long* p = part_s[w];
        p[kLoops] = loops; p[kTerm1] = term1; p[kNumGaps] = ngaps; p[kGapLo] = gap.lo; p[kGapHi] = gap.hi; p[kLocLo] = loc.lo; p[kLocHi] = loc.hi;
        p[kPartWords] = any_oob ? 1ull : 0ull;
    }
    if (bin) atomicAdd(&bins_s[lane], bin);
    __syncthreads();
    if (w == 0) {
        if (lane <= kNumGaps) {                                             // sums of at most `arcs` ones: no wrap
            const unsigned long long v = part_s[0][lane] + part_s[1][lane] + part_s[2][lane] + part_s[3][lane];
            if (v) atomicAdd(acc + lane, v);
        } else if (lane == kGapLo || lane == kLocLo) {
            U128 s{0, 0};
            for (int i = 0; i < 4; i++) { U128 o{part_s[i][lane], part_s[i][lane + 1]}; s.add(o); }
            global_add128(acc, (int)lane, s);
        } else if (lane == kBad) {
            if (part_s[0][kPartWords] | part_s[1][kPartWords] | part_s[2][kPartWords] | part_s[3][kPartWords]) atomicOr(acc + kBad, 1ull);
        }
    } else if (w == 1) {
        const unsigned long long v = bins_s[lane];
        if (v) atomicAdd(acc + kBins + lane, v);
    }
}

// ---- min / max with their nodes over a per-node array, and the number of zeros

struct Extremes { unsigned long long minv, maxv; long long minn, maxn; };   // minn < 0: nothing seen yet
constexpr int kExtWords = 5;                                                 // per wavefront: minv, minn, maxv, maxn, zeros

// is (v, x) a better minimum (LESS) / maximum than (bv, bx)?  Ties go to the larger node when LARGE, else to the smaller
template <bool LARGE, bool LESS> __device__ __forceinline__ bool better(unsigned long long v, long long x, unsigned long long bv, long long bx) {
    if (x < 0) return false;
    if (bx < 0) return true;
    if (v != bv) return LESS ? v < bv : v > bv;
    return LARGE ? x > bx : x < bx;
}

// out[wavefront * kExtWords ..]: the extremes of the elements the wavefront saw (LARGE: the tie rule) and how many are zero
template <typename V, bool LARGE> __global__ void __launch_bounds__(256) stats_extremes_kernel(const V* val, int64_t n, unsigned long long* out) {
    Extremes e{0, 0, -1, -1};
    unsigned long long zeros = 0;
    BVG_FOR(x, n) {
        const unsigned long long v = (unsigned long long)val[x];
        if (better<LARGE, true>(v, x, e.minv, e.minn)) { e.minv = v; e.minn = x; }
        if (better<LARGE, false>(v, x, e.maxv, e.maxn)) { e.maxv = v; e.maxn = x; }
        zeros += v == 0 ? 1 : 0;
    }
    for (int s = 32; s; s >>= 1) {
        const unsigned long long ov = __shfl_xor(e.minv, s, 64), pv = __shfl_xor(e.maxv, s, 64);
        const long long on = __shfl_xor(e.minn, s, 64), pn = __shfl_xor(e.maxn, s, 64);
        if (better<LARGE, true>(ov, on, e.minv, e.minn)) { e.minv = ov; e.minn = on; }
        if (better<LARGE, false>(pv, pn, e.maxv, e.maxn)) { e.maxv = pv; e.maxn = pn; }
    }
    zeros = wave_sum(zeros);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* p = out + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kExtWords;
        p[0] = e.minv; p[1] = (unsigned long long)e.minn; p[2] = e.maxv; p[3] = (unsigned long long)e.maxn; p[4] = zeros;
    }
}

// ---- count of counts: dist[val[x]] += 1.  The low values take most increments (count[1]: 42 % of cnr-2000's indegrees), so each
// workgroup counts values below kLowBins in LDS and flushes the bins it touched once; the tail goes to global memory directly

constexpr int kLowBins = 1024;
template <typename V> __global__ void __launch_bounds__(256) stats_distribution_kernel(const V* val, int64_t n, unsigned long long* dist, uint64_t len) {
    __shared__ unsigned long long low_s[kLowBins];
    for (int i = threadIdx.x; i < kLowBins; i += 256) low_s[i] = 0;
    __syncthreads();
    BVG_FOR(x, n) {
        const unsigned long long v = (unsigned long long)val[x];
        if (v < (unsigned long long)kLowBins) atomicAdd(&low_s[v], 1ull);
        else if (v < len) atomicAdd(dist + v, 1ull);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLowBins; i += 256) {
        const unsigned long long c = low_s[i];
        if (c && (uint64_t)i < len) atomicAdd(dist + i, c);
    }
}

}  // namespace

}  // namespace bvg

struct bvg_stats {
    int device = 0;
    int64_t n = 0;
    bool wide = false;                                // the per-node indegrees are uint64 (else uint32)
    DevArray<uint8_t> indeg;                          // (bytes: 4 or 8 per node) kept with BVG_STATS_KEEP_INDEGREES
    bool keep = false;
    bvg_stats_summary sum{};
    std::vector<uint64_t> dist[2];                    // [BVG_STATS_OUT], [BVG_STATS_IN]
};

namespace {

constexpr unsigned kExtGrid = 1024;                   // workgroups of the extremes pass: 4096 partial results for the host to fold

// the scatter form: one atomic per arc unless BVG_STATS_SCATTER=elect (test knob; DESIGN.md 7g holds the measurements)
bool scatter_elect() { const char* k = knob("BVG_STATS_SCATTER"); return k && !strcmp(k, "elect"); }

struct HostExtremes { uint64_t minv = 0, maxv = 0; int64_t minn = -1, maxn = -1; uint64_t zeros = 0; };

template <typename V, bool LARGE> int extremes_of(bvg_graph* g, const V* d_val, int64_t n, HostExtremes* out) {
    const unsigned blocks = std::min<unsigned>(kExtGrid, grid(n, 256));
    const size_t words = (size_t)blocks * 4 * kExtWords;
    DevArray<unsigned long long> part;
    if (part.alloc(words)) return BVG_E_NOMEM;
    hipLaunchKernelGGL((stats_extremes_kernel<V, LARGE>), dim3(blocks), dim3(256), 0, g->stream, d_val, n, part.get());
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> h(words);
    HIPCHK(hipMemcpyAsync(h.data(), part.get(), words * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    HostExtremes e;
    auto better = [](bool less, uint64_t v, int64_t x, uint64_t bv, int64_t bx) {
        if (x < 0) return false;
        if (bx < 0) return true;
        if (v != bv) return less ? v < bv : v > bv;
        return LARGE ? x > bx : x < bx;
    };
    for (size_t i = 0; i < words; i += kExtWords) {
        if (better(true, h[i], (int64_t)h[i + 1], e.minv, e.minn)) { e.minv = h[i]; e.minn = (int64_t)h[i + 1]; }
        if (better(false, h[i + 2], (int64_t)h[i + 3], e.maxv, e.maxn)) { e.maxv = h[i + 2]; e.maxn = (int64_t)h[i + 3]; }
        e.zeros += h[i + 4];
    }
    if (e.maxv == 0) e.maxn = 0;                                            // (the reference's maximum starts at 0 at node 0 and moves on a strict > only)
    *out = e;
    return 0;
}

// the count of counts of d_val[0, n), whose largest value is maxv, into `out` (maxv + 1 entries)
template <typename V> int distribution_of(bvg_graph* g, const V* d_val, int64_t n, uint64_t maxv, std::vector<uint64_t>& out) {
    const uint64_t len = maxv + 1;
    DevArray<unsigned long long> dist;
    if (dist.alloc(len)) return BVG_E_NOMEM;
    HIPCHK(hipMemsetAsync(dist.get(), 0, len * 8, g->stream));
    hipLaunchKernelGGL((stats_distribution_kernel<V>), dim3(std::min<unsigned>(1024, grid(n, 4096))), dim3(256), 0, g->stream, d_val, n, dist.get(), len);
    HIPCHK(hipGetLastError());
    out.resize(len);
    HIPCHK(hipMemcpyAsync(out.data(), dist.get(), len * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

template <typename T> int stats_t(bvg_graph* g, bvg_stats* s) {
    Shared* sh = g->sh; const int64_t n = sh->p.nodes;
    const bool dbgt = dbg_on();
    const bool elect = scatter_elect();
    Stopwatch sw;
    index_first(g);
    if (s->indeg.alloc((size_t)n * sizeof(T))) return BVG_E_NOMEM;
    T* const d_indeg = (T*)s->indeg.get();
    HIPCHK(hipMemsetAsync(d_indeg, 0, (size_t)n * sizeof(T), g->stream));
    bvg_stats_summary& r = s->sum;
    {   // every node's outdegree (4 bytes per node, gone before the batch is sized)
        DevArray<int32_t> deg;
        if (deg.alloc((size_t)n)) return BVG_E_NOMEM;
        outdegrees_of(g, 0, n, deg);
        HostExtremes e;
        int rc = extremes_of<uint32_t, false>(g, (const uint32_t*)deg.get(), n, &e); if (rc) return rc;
        if (e.maxv > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                // (Stats.java:120)
        r.min_outdegree = (int64_t)e.minv; r.min_outdegree_node = e.minn; r.max_outdegree = (int64_t)e.maxv; r.max_outdegree_node = e.maxn;
        r.dangling = e.zeros;
        rc = distribution_of<uint32_t>(g, (const uint32_t*)deg.get(), n, e.maxv, s->dist[BVG_STATS_OUT]); if (rc) return rc;
    }
    DevArray<unsigned long long> accb;
    if (accb.alloc(kAccWords)) return BVG_E_NOMEM;
    unsigned long long h_acc[kAccWords] = {};
    if (const char* k = knob("BVG_STATS_SUM_SEED")) h_acc[kGapLo] = h_acc[kLocLo] = strtoull(k, nullptr, 0);
    HIPCHK(hipMemcpyAsync(accb, h_acc, sizeof h_acc, hipMemcpyHostToDevice, g->stream));
    unsigned long long* const d_acc = accb;
    const double t_deg = sw.lap();
    uint64_t per = 0;                                                       // (of what is free once the indegrees are there)
    int rc = arc_budget(n, kMaxBatchArcs, "BVG_STATS_BATCH_ARCS", &per); if (rc) return rc;
    SweepPlan sp;
    rc = sp.build(g, per); if (rc) return rc;                               // (the nodes it leaves out have no arcs: counted above)
    const double t_plan = sw.lap();
    double t_dec = 0, t_arc = 0;
    if (!sp.batches.empty()) {
        DevArray<uint8_t> ws;
        if (ws.alloc(sp.bytes)) return BVG_E_NOMEM;                         // indegrees + the largest batch: does not fit
        sp.bind(ws.get());
        for (const Batch& b : sp.batches) {
            const int64_t cnt = b.hi - b.lo;
            sw.lap();
            rc = sp.decode(g, b); if (rc) return rc;
            if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_dec += sw.lap(); }
            if (elect) hipLaunchKernelGGL((stats_sweep_kernel<T, true>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const uint64_t*)sp.cum(), b.lo, cnt, (const int64_t*)sp.succ(), n, d_indeg, d_acc);
            else hipLaunchKernelGGL((stats_sweep_kernel<T, false>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const uint64_t*)sp.cum(), b.lo, cnt, (const int64_t*)sp.succ(), n, d_indeg, d_acc);
            HIPCHK(hipGetLastError());
            if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_arc += sw.lap(); }
        }
        HIPCHK(hipStreamSynchronize(g->stream));                            // (the workspace goes: its last kernel first)
    }
    HIPCHK(hipMemcpyAsync(h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (h_acc[kBad]) return BVG_E_EOF;                                      // a successor outside [0, n): malformed stream
    sw.lap();
    r.nodes = (uint64_t)n; r.arcs = sp.arcs; r.loops = h_acc[kLoops]; r.terminal = r.dangling + h_acc[kTerm1]; r.num_gaps = h_acc[kNumGaps];
    r.tot_gap_lo = h_acc[kGapLo]; r.tot_gap_hi = h_acc[kGapHi]; r.tot_loc_lo = h_acc[kLocLo]; r.tot_loc_hi = h_acc[kLocHi];
    for (int i = 0; i < 64; i++) r.log_delta[i] = h_acc[kBins + i];
    HostExtremes e;
    rc = extremes_of<T, true>(g, (const T*)d_indeg, n, &e); if (rc) return rc;
    if (e.maxv > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                    // (Stats.java:217)
    r.min_indegree = (int64_t)e.minv; r.min_indegree_node = e.minn; r.max_indegree = (int64_t)e.maxv; r.max_indegree_node = e.maxn;
    rc = distribution_of<T>(g, (const T*)d_indeg, n, e.maxv, s->dist[BVG_STATS_IN]); if (rc) return rc;
    if (dbgt) fprintf(stderr, "[bvg] stats: degrees %.1f ms, plan %.1f ms (%zu batches of <= %llu arcs, %llu arcs), decode %.1f ms, arcs %.1f ms (%s), indegrees %.1f ms\n",
                      t_deg, t_plan, sp.batches.size(), (unsigned long long)per, (unsigned long long)sp.arcs, t_dec, t_arc, elect ? "elect" : "plain", sw.lap());
    return 0;
}

int stats_impl(bvg_graph* g, uint32_t flags, bvg_stats* s) {
    Shared* sh = g->sh;
    s->device = sh->device; s->n = sh->p.nodes; s->keep = (flags & BVG_STATS_KEEP_INDEGREES) != 0;
    s->wide = sh->wide || g->tun.force_wide;
    s->sum.min_outdegree = s->sum.min_indegree = INT64_MAX;                  // (Stats.java:101, 210: what an empty graph reports)
    s->dist[0].assign(1, 0); s->dist[1].assign(1, 0);
    if (s->n == 0) return 0;
    HIPCHK(hipSetDevice(sh->device));
    const int rc = s->wide ? stats_t<uint64_t>(g, s) : stats_t<uint32_t>(g, s);
    if (rc) return rc;
    if (!s->keep) s->indeg.reset();
    return 0;
}

// indegrees of [from, to) as int64 into out (host or device memory): widened on the host side of the copy or by a strided device copy
template <typename T> __global__ void stats_widen_kernel(const T* in, int64_t cnt, int64_t* out) {
    BVG_FOR(i, cnt) out[i] = (int64_t)in[i];
}

int indegrees_impl(bvg_stats* s, int64_t from, int64_t to, int64_t* out, bool dev) {
    if (!s) return BVG_E_ARG;
    if (from < 0 || to < from || to > s->n) return BVG_E_ARG;
    if (!s->keep) return BVG_E_UNSUPPORTED;
    if (to == from) return 0;
    if (!out) return BVG_E_ARG;
    HIPCHK(hipSetDevice(s->device));
    const int64_t cnt = to - from;
    DevArray<int64_t> tmp;
    int64_t* d_out = out;
    if (!dev) { if (tmp.alloc((size_t)cnt)) return BVG_E_NOMEM; d_out = tmp; }
    if (s->wide) hipLaunchKernelGGL((stats_widen_kernel<uint64_t>), dim3(grid(cnt, 256)), dim3(256), 0, nullptr, (const uint64_t*)s->indeg.get() + from, cnt, d_out);
    else hipLaunchKernelGGL((stats_widen_kernel<uint32_t>), dim3(grid(cnt, 256)), dim3(256), 0, nullptr, (const uint32_t*)s->indeg.get() + from, cnt, d_out);
    HIPCHK(hipGetLastError());
    if (!dev) HIPCHK(hipMemcpy(out, d_out, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    else HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace

int bvg_stats_compute(bvg_graph* g, uint32_t flags, bvg_stats** out) {
    if (!g || !out || (flags & ~(uint32_t)BVG_STATS_KEEP_INDEGREES)) return BVG_E_ARG;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    *out = nullptr;
    return guarded([&]() -> int {
        bvg_stats* s = new bvg_stats();
        const int rc = stats_impl(g, flags, s);
        if (rc) { (void)hipSetDevice(g->sh->device); delete s; return rc; }
        *out = s;
        return 0;
    });
}

void bvg_stats_close(bvg_stats* s) {
    if (!s) return;
    if (s->indeg) (void)hipSetDevice(s->device);
    delete s;
}

int bvg_stats_get(const bvg_stats* s, bvg_stats_summary* out) {
    if (!s || !out) return BVG_E_ARG;
    *out = s->sum;
    return 0;
}

int bvg_stats_distribution(const bvg_stats* s, int which, uint64_t* out, uint64_t cap, uint64_t* len) {
    if (!s || !len || (which != BVG_STATS_OUT && which != BVG_STATS_IN)) return BVG_E_ARG;
    const std::vector<uint64_t>& d = s->dist[which];
    *len = d.size();
    if (cap < d.size()) return BVG_E_CAPACITY;
    if (!out) return BVG_E_ARG;
    memcpy(out, d.data(), d.size() * 8);
    return 0;
}

int bvg_stats_indegrees(bvg_stats* s, int64_t from, int64_t to, int64_t* out) {
    return guarded([&] { return indegrees_impl(s, from, to, out, false); });
}
int bvg_stats_indegrees_dev(bvg_stats* s, int64_t from, int64_t to, void* d_out) {
    return guarded([&] { return indegrees_impl(s, from, to, (int64_t*)d_out, true); });
}
