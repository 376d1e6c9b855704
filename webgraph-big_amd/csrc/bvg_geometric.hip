// bvg_geometric.hip — exact geometric centralities on the device (algo/LinearGeometricCentrality.java).
//
// The reference runs one breadth-first visit per source, each thread with a distance array of its own (LinearGeometricCentrality.java:
// IterationThread), and adds coeff(d) to centrality[source] for every node it discovers at distance d.  Here the visits are bit-parallel:
// the sources [from, to) go in passes of S = 64 W consecutive sources (W = 1, 2, 4 or 8 words per node), source pass_start + j owning bit j.
// Per node three arrays of W 64-bit words, node-major (the W words of a node are contiguous): seen (the sources that have reached the
// node), frontier (those that reached it in the last level) and next (those that reach it in this one).  ONE sweep of the compressed graph
// (SweepPlan, bvg_plan.hip) advances all S visits by one level, so the decode is shared by up to 512 sources.
//
//   pass setup   seen[s] and frontier[s] get bit j of source s = pass_start + j; acc[j] = 0 (double), reach[j] = 1
//   level d      mark kernel after every decoded batch: for every arc x -> y of a list whose frontier[x] has a bit, and every word k,
//                  m = frontier[x][k] & ~seen[y][k]; when m has a bit that a plain load of next[y][k] lacks, an atomic OR of m into next[y][k].
//                advance kernel, once: new = next & ~seen; seen |= new; frontier = new; next = 0; the nodes that gained bit b are counted
//                  per wavefront with ballots, summed in registers over the grid-stride loop and added to cnt[b] with one INTEGER atomic per
//                  lane and wavefront.
//                accumulate kernel, one workgroup: acc[j] += coeff(d) * cnt[j]; reach[j] += cnt[j]; cnt[j] = 0; the level's total is stored
//                  for the host, which reads it back with the malformed-stream flag (one copy per level) and ends the pass when it is 0.
//   end of pass  centrality[s] = (float)(coeff(0) + acc[j]), reachable[s] = reach[j]: the source counts as reachable and coefficient 0 is
//                added once, as in the reference.
// coeff(d) is evaluated on the host, once per level, in double (1.0 / d, libm pow, or the table entry) and passed as a kernel argument.
// No floating-point atomic anywhere: the counts are exact integers, and acc[j] is touched by thread j of one workgroup only.  So every
// output is a function of the graph and the sources alone: seen and frontier are not written during a sweep, a stale load of next can only
// cause a needless atomic (OR is idempotent and commutative), and neither the lane order, nor the batch size, nor W can reach the result.
// hist[d] = the level totals summed over the passes: the exact distance histogram over the chosen sources, and so their exact
// neighbourhood function -- what bvg_hyperball's estimate can be checked against.
//
// DIFFERENCE FROM THE REFERENCE.  It adds coeff to a float32 once per discovered node, so its value carries up to one float rounding per
// reached node.  Here sum_d coeff(d) * N_d is formed in double over the levels and rounded to float once: the reference's value up to
// that accumulated float error, and closer to the exact sum.  PowerLawCoefficients with a negative exponent has coeff(0) = +inf, and so
// every centrality is +inf, as in the reference.
//
// Sweeps.  A plan of one batch is decoded once and stays resident for the whole call (as bvg_scc): a level is then three launches.  With
// several batches every level decodes every batch again.  Memory: 24 W bytes per node, one batch of the decode, O(S) accumulators.
// W: the largest of 1, 2, 4, 8 that does not exceed ceil((to - from) / 64) and whose arrays take at most half of the free memory (the
// rest is the batch's).  On cnr-2000 and an eu-like stand-in of 2^20 nodes, 512 sources, W = 8 was the fastest of the four.  Test knobs: BVG_GEO_WORDS (1, 2, 4, 8) and BVG_GEO_BATCH_ARCS.
//
// NOT BUILT: a route for small frontiers by batched random access, as bvg_bfs has (bvg_successors_batch on the nodes that hold a frontier
// bit): the first levels of a pass, where 64 W nodes hold a bit, still cost a sweep each.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "bvg_arcwalk.h"
#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

enum : int { kCtlBad, kCtlTotal, kCtlWords };                                // control words (unsigned long long) the host reads back every level

template <int W> struct alignas(W >= 2 ? 16 : 8) Words { uint64_t w[W]; };  // the words of one node: one or more 16-byte accesses

// One wavefront per 64 consecutive lists of the batch [lo, lo + cnt) (four per workgroup); the arcs of the lists that take part (some word
// of frontier[x] is non-zero) are walked as bvg_arcwalk.h describes, the lists' frontier words being in LDS next to the list ends.  A target
// outside [0, n) is a malformed stream: it is flagged and never used as an index.
template <int W>
__global__ void __launch_bounds__(256) geo_mark_kernel(const uint64_t* cum, int64_t lo, int64_t cnt, const int64_t* succ, int64_t n, const uint64_t* seen,
                                                       const uint64_t* frontier, uint64_t* next, unsigned long long* ctl) {
    __shared__ ArcWalk walk_s[4];
    __shared__ uint64_t fr_s[4][64 * W];   // frontier[x][k] of list l at l * W + k
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ArcWalk& walk = walk_s[w]; uint64_t* fr = fr_s[w];
    bool oob = false;
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const int64_t i = x0 + lane;
        const bool valid = i < cnt;
        const uint64_t b = valid ? cum[i] : 0, e = valid ? cum[i + 1] : 0;
        Words<W> f = {};
        bool act = false;
        if (valid && e > b) {
            f = *(const Words<W>*)(frontier + (lo + i) * W);
#pragma unroll
            for (int k = 0; k < W; k++) act |= f.w[k] != 0;
        }
        const uint64_t total = walk.begin(lane, act, b, e, [&] {
#pragma unroll
            for (int k = 0; k < W; k++) fr[lane * W + k] = f.w[k];
        });
        if (total == 0) continue;                                            // (uniform: no list of this group takes part)
        walk.for_each_arc(lane, total, [&](int l, uint64_t at) {
            const int64_t y = succ[at];
            if (y < 0 || y >= n) { oob = true; return; }
            const Words<W> s = *(const Words<W>*)(seen + y * W);
#pragma unroll
            for (int k = 0; k < W; k++) {
                const uint64_t m = fr[l * W + k] & ~s.w[k];
                if (m && (m & ~next[y * W + k])) (void)__hip_atomic_fetch_or(next + y * W + k, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a stale next: a needless atomic)
            }
        });
        walk.end();
    }
    if (oob) atomicOr(ctl + kCtlBad, 1ull);
}

// the sources of a pass: source s0 + j owns bit j; acc / reach / cnt of the pass
template <int W> __global__ void geo_seed_kernel(uint64_t* seen, uint64_t* frontier, int64_t s0, int count, double* acc, unsigned long long* reach, unsigned long long* cnt) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= 64 * W) return;
    acc[j] = 0.0; reach[j] = 1; cnt[j] = 0;
    if (j < count) {                                                         // (sources are distinct nodes: no two threads share a word)
        const int64_t at = (s0 + j) * W + (j >> 6);
        seen[at] = 1ull << (j & 63); frontier[at] = 1ull << (j & 63);
    }
}

// The end of a level, per node and word: new = next & ~seen; seen |= new; frontier = new; next = 0.  A wavefront takes 64 consecutive nodes,
// every lane the W words of one; for word k and bit b the nodes that gained the bit are popcount(ballot), a wavefront-uniform number that
// lane b adds to its running sum for word k.  One integer atomic per lane, word and wavefront at the end.
template <int W>
__global__ void __launch_bounds__(256) geo_advance_kernel(uint64_t* seen, uint64_t* frontier, uint64_t* next, int64_t n, unsigned long long* cnt) {
    const unsigned lane = threadIdx.x & 63;
    unsigned long long sum[W];
#pragma unroll
    for (int k = 0; k < W; k++) sum[k] = 0;
    for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); x0 < n; x0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform per wavefront: the ballots)
        const int64_t x = x0 + lane;
        Words<W> nw = {}, nx = {};
        if (x < n) {
            nx = *(const Words<W>*)(next + x * W);
            const Words<W> s = *(const Words<W>*)(seen + x * W);
            bool any = false, had = false;
            Words<W> s2;
#pragma unroll
            for (int k = 0; k < W; k++) { nw.w[k] = nx.w[k] & ~s.w[k]; s2.w[k] = s.w[k] | nw.w[k]; any |= nw.w[k] != 0; had |= nx.w[k] != 0; }
            if (any) *(Words<W>*)(seen + x * W) = s2;
            *(Words<W>*)(frontier + x * W) = nw;
            if (had) *(Words<W>*)(next + x * W) = Words<W>{};
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            const uint64_t v = nw.w[k];
            if (__ballot(v != 0) == 0) continue;                             // (uniform)
#pragma unroll 8
            for (unsigned b = 0; b < 64; b++) {
                const unsigned c = (unsigned)__builtin_popcountll(__ballot((v >> b) & 1));
                if (lane == b) sum[k] += c;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < W; k++) if (sum[k]) atomicAdd(cnt + k * 64 + lane, sum[k]);
}

// the level's counts into the accumulators: ONE workgroup of S = 64 W threads (at most 512), thread j owning bit j.  ctl[kCtlTotal] = the
// level's total (a plain store by one thread: nothing else writes it)
__global__ void __launch_bounds__(512) geo_accumulate_kernel(int S, double coeff, double* acc, unsigned long long* reach, unsigned long long* cnt, unsigned long long* ctl) {
    __shared__ unsigned long long part[8];
    const int j = (int)threadIdx.x;
    unsigned long long c = 0;
    if (j < S) {
        c = cnt[j];
        if (c) { acc[j] += coeff * (double)c; reach[j] += c; cnt[j] = 0; }
    }
    unsigned long long t = c;
    for (unsigned o = 32; o; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (unsigned i = 0; i < blockDim.x >> 6; i++) total += part[i];
        ctl[kCtlTotal] = total;
    }
}

// the end of a pass: either output may be null
__global__ void geo_finish_kernel(int count, double coeff0, const double* acc, const unsigned long long* reach, float* centrality, int64_t* reachable) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= count) return;
    if (centrality) centrality[j] = (float)(coeff0 + acc[j]);
    if (reachable) reachable[j] = (int64_t)reach[j];
}

}  // namespace

}  // namespace bvg

namespace {

using bvghost::Batch;

enum : int { kPasses, kSweeps, kDecodes, kWordsUsed, kDeepest, kSkippedLevels, kResident, kReserved };   // bvg_geometric's counters

struct Coefficients {
    int kind; double param; const double* table; uint64_t table_len;
    double operator()(uint64_t d) const {
        switch (kind) {
            case BVG_GEO_HARMONIC: return d == 0 ? 0.0 : 1.0 / (double)d;
            case BVG_GEO_POWER_LAW: return pow((double)d, param);
            case BVG_GEO_EXPONENTIAL: return pow(param, (double)d);
            default: return d < table_len ? table[d] : 0.0;
        }
    }
};

struct GeoOut { float* centrality; int64_t* reachable; uint64_t* hist; uint64_t hist_cap; uint64_t* hist_len; uint64_t* counters; };

template <int W> int geometric_t(bvg_graph* g, const Coefficients& coeff, int64_t from, int64_t to, const GeoOut& out, bool dev) {
    constexpr int S = 64 * W;
    const int64_t n = g->sh->p.nodes, count = to - from;
    const bool dbgt = dbg_on();
    Stopwatch sw;
    uint64_t counters[BVG_GEO_COUNTERS] = {};
    // seen | frontier | next in one allocation (zeroed together at the start of a pass), then the accumulators
    const size_t words = (size_t)n * W;
    DevArray<uint64_t> bits; DevArray<unsigned long long> accb; DevArray<uint8_t> ws; DevArray<float> oc; DevArray<int64_t> orr;
    if (bits.alloc(words * 3) || accb.alloc((size_t)S * 3 + kCtlWords)) return BVG_E_NOMEM;
    uint64_t* const seen = bits; uint64_t* const frontier = seen + words; uint64_t* const next = frontier + words;
    double* const acc = (double*)accb.get();
    unsigned long long* const reach = accb + S; unsigned long long* const cnt = reach + S; unsigned long long* const ctl = cnt + S;
    float* d_c = out.centrality; int64_t* d_r = out.reachable;
    if (!dev) {
        if (out.centrality) { if (oc.alloc((size_t)count)) return BVG_E_NOMEM; d_c = oc; }
        if (out.reachable) { if (orr.alloc((size_t)count)) return BVG_E_NOMEM; d_r = orr; }
    }
    uint64_t per = 0;                                                       // (of what is free once the per-node arrays are there)
    int rc = arc_budget(n, kMaxBatchArcs, "BVG_GEO_BATCH_ARCS", &per); if (rc) return rc;
    bvghost::SweepPlan sp;
    rc = sp.build(g, per); if (rc) return rc;
    if (!sp.batches.empty()) { if (ws.alloc(sp.bytes)) return BVG_E_NOMEM; sp.bind(ws.get()); }
    counters[kWordsUsed] = W; counters[kResident] = sp.single() ? 1 : 0;
    HIPCHK(hipMemsetAsync(ctl, 0, kCtlWords * 8, g->stream));
    std::vector<uint64_t> hist(1, 0);
    const double coeff0 = coeff(0);
    for (int64_t s0 = from; s0 < to; s0 += S) {
        const int in_pass = (int)std::min<int64_t>(S, to - s0);
        counters[kPasses]++;
        hist[0] += (uint64_t)in_pass;
        HIPCHK(hipMemsetAsync(bits, 0, words * 3 * 8, g->stream));
        hipLaunchKernelGGL((geo_seed_kernel<W>), dim3((S + 255) / 256), dim3(256), 0, g->stream, seen, frontier, s0, in_pass, acc, reach, cnt);
        for (uint64_t d = 1;; d++) {
            for (const Batch& b : sp.batches) {
                rc = sp.load(g, b, &counters[kDecodes]); if (rc) return rc;
                const int64_t nb = b.hi - b.lo;
                hipLaunchKernelGGL((geo_mark_kernel<W>), dim3(grid(nb, 256)), dim3(256), 0, g->stream, (const uint64_t*)sp.cum(), b.lo, nb, (const int64_t*)sp.succ(), n,
                                   (const uint64_t*)seen, (const uint64_t*)frontier, next, ctl);
                HIPCHK(hipGetLastError());
            }
            counters[kSweeps]++;
            hipLaunchKernelGGL((geo_advance_kernel<W>), dim3(grid(n, 256)), dim3(256), 0, g->stream, seen, frontier, next, n, cnt);
            hipLaunchKernelGGL(geo_accumulate_kernel, dim3(1), dim3(S), 0, g->stream, S, coeff(d), acc, reach, cnt, ctl);
            HIPCHK(hipGetLastError());
            unsigned long long h[kCtlWords];
            HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, g->stream));
            HIPCHK(hipStreamSynchronize(g->stream));
            if (h[kCtlBad]) return BVG_E_EOF;                                // a successor outside [0, n) was met
            if (!h[kCtlTotal]) break;
            if (hist.size() <= d) hist.resize(d + 1, 0);
            hist[d] += h[kCtlTotal];
            counters[kDeepest] = std::max<uint64_t>(counters[kDeepest], d);
        }
        if (d_c || d_r)
            hipLaunchKernelGGL(geo_finish_kernel, dim3((in_pass + 255) / 256), dim3(256), 0, g->stream, in_pass, coeff0, (const double*)acc, (const unsigned long long*)reach,
                               d_c ? d_c + (s0 - from) : nullptr, d_r ? d_r + (s0 - from) : nullptr);
    }
    HIPCHK(hipGetLastError());
    if (!dev) {
        if (out.centrality) HIPCHK(hipMemcpyAsync(out.centrality, d_c, (size_t)count * 4, hipMemcpyDeviceToHost, g->stream));
        if (out.reachable) HIPCHK(hipMemcpyAsync(out.reachable, d_r, (size_t)count * 8, hipMemcpyDeviceToHost, g->stream));
    }
    HIPCHK(hipStreamSynchronize(g->stream));
    if (out.counters) memcpy(out.counters, counters, sizeof counters);
    if (dbgt) fprintf(stderr, "[bvg] geometric: %lld sources, %d words per node, %zu batches of <= %llu arcs (%llu arcs), %llu passes, %llu sweeps, %llu decodes, deepest %llu: %.1f ms\n",
                      (long long)count, W, sp.batches.size(), (unsigned long long)per, (unsigned long long)sp.arcs, (unsigned long long)counters[kPasses],
                      (unsigned long long)counters[kSweeps], (unsigned long long)counters[kDecodes], (unsigned long long)counters[kDeepest], sw.lap());
    if (out.hist) {
        *out.hist_len = hist.size();
        memcpy(out.hist, hist.data(), (size_t)std::min<uint64_t>(hist.size(), out.hist_cap) * 8);
        if (out.hist_cap < hist.size()) return BVG_E_CAPACITY;
    } else if (out.hist_len) *out.hist_len = hist.size();
    return 0;
}

// the largest of 1, 2, 4, 8 words per node that the sources can fill and whose three arrays take at most half of the free memory
int words_per_node(int64_t n, int64_t count, int* w_out) {
    if (const char* k = knob("BVG_GEO_WORDS")) { const int v = atoi(k); if (v == 1 || v == 2 || v == 4 || v == 8) { *w_out = v; return 0; } }
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    int w = 8;
    while (w > 1 && ((int64_t)w > (count + 63) / 64 || (uint64_t)n * 24 * (uint64_t)w > fr / 2)) w >>= 1;
    *w_out = w;
    return 0;
}

int geometric_impl(bvg_graph* g, int kind, double param, const double* table, uint64_t table_len, int64_t from, int64_t to, float* centrality, int64_t* reachable,
                   uint64_t* hist, uint64_t hist_cap, uint64_t* hist_len, uint64_t* counters, bool dev) {
    if (!g) return BVG_E_ARG;
    if (kind != BVG_GEO_HARMONIC && kind != BVG_GEO_POWER_LAW && kind != BVG_GEO_EXPONENTIAL && kind != BVG_GEO_TABLE) return BVG_E_ARG;
    if (kind == BVG_GEO_TABLE && (!table || !table_len)) return BVG_E_ARG;
    if (hist && !hist_len) return BVG_E_ARG;
    Shared* sh = g->sh;
    if (from < 0 || from > to || to > sh->p.nodes) return BVG_E_ARG;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    if (counters) memset(counters, 0, BVG_GEO_COUNTERS * sizeof(uint64_t));
    if (hist_len) *hist_len = 0;
    if (from == to) return 0;
    HIPCHK(hipSetDevice(sh->device));
    index_first(g);
    int w = 1;
    int rc = words_per_node(sh->p.nodes, to - from, &w); if (rc) return rc;
    const Coefficients coeff{kind, param, table, table_len};
    const GeoOut out{centrality, reachable, hist, hist_cap, hist_len, counters};
    switch (w) {
        case 8: return geometric_t<8>(g, coeff, from, to, out, dev);
        case 4: return geometric_t<4>(g, coeff, from, to, out, dev);
        case 2: return geometric_t<2>(g, coeff, from, to, out, dev);
        default: return geometric_t<1>(g, coeff, from, to, out, dev);
    }
}

}  // namespace

int bvg_geometric(bvg_graph* g, int kind, double param, const double* table, uint64_t table_len, int64_t from, int64_t to, float* centrality, int64_t* reachable,
                  uint64_t* hist, uint64_t hist_cap, uint64_t* hist_len, uint64_t* counters) {
    return guarded([&] { return geometric_impl(g, kind, param, table, table_len, from, to, centrality, reachable, hist, hist_cap, hist_len, counters, false); });
}
int bvg_geometric_dev(bvg_graph* g, int kind, double param, const double* table, uint64_t table_len, int64_t from, int64_t to, void* d_centrality, void* d_reachable,
                      uint64_t* hist, uint64_t hist_cap, uint64_t* hist_len, uint64_t* counters) {
    return guarded([&] { return geometric_impl(g, kind, param, table, table_len, from, to, (float*)d_centrality, (int64_t*)d_reachable, hist, hist_cap, hist_len, counters, true); });
}
