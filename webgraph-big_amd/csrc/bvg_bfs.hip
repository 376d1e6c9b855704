// bvg_bfs.hip — breadth-first visits on the device (algo/ParallelBreadthFirstVisit.java).
//
// A visit object keeps what the reference's class keeps (ParallelBreadthFirstVisit.java:79-148) -- a marker per node (-1 = not enqueued yet), the
// round counter, the queue of the last visit and its cut points -- in HBM between visits, plus dist[] (the level of every node of the last visit).
// A visit is level-synchronous and the frontier never leaves HBM; per level a few words come back to the host (the arcs of the frontier, the size
// of the next one, an error flag).
//
//   expand     the successor lists of level d, by one of two routes chosen per level:
//                frontier  the body of bvg_successors_batch with the requests read from the queue (batch_degrees / batch_halos / batch_decode,
//                          bvg_api.hip), in pieces of at most the arc budget;
//                sweep     the whole graph decoded in arc-bounded node ranges (SweepPlan, bvg_plan.hip), of which the
//                          mark kernel takes the lists whose source has dist == d.  Random access to a large share of the graph costs more than
//                          decoding all of it in order.
//   mark       one wavefront per 64 lists: the lengths of the lists to expand are prefix-summed across the wavefront (LDS), then the lanes walk
//              those arcs in chunks of 64 -- the owner of arc t is found by binary search over the list ends (bvg_arcwalk.h).  Per arc: bounds
//              check, a plain load of marker[y], and only for an unmarked y an atomic.  The lane that wins y sets dist[y] = d + 1 and appends y to
//              a short list (one atomic per wavefront and chunk).
//   next       the next level in increasing id, without a sort of the graph's size: when the winners fit the short list it is radix-sorted into the
//              queue; otherwise the node range is compacted (rocPRIM select over a counting iterator, predicate dist[x] == d + 1).  Both give the
//              same queue; the first costs O(level), so a path graph does not pay O(n) per level.
//   visit_all  the search for the next node to visit is a device pass over a chunk of nodes: the first unmarked node that needs an expansion is
//              found with a minimum, and every unmarked node before it (no successors, or a lone self-loop) is marked and numbered in the same pass
//              (prefix sum of the unmarked flags), so n isolated nodes cost n / chunk round trips, not n.
//
// Determinism.  The queue holds each level in increasing id (above).  Parent mode (BVG_BFS_PARENT) must end with the SMALLEST parent, and a CAS keeps
// the first: so the parents of a level are collected with an atomic minimum on a candidate array (cand[], all ones between levels) and moved to
// marker[] by a kernel over the new level, which also resets its candidates -- O(level) again.  CAS-then-min on marker[] itself was not taken: it
// would have to tell a node marked in THIS level (parent may still shrink) from one marked before (final), which needs a second array anyway.
//
// Concurrency.  A CU's vector L1 is not refreshed by another CU's stores, so a plain load may return what the location held when the kernel began
// (L1 is invalidated between kernels).  Round mode: marker[y] goes from -1 to the round once per visit and never back inside a kernel, so a stale
// read can only be a -1 for a node marked meanwhile: the CAS (agent scope, performed at L2) then fails -- a wasted atomic, never a second winner.
// Parent mode: marker[] is read-only inside the mark kernel (exact); cand[y] only decreases, so a stale value is >= the current one: skipping
// when the stale cand[y] <= u is right (the current one is <= u too), not skipping costs a wasted atomic minimum.  dist[y] is stored by the winner
// only and read by later kernels only (the sweep route reads dist[source] == d, and a level's kernels store d + 1: no list of the next level is
// expanded early, whichever batch marked its source).
#include <cstdint>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "bvg_arcwalk.h"
#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

enum : int { kCtlBad = 0, kCtlCount = 1, kCtlFirst = 2, kCtlWords = 4 };   // control words (unsigned long long) the host reads back

template <typename T> __global__ void bfs_fill_kernel(T* marker, T* cand, int32_t* dist, int64_t n) {
    BVG_FOR(x, n) { marker[x] = none<T>(); if (cand) cand[x] = none<T>(); dist[x] = -1; }
}

__global__ void bfs_reset_dist_kernel(const int64_t* queue, uint64_t count, int32_t* dist) {
    BVG_FOR(i, count) dist[queue[i]] = -1;
}

template <typename T> __global__ void bfs_seed_kernel(int64_t start, T mark, T* marker, int32_t* dist, int64_t* queue) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { marker[start] = mark; dist[start] = 0; queue[0] = start; }
}

// One wavefront per 64 consecutive lists of the batch (four per workgroup): list i holds succ[cum[i] .. cum[i + 1]) and belongs to node
// nodes[i] (frontier route: every list is expanded) or lo + i (SWEEP: only when dist[lo + i] == d).  The arcs of the lists to expand are
// walked as bvg_arcwalk.h describes.  none<T>() (there too) is the marker's -1.
template <typename T, bool PARENT, bool SWEEP>
__global__ void __launch_bounds__(256) bfs_mark_kernel(const uint64_t* cum, const int64_t* nodes, int64_t lo, int64_t cnt, const int64_t* succ, int64_t n, T* marker, T* cand,
                                                       int32_t* dist, int32_t d, T round, unsigned long long* ctl, int64_t* small, uint64_t small_cap) {
    __shared__ ArcWalk walk_s[4];
    __shared__ T src_s[4][64];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ArcWalk& walk = walk_s[w]; T* src = src_s[w];
    bool oob = false;
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const int64_t i = x0 + lane;
        const bool valid = i < cnt;
        const uint64_t b = valid ? cum[i] : 0, e = valid ? cum[i + 1] : 0;
        const int64_t u = valid ? (SWEEP ? lo + i : nodes[i]) : 0;
        const bool act = valid && e > b && (!SWEEP || dist[u] == d);
        const uint64_t total = walk.begin(lane, act, b, e, [&] { src[lane] = (T)u; });
        if (total == 0) continue;                                            // (uniform: nothing of this group is in the level)
        walk.for_each_chunk(lane, total, [&](bool has, int l, uint64_t at) {  // (the uniform walk: ballots below)
            bool won = false; int64_t y = 0;
            if (has) {
                y = succ[at];
                if (y < 0 || y >= n) oob = true;                             // malformed stream: flagged, never used as an index
                else if (marker[y] == none<T>()) {
                    if (PARENT) {
                        const T p = src[l];
                        if (cand[y] > p) won = __hip_atomic_fetch_min(cand + y, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == none<T>();
                    } else {
                        T expect = none<T>();
                        won = __hip_atomic_compare_exchange_strong(marker + y, &expect, round, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (won) dist[y] = d + 1;
                }
            }
            const uint64_t wins = __ballot(won);
            if (wins) {                                                      // one atomic per wavefront and chunk
                const unsigned leader = (unsigned)__builtin_ctzll(wins);
                unsigned long long at_q = 0;
                if (lane == leader) at_q = atomicAdd(ctl + kCtlCount, (unsigned long long)__builtin_popcountll(wins));
                at_q = __shfl(at_q, (int)leader, 64) + (unsigned long long)__builtin_popcountll(wins & ((1ull << lane) - 1));
                if (won && at_q < small_cap) small[at_q] = y;
            }
        });
        walk.end();
    }
    if (oob) atomicOr(ctl + kCtlBad, 1ull);
}

// parent mode, over the new level: the smallest candidate becomes the parent, and the candidate is reset for the levels to come
template <typename T> __global__ void bfs_adopt_kernel(const int64_t* level, uint64_t count, T* marker, T* cand) {
    BVG_FOR(i, count) { const int64_t y = level[i]; marker[y] = cand[y]; cand[y] = none<T>(); }
}

template <typename T> __global__ void bfs_widen_kernel(const T* marker, int64_t n, int64_t* out) {
    BVG_FOR(x, n) { const T m = marker[x]; out[x] = m == none<T>() ? -1 : (int64_t)m; }
}

// ---- visit_all: what the nodes of a chunk [a, a + cnt) need
// need[i] = 1: node a + i has successors; nodes of outdegree 1 are listed (any order) for the check of their one successor
__global__ void bfs_classify_kernel(const int32_t* deg, int64_t a, int64_t cnt, uint8_t* need, int64_t* ones, unsigned long long* n_ones) {
    BVG_FOR(i, cnt) {
        const int32_t dg = deg[i];
        need[i] = dg > 0 ? 1 : 0;
        if (dg == 1) ones[atomicAdd(n_ones, 1ull)] = a + i;
    }
}
// a node whose only successor is itself needs no expansion (ParallelBreadthFirstVisit.java:309-317)
__global__ void bfs_loops_kernel(const int64_t* ones, int64_t count, const uint64_t* cum, const int64_t* succ, int64_t a, uint8_t* need) {
    BVG_FOR(i, count) if (cum[i + 1] == cum[i] + 1 && succ[cum[i]] == ones[i]) need[ones[i] - a] = 0;
}
// the first node of [from, to) that is unmarked and needs an expansion (*first: `to` when there is none).  Lanes hold increasing ids, so the
// lowest set lane of a wavefront is its minimum: one atomic per wavefront, and none once a smaller node is known (a stale *first is larger:
// a wasted atomic)
template <typename T> __global__ void __launch_bounds__(256) bfs_find_kernel(const T* marker, const uint8_t* need, int64_t a, int64_t from, int64_t to, unsigned long long* first) {
    for (int64_t x0 = from + (int64_t)blockIdx.x * blockDim.x; x0 < to; x0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform per workgroup)
        const int64_t x = x0 + threadIdx.x;
        const bool hit = x < to && need[x - a] && marker[x] == none<T>();
        const uint64_t hits = __ballot(hit);
        if (hits && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(hits) && (unsigned long long)x < *first) atomicMin(first, (unsigned long long)x);
    }
}
template <typename T> __global__ void bfs_flag_kernel(const T* marker, int64_t from, int64_t to, const unsigned long long* first, int32_t* flag) {
    const int64_t stop = (int64_t)*first < to ? (int64_t)*first : to;
    BVG_FOR(i, to - from) flag[i] = (from + i < stop && marker[from + i] == none<T>()) ? 1 : 0;
}
// the unmarked nodes before *first get their marker: each is a visit of its own, so round numbers go up by one per node
template <typename T, bool PARENT> __global__ void bfs_number_kernel(T* marker, int64_t from, int64_t to, const int32_t* flag, const uint64_t* rank, int64_t round) {
    BVG_FOR(i, to - from) if (flag[i]) marker[from + i] = PARENT ? (T)(from + i) : (T)(round + 1 + (int64_t)rank[i]);
}

struct InLevel {
    const int32_t* dist; int32_t level;
    __device__ bool operator()(const int64_t& x) const { return dist[x] == level; }
};

}  // namespace

}  // namespace bvg

using bvghost::Batch;
using bvghost::BatchBufs;
using bvghost::DeepRequest;

namespace {

constexpr uint64_t kMaxBudgetArcs = 1ull << 30;    // 8 GiB of successors per batch.  Below kMaxBatchArcs: the object keeps two such buffers between visits (succ for the
                                                   // frontier route, sw_ws for the sweep), each with grow()'s quarter of slack
constexpr uint64_t kSmallCap = 1ull << 16;         // winners up to this many are sorted; more: the node range is compacted
constexpr int64_t kPiece = 1ll << 24;              // requests of one frontier piece (its node-side arrays: ~100 bytes each)
constexpr int64_t kChunk = 1ll << 20;              // nodes of one visit_all search chunk
constexpr uint64_t kSwitchDen = 16;                // sweep when the frontier's outdegrees sum to >= arcs / 16 (UNMEASURED default: DESIGN.md 7c)

// a workspace of the object grown on demand, with a quarter of slack; contents not kept
int grow(DevWorkspace& w, size_t want) { return want <= w.bytes() ? 0 : w.reserve(want + want / 4); }

}  // namespace

struct bvg_bfs {
    bvg_graph* g = nullptr;                        // a bvg_copy() flyweight: own stream and workspaces
    bool parent = false, wide = false;
    int64_t n = 0;
    DevArray<uint8_t> marker, cand;                // uint32 per node, uint64 when `wide`
    DevArray<int32_t> dist; DevArray<int64_t> queue, small; DevArray<unsigned long long> ctl;
    std::vector<uint64_t> cuts;
    int64_t round = -1; uint64_t qsize = 0;
    // knobs
    int force_route = 0;                           // 1 frontier, 2 sweep
    uint64_t per = 0, small_cap = kSmallCap, switch_den = kSwitchDen;
    // the graph in arc-bounded node ranges (sweep route), planned at the first need
    bool planned = false; bvghost::SweepPlan sweep; uint64_t arcs = 0; bool arcs_known = false;
    DevWorkspace fr_bufs, succ, sw_ws, prim, chunk_ws, wide_out;
    // visit_all's chunk
    int64_t ch_a = -1, ch_b = -1;
    uint64_t counters[BVG_BFS_COUNTERS] = {};
    ~bvg_bfs() { if (g) { (void)hipSetDevice(g->sh->device); bvg_close(g); } }
};

namespace {

enum : int { kFrontierLevels, kSweepLevels, kDeep, kFrontierBatches, kSweepBatches, kSortedLevels, kCompactedLevels, kFirstLevelRoute };

template <typename T> int clear_t(bvg_bfs* v) {
    bvg_graph* g = v->g;
    if (v->n) hipLaunchKernelGGL((bfs_fill_kernel<T>), dim3(grid(v->n, 256)), dim3(256), 0, g->stream, (T*)v->marker.get(), (T*)v->cand.get(), v->dist.get(), v->n);
    v->round = -1; v->qsize = 0; v->cuts.clear();
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

// the arc budget, at the first visit and before any plan: the frontier route needs it without a sweep (the knob was read when the object was created)
int budget(bvg_bfs* v) { return v->per ? 0 : arc_budget(v->n, kMaxBudgetArcs, nullptr, &v->per); }

int ensure_plan(bvg_bfs* v) {
    if (v->planned) return 0;
    int rc = budget(v); if (rc) return rc;
    index_first(v->g);
    rc = v->sweep.build(v->g, v->per); if (rc) return rc;
    v->arcs = v->sweep.arcs; v->arcs_known = true; v->planned = true;
    return 0;
}

template <typename T> void launch_mark(bvg_bfs* v, bool sweep, const uint64_t* cum, const int64_t* nodes, int64_t lo, int64_t cnt, const int64_t* succ, int32_t d) {
    bvg_graph* g = v->g;
    const dim3 gr(grid(cnt, 256)), bl(256);
    T* const marker = (T*)v->marker.get(); T* const cand = (T*)v->cand.get(); int32_t* const dist = v->dist.get();
    unsigned long long* const ctl = v->ctl.get(); int64_t* const small = v->small.get();
    const T round = (T)v->round;
#define BFS_MARK(P, S) hipLaunchKernelGGL((bfs_mark_kernel<T, P, S>), gr, bl, 0, g->stream, cum, nodes, lo, cnt, succ, v->n, marker, cand, dist, d, round, ctl, small, v->small_cap)
    if (v->parent) { if (sweep) BFS_MARK(true, true); else BFS_MARK(true, false); }
    else { if (sweep) BFS_MARK(false, true); else BFS_MARK(false, false); }
#undef BFS_MARK
}

// the lists of `count` requests (d_nodes, on the device) decoded into v->succ, list i at bufs.cum[i]; the degrees are in `b` already
int decode_requests(bvg_bfs* v, const BatchBufs& b, const int64_t* d_nodes, int64_t count, uint64_t total) {
    bvg_graph* g = v->g;
    std::vector<DeepRequest> deep;
    int rc = batch_halos(g, b, d_nodes, count, deep); if (rc) return rc;
    rc = grow(v->succ, (size_t)(total ? total : 1) * 8); if (rc) return rc;
    int64_t* const d_succ = (int64_t*)v->succ.get();
    rc = batch_decode(g, b, count, d_succ); if (rc) return rc;
    for (const DeepRequest& q : deep) {                                     // through the block plan, one by one (few)
        int64_t x = 0; uint64_t got = 0;
        HIPCHK(hipMemcpyAsync(&x, d_nodes + q.index, 8, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (!q.arcs) continue;
        rc = decode_range_impl(g, x, x + 1, nullptr, d_succ + q.at, q.arcs, &got, true); if (rc) return rc;
        if (got != q.arcs) return BVG_E_STATE;
    }
    v->counters[kDeep] += deep.size();
    return 0;
}

// Frontier route over queue[lo, hi).  *switched: the level's arcs passed the switch point (auto mode), the caller sweeps instead -- what was
// marked so far stays (marking is idempotent: a node is won once).
template <typename T> int expand_frontier(bvg_bfs* v, uint64_t lo, uint64_t hi, int32_t d, bool autoroute, bool* switched) {
    bvg_graph* g = v->g;
    const int64_t* const q = v->queue.get();
    uint64_t level_arcs = 0;
    *switched = false;
    for (uint64_t p0 = lo; p0 < hi; p0 += (uint64_t)kPiece) {
        const int64_t cnt = (int64_t)std::min<uint64_t>(hi - p0, (uint64_t)kPiece);
        int rc = grow(v->fr_bufs, batch_bufs_bytes(cnt)); if (rc) return rc;
        BatchBufs b = batch_bufs_at(v->fr_bufs.at(0), cnt);
        uint64_t total = 0;
        rc = batch_degrees(g, b, q + p0, cnt, &total); if (rc) return rc;
        level_arcs += total;
        if (autoroute && v->arcs_known && level_arcs * v->switch_den >= v->arcs && level_arcs > 0) { *switched = true; return 0; }
        if (!total) continue;
        if (total <= v->per) {
            rc = decode_requests(v, b, q + p0, cnt, total); if (rc) return rc;
            launch_mark<T>(v, false, b.cum, q + p0, 0, cnt, (const int64_t*)v->succ.get(), d);
            v->counters[kFrontierBatches]++;
            continue;
        }
        std::vector<Batch> parts; uint64_t longest = 0;                      // more arcs than the budget: the piece in arc-bounded parts
        rc = cut_batches(g, b.cum, cnt, total, v->per, parts, &longest); if (rc) return rc;
        for (const Batch& pt : parts) {
            const int64_t c = pt.hi - pt.lo;
            b = batch_bufs_at(v->fr_bufs.at(0), c);
            rc = batch_degrees(g, b, q + p0 + pt.lo, c, &total); if (rc) return rc;
            if (!total) continue;
            rc = decode_requests(v, b, q + p0 + pt.lo, c, total); if (rc) return rc;
            launch_mark<T>(v, false, b.cum, q + p0 + pt.lo, 0, c, (const int64_t*)v->succ.get(), d);
            v->counters[kFrontierBatches]++;
        }
    }
    return 0;
}

template <typename T> int expand_sweep(bvg_bfs* v, int32_t d) {
    bvg_graph* g = v->g;
    int rc = ensure_plan(v); if (rc) return rc;
    bvghost::SweepPlan& sp = v->sweep;
    if (sp.batches.empty()) return 0;
    rc = grow(v->sw_ws, sp.bytes); if (rc) return rc;
    sp.bind(v->sw_ws.get());
    for (const Batch& b : sp.batches) {
        rc = sp.decode(g, b); if (rc) return rc;
        launch_mark<T>(v, true, sp.cum(), nullptr, b.lo, b.hi - b.lo, sp.succ(), d);
        HIPCHK(hipGetLastError());
        v->counters[kSweepBatches]++;
    }
    return 0;
}

// the winners of level d + 1 into queue[at, at + added), in increasing id
template <typename T> int next_level(bvg_bfs* v, uint64_t at, uint64_t added, int32_t d) {
    bvg_graph* g = v->g;
    int64_t* const out = v->queue.get() + at;
    if (added <= v->small_cap) {
        if (added == 1) HIPCHK(hipMemcpyAsync(out, v->small.get(), 8, hipMemcpyDeviceToDevice, g->stream));
        else {
            const unsigned bits = 64u - (unsigned)__builtin_clzll((unsigned long long)(v->n > 1 ? v->n - 1 : 1));
            size_t tb = 0;
            if (rocprim::radix_sort_keys(nullptr, tb, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)added, 0u, bits, g->stream) != hipSuccess) return BVG_E_HIP;
            int rc = grow(v->prim, tb ? tb : 1); if (rc) return rc;
            if (rocprim::radix_sort_keys(v->prim.get(), tb, (const uint64_t*)v->small.get(), (uint64_t*)out, (size_t)added, 0u, bits, g->stream) != hipSuccess) return BVG_E_HIP;
        }
        v->counters[kSortedLevels]++;
    } else {
        const InLevel pred{v->dist.get(), d + 1};
        unsigned long long* const d_sel = v->ctl.get() + kCtlFirst;   // (what a call selected)
        const bool ranges = v->n > bvghost::kMaxBatchNodes;                  // node ranges below 2^32 elements per call; their outputs follow one another
        uint64_t done = 0;
        for (int64_t a = 0; a < v->n; a += bvghost::kMaxBatchNodes) {
            const int64_t c = std::min(v->n - a, bvghost::kMaxBatchNodes);
            rocprim::counting_iterator<int64_t> in(a);
            size_t tb = 0;
            if (rocprim::select(nullptr, tb, in, out + done, d_sel, (size_t)c, pred, g->stream) != hipSuccess) return BVG_E_HIP;
            const int rc = grow(v->prim, tb ? tb : 1); if (rc) return rc;
            if (rocprim::select(v->prim.get(), tb, in, out + done, d_sel, (size_t)c, pred, g->stream) != hipSuccess) return BVG_E_HIP;
            if (ranges) {
                unsigned long long sel = 0;
                HIPCHK(hipMemcpyAsync(&sel, d_sel, 8, hipMemcpyDeviceToHost, g->stream));
                HIPCHK(hipStreamSynchronize(g->stream));
                done += sel;
            }
        }
        v->counters[kCompactedLevels]++;
    }
    if (v->parent) hipLaunchKernelGGL((bfs_adopt_kernel<T>), dim3(grid((int64_t)added, 256)), dim3(256), 0, g->stream, (const int64_t*)out, added, (T*)v->marker.get(), (T*)v->cand.get());
    HIPCHK(hipGetLastError());
    return 0;
}

// one visit from `start` (unmarked), v->round being its round already
template <typename T> int visit_t(bvg_bfs* v, int64_t start) {
    bvg_graph* g = v->g;
    unsigned long long* const ctl = v->ctl.get();
    if (v->qsize) hipLaunchKernelGGL(bfs_reset_dist_kernel, dim3(grid((int64_t)v->qsize, 256)), dim3(256), 0, g->stream, v->queue.get(), v->qsize, v->dist.get());
    hipLaunchKernelGGL((bfs_seed_kernel<T>), dim3(1), dim3(64), 0, g->stream, start, v->parent ? (T)start : (T)v->round, (T*)v->marker.get(), v->dist.get(), v->queue.get());
    v->cuts.assign({0, 1}); v->qsize = 1;
    int rc = budget(v); if (rc) return rc;
    if (!v->arcs_known && v->g->sh->p.arcs >= 0) { v->arcs = (uint64_t)v->g->sh->p.arcs; v->arcs_known = true; }
    for (int32_t d = 0;; d++) {
        if (d == INT32_MAX) return BVG_E_UNSUPPORTED;
        const uint64_t lo = v->cuts[(size_t)d], hi = v->cuts[(size_t)d + 1];
        HIPCHK(hipMemsetAsync(ctl, 0, kCtlWords * 8, g->stream));
        bool sweep = v->force_route == 2;
        if (!sweep && !v->force_route) {
            if (!v->arcs_known) { rc = ensure_plan(v); if (rc) return rc; }
            sweep = (hi - lo) * 4 >= (uint64_t)v->n && v->n >= 4096;          // a quarter of the nodes: no need to look at their outdegrees
        }
        if (!sweep) {
            bool switched = false;
            rc = expand_frontier<T>(v, lo, hi, d, v->force_route == 0, &switched); if (rc) return rc;
            sweep = switched;
        }
        if (sweep) { rc = expand_sweep<T>(v, d); if (rc) return rc; }
        v->counters[sweep ? kSweepLevels : kFrontierLevels]++;
        if (d == 0) v->counters[kFirstLevelRoute] = sweep ? 2 : 1;
        unsigned long long h[2] = {0, 0};
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (h[kCtlBad]) return BVG_E_EOF;                                    // a successor outside [0, n): malformed stream
        const uint64_t added = h[kCtlCount];
        if (!added) break;
        if (v->qsize + added > (uint64_t)v->n) return BVG_E_STATE;
        rc = next_level<T>(v, v->qsize, added, d); if (rc) return rc;
        v->qsize += added; v->cuts.push_back(v->qsize);
    }
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

// visit_all: need[] of the chunk [a, b)
template <typename T> int prepare_chunk(bvg_bfs* v, int64_t a, int64_t b, size_t o_need, size_t o_deg, size_t o_ones) {
    bvg_graph* g = v->g;
    char* const w = v->chunk_ws.at(0);
    const int64_t cnt = b - a;
    unsigned long long* const ctl = v->ctl.get();
    uint8_t* const need = (uint8_t*)(w + o_need); int64_t* const ones = (int64_t*)(w + o_ones);
    HIPCHK(hipMemsetAsync(ctl, 0, kCtlWords * 8, g->stream));
    outdegrees_of(g, a, b, (int32_t*)(w + o_deg));
    hipLaunchKernelGGL(bfs_classify_kernel, dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const int32_t*)(w + o_deg), a, cnt, need, ones, ctl + kCtlCount);
    unsigned long long n_ones = 0;
    HIPCHK(hipMemcpyAsync(&n_ones, ctl + kCtlCount, 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (n_ones) {
        int rc = grow(v->fr_bufs, batch_bufs_bytes((int64_t)n_ones)); if (rc) return rc;
        const BatchBufs bb = batch_bufs_at(v->fr_bufs.at(0), (int64_t)n_ones);
        uint64_t total = 0;
        rc = batch_degrees(g, bb, ones, (int64_t)n_ones, &total); if (rc) return rc;
        rc = decode_requests(v, bb, ones, (int64_t)n_ones, total); if (rc) return rc;
        hipLaunchKernelGGL(bfs_loops_kernel, dim3(grid((int64_t)n_ones, 256)), dim3(256), 0, g->stream, (const int64_t*)ones, (int64_t)n_ones, (const uint64_t*)bb.cum,
                           (const int64_t*)v->succ.get(), a, need);
        HIPCHK(hipGetLastError());
    }
    v->ch_a = a; v->ch_b = b;
    return 0;
}

template <typename T> int visit_all_t(bvg_bfs* v) {
    bvg_graph* g = v->g;
    int rc = clear_t<T>(v); if (rc) return rc;
    const int64_t n = v->n;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t C = (size_t)std::min(n, kChunk);
    const size_t o_need = 0, o_deg = o_need + al(C), o_ones = o_deg + al(C * 4), o_flag = o_ones + al(C * 8), o_rank = o_flag + al(C * 4), o_tmp = o_rank + al((C + 1) * 8);
    rc = grow(v->chunk_ws, o_tmp + al(scan_tmp_elems((int64_t)C) * 8)); if (rc) return rc;
    char* const w = v->chunk_ws.at(0);
    unsigned long long* const ctl = v->ctl.get();
    T* const marker = (T*)v->marker.get();
    v->ch_a = v->ch_b = -1;
    for (int64_t a = 0; a < n; a += kChunk) {
        const int64_t b = std::min(n, a + kChunk);
        rc = prepare_chunk<T>(v, a, b, o_need, o_deg, o_ones); if (rc) return rc;
        int64_t curr = a;
        while (curr < b) {
            const int64_t cnt = b - curr;
            const unsigned long long none_found = (unsigned long long)b;
            HIPCHK(hipMemcpyAsync(ctl + kCtlFirst, &none_found, 8, hipMemcpyHostToDevice, g->stream));
            hipLaunchKernelGGL((bfs_find_kernel<T>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const T*)marker, (const uint8_t*)(w + o_need), a, curr, b, ctl + kCtlFirst);
            hipLaunchKernelGGL((bfs_flag_kernel<T>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const T*)marker, curr, b, (const unsigned long long*)(ctl + kCtlFirst), (int32_t*)(w + o_flag));
            launch_exclusive_scan((const int32_t*)(w + o_flag), (uint64_t*)(w + o_rank), cnt, (uint64_t*)(w + o_tmp), g->stream);
            if (v->parent) hipLaunchKernelGGL((bfs_number_kernel<T, true>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, marker, curr, b, (const int32_t*)(w + o_flag), (const uint64_t*)(w + o_rank), v->round);
            else hipLaunchKernelGGL((bfs_number_kernel<T, false>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, marker, curr, b, (const int32_t*)(w + o_flag), (const uint64_t*)(w + o_rank), v->round);
            HIPCHK(hipGetLastError());
            unsigned long long first = 0, numbered = 0;
            HIPCHK(hipMemcpyAsync(&first, ctl + kCtlFirst, 8, hipMemcpyDeviceToHost, g->stream));
            HIPCHK(hipMemcpyAsync(&numbered, (uint64_t*)(w + o_rank) + cnt, 8, hipMemcpyDeviceToHost, g->stream));
            HIPCHK(hipStreamSynchronize(g->stream));
            v->round += (int64_t)numbered;
            if ((int64_t)first >= b) break;
            v->round++;
            rc = visit_t<T>(v, (int64_t)first); if (rc) return rc;
            curr = (int64_t)first + 1;
        }
    }
    return 0;
}

int clear_any(bvg_bfs* v) { return v->wide ? clear_t<uint64_t>(v) : clear_t<uint32_t>(v); }

uint64_t knob_u64(const char* name, uint64_t dflt) {
    if (const char* k = knob(name)) { const long long x = atoll(k); if (x >= 0) return (uint64_t)x; }
    return dflt;
}

int get_impl(bvg_bfs* v, int64_t* marker, int64_t* queue, uint64_t queue_cap, uint64_t* cutpoints, uint64_t cut_cap, int32_t* dist, bool dev) {
    bvg_graph* g = v->g;
    if ((queue && queue_cap < v->qsize) || (cutpoints && cut_cap < v->cuts.size())) return BVG_E_CAPACITY;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (marker && v->n) {
        int64_t* d_out = marker;
        if (!dev) { int rc = grow(v->wide_out, (size_t)v->n * 8); if (rc) return rc; d_out = (int64_t*)v->wide_out.get(); }
        if (v->wide) hipLaunchKernelGGL((bfs_widen_kernel<uint64_t>), dim3(grid(v->n, 256)), dim3(256), 0, g->stream, (const uint64_t*)v->marker.get(), v->n, d_out);
        else hipLaunchKernelGGL((bfs_widen_kernel<uint32_t>), dim3(grid(v->n, 256)), dim3(256), 0, g->stream, (const uint32_t*)v->marker.get(), v->n, d_out);
        HIPCHK(hipGetLastError());
        if (!dev) HIPCHK(hipMemcpyAsync(marker, d_out, (size_t)v->n * 8, hipMemcpyDeviceToHost, g->stream));
    }
    if (queue && v->qsize) HIPCHK(hipMemcpyAsync(queue, v->queue.get(), (size_t)v->qsize * 8, kind, g->stream));
    if (cutpoints && !v->cuts.empty()) HIPCHK(hipMemcpyAsync(cutpoints, v->cuts.data(), v->cuts.size() * 8, dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost, g->stream));
    if (dist && v->n) HIPCHK(hipMemcpyAsync(dist, v->dist.get(), (size_t)v->n * 4, kind, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return 0;
}

}  // namespace

extern "C" {

int bvg_bfs_create(bvg_graph* g, uint32_t flags, bvg_bfs** out) {
    if (!g || !out || (flags & ~(uint32_t)BVG_BFS_PARENT)) return BVG_E_ARG;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    *out = nullptr;
    return bvghost::guarded([&]() -> int {
        HIPCHK(hipSetDevice(g->sh->device));
        std::unique_ptr<bvg_bfs> v(new bvg_bfs);
        int rc = bvg_copy(g, &v->g); if (rc) { v->g = nullptr; return rc; }
        v->parent = (flags & BVG_BFS_PARENT) != 0;
        v->wide = g->sh->wide || g->tun.force_wide;
        v->n = g->sh->p.nodes;
        const size_t nn = (size_t)(v->n > 0 ? v->n : 1), tb = v->wide ? 8 : 4;
        v->small_cap = knob_u64("BVG_BFS_SMALL", kSmallCap);
        if (v->small_cap > kSmallCap) v->small_cap = kSmallCap;
        v->per = knob_u64("BVG_BFS_BATCH_ARCS", 0);
        v->switch_den = std::max<uint64_t>(1, knob_u64("BVG_BFS_SWITCH", kSwitchDen));
        if (const char* k = knob("BVG_BFS_ROUTE")) v->force_route = !strcmp(k, "frontier") ? 1 : !strcmp(k, "sweep") ? 2 : 0;
        if (v->marker.alloc(nn * tb) || v->dist.alloc(nn) || v->queue.alloc(nn) || v->ctl.alloc(32) || v->small.alloc((size_t)std::max<uint64_t>(v->small_cap, 1))) return BVG_E_NOMEM;
        if (v->parent && v->cand.alloc(nn * tb)) return BVG_E_NOMEM;
        rc = clear_any(v.get()); if (rc) return rc;
        *out = v.release();
        return 0;
    });
}

void bvg_bfs_close(bvg_bfs* v) { delete v; }

int bvg_bfs_clear(bvg_bfs* v) { return on_device(v, [&] { return clear_any(v); }); }

int bvg_bfs_visit(bvg_bfs* v, int64_t start, uint64_t* visited) {
    if (visited) *visited = 0;
    return on_device(v, [&]() -> int {
        if (start < 0 || start >= v->n) return BVG_E_ARG;
        uint64_t m = 0;                                                      // the start's marker: one element back to the host
        HIPCHK(hipMemcpyAsync(&m, (char*)v->marker.get() + (size_t)start * (v->wide ? 8 : 4), v->wide ? 8 : 4, hipMemcpyDeviceToHost, v->g->stream));
        HIPCHK(hipStreamSynchronize(v->g->stream));
        if (m != (v->wide ? ~0ull : 0xFFFFFFFFull)) return 0;                 // visited already: nothing changes (ParallelBreadthFirstVisit.java:223)
        v->round++;
        const int rc = v->wide ? visit_t<uint64_t>(v, start) : visit_t<uint32_t>(v, start);
        if (rc) { (void)clear_any(v); return rc; }
        if (visited) *visited = v->qsize;
        return 0;
    });
}

int bvg_bfs_visit_all(bvg_bfs* v) {
    return on_device(v, [&]() -> int {
        const int rc = v->wide ? visit_all_t<uint64_t>(v) : visit_all_t<uint32_t>(v);
        if (rc) (void)clear_any(v);
        return rc;
    });
}

int bvg_bfs_info(const bvg_bfs* v, int64_t* round, uint64_t* queue_size, uint64_t* n_cutpoints) {
    if (!v) return BVG_E_ARG;
    if (round) *round = v->round;
    if (queue_size) *queue_size = v->qsize;
    if (n_cutpoints) *n_cutpoints = v->cuts.size();
    return 0;
}

int bvg_bfs_get(bvg_bfs* v, int64_t* marker, int64_t* queue, uint64_t queue_cap, uint64_t* cutpoints, uint64_t cut_cap, int32_t* dist) {
    return on_device(v, [&] { return get_impl(v, marker, queue, queue_cap, cutpoints, cut_cap, dist, false); });
}
int bvg_bfs_get_dev(bvg_bfs* v, void* d_marker, void* d_queue, uint64_t queue_cap, void* d_cutpoints, uint64_t cut_cap, void* d_dist) {
    return on_device(v, [&] { return get_impl(v, (int64_t*)d_marker, (int64_t*)d_queue, queue_cap, (uint64_t*)d_cutpoints, cut_cap, (int32_t*)d_dist, true); });
}

int bvg_bfs_counters(const bvg_bfs* v, uint64_t* out) {
    if (!v || !out) return BVG_E_ARG;
    memcpy(out, v->counters, sizeof v->counters);
    return 0;
}

}  // extern "C"
