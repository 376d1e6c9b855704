// bvg_arcwalk.h — how one wavefront walks the arcs of 64 consecutive lists of a decoded batch: the device half of the shared sweep
// (bvg_plan.hip holds the host half, SweepPlan).  Device-only; included by the kernels that consume a batch arc by arc: cc_hook_kernel
// (bvg_components.hip), bfs_mark_kernel (bvg_bfs.hip), scc_sweep_kernel (bvg_scc.hip), geo_mark_kernel (bvg_geometric.hip) and
// stats_sweep_kernel (bvg_stats.hip).
//
// Lane i of the wavefront knows the range [b, e) of list x0 + i in succ[] and whether that list takes part (`act`: it has arcs, and
// whatever the kernel asks of its source).  The lengths of the lists that take part are prefix-summed across the wavefront: they are
// laid end to end as "virtual" arcs 0 .. total - 1, and the 64 lanes walk those in chunks of 64, so a long list is spread over all lanes
// and an absent one costs nothing.  Virtual arc t belongs to the first list l whose inclusive prefix sum vend[l] is > t, found by binary
// search in LDS, and is succ[base[l] + t].  A kernel declares `__shared__ ArcWalk walk_s[4]` (one per wavefront of the workgroup) next to
// its own per-list payload and, per group of 64 lists: begin(), `continue` when it returns 0, one of the two walks, end().
//
// What the kernels rely on:
//   * base[l] = b - (inc - len) is taken mod 2^64: the lists before l may hold more virtual arcs than b real ones, and base[l] + t wraps
//     back to the real index.  Only a list that takes part has a base that is ever used.
//   * the search never looks past lane 63: vend[63] == total > t for every arc walked, so r starts at 63 and vend[] needs no sentinel.
//     Lists that do not take part have the prefix sum of their predecessor and are never an owner.
//   * total is uniform, and on total == 0 begin() returns before any LDS write or barrier: the caller `continue`s with LDS untouched.
//   * one barrier between the LDS writes (vend, base, the caller's payload) and the walk, one after it: the next group's writes come
//     after every lane's reads.  A wavefront's LDS operations complete in order, so these are wave barriers, not workgroup ones: the four
//     wavefronts of a workgroup share nothing here.
//   * the functors are inlined lambdas that capture the kernel's locals by reference.  What one of them stores to in sibling branches must be
//     ONE local (scc_sweep_kernel's `met` word, not two bools): the compiler sinks two such stores into one store through a selected
//     address, and then neither local is promoted to a register (8 bytes of scratch per lane, seen in the resource usage remarks).
#pragma once
#include <hip/hip_runtime.h>

namespace bvg {

// all ones: "no node" in the per-node arrays of the analytics (never a node: the 32-bit kernels stop at 2^32 - 256 nodes)
template <typename T> __device__ __host__ __forceinline__ constexpr T none() { return (T)~(T)0; }

struct ArcWalk {
    uint64_t vend[64];     // inclusive prefix sums of the lengths of the lists that take part: the ends in virtual arc indices
    uint64_t base[64];     // real index of virtual arc t of list l = base[l] + t (mod 2^64)

    // Sets up the walk; returns the number of arcs to walk (uniform).  `payload` writes the caller's own per-list LDS entries of this lane:
    // it runs only when there is something to walk, before the one barrier that orders all these writes before the walk's reads.
    template <typename P> __device__ __forceinline__ uint64_t begin(unsigned lane, bool act, uint64_t b, uint64_t e, P&& payload) {
        const uint64_t len = act ? e - b : 0;
        uint64_t inc = len;
        for (unsigned o = 1; o < 64; o <<= 1) { const uint64_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        const uint64_t total = __shfl(inc, 63, 64);
        if (total == 0) return 0;
        vend[lane] = inc; base[lane] = b - (inc - len);
        payload();
        __builtin_amdgcn_wave_barrier();
        return total;
    }

    // the list that virtual arc t belongs to; for t >= total: 63
    __device__ __forceinline__ int owner(uint64_t t) const {
        int l = 0, r = 63;
        while (l < r) { const int m = (l + r) >> 1; if (vend[m] <= t) l = m + 1; else r = m; }
        return l;
    }

    // f(l, at) for every arc, by the lane that holds it: the arc is succ[at] and belongs to list l of the group.  Lanes leave the loop when
    // they run out of arcs: nothing in f may need the whole wavefront
    template <typename F> __device__ __forceinline__ void for_each_arc(unsigned lane, uint64_t total, F&& f) const {
        for (uint64_t t = lane; t < total; t += 64) { const int l = owner(t); f(l, base[l] + t); }
    }

    // f(has, l, at) for every chunk of 64 arcs, by all 64 lanes (a uniform trip count: f may use ballots and shuffles).  Without `has` the
    // lane holds no arc in this chunk and l and at mean nothing
    template <typename F> __device__ __forceinline__ void for_each_chunk(unsigned lane, uint64_t total, F&& f) const {
        for (uint64_t t0 = 0; t0 < total; t0 += 64) {
            const uint64_t t = t0 + lane;
            const int l = owner(t);
            f(t < total, l, base[l] + t);
        }
    }

    __device__ __forceinline__ void end() const { __builtin_amdgcn_wave_barrier(); }   // (the next group's LDS writes after every lane's reads)
};

}  // namespace bvg
