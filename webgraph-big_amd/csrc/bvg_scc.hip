// bvg_scc.hip — strongly connected components on the device (algo/StronglyConnectedComponents.java).
//
// The reference is a single-threaded iterative Tarjan visit that calls successors(x) at random and keeps three per-node stacks
// (StronglyConnectedComponents.java: Visit).  Here the same partition comes from sweeps of the compressed graph over forward arcs only
// (SweepPlan, bvg_plan.hip): no transpose, no CSR of the whole graph in HBM.  Per node: rep[] (the smallest node of the finished SCC, all ones
// while the node is live), colour[] (the class of a live node, all ones once it is retired) and one byte of flags.  An arc u -> v COUNTS when
// colour[u] == colour[v] and neither is all ones: both ends live and in the same class of whatever partition is known (SCCs never cross it).
//
//   trim      per counting arc with u != v: has-live-out on u, has-live-in on v.  A per-node kernel then retires every live node lacking
//             either flag as an SCC of its own (rep[x] = x).  Repeated until a sweep retires nothing.
//   fw / bw   fw[u] sets fw[v]; bw[v] sets bw[u]: backward reachability on FORWARD arcs, which is why no transpose is needed.
//   colour    colour[v] = max(colour[v], colour[u]) over arcs between live nodes (atomic maximum, issued only when a plain load shows
//             colour[v] smaller).  While it runs the colours are being rebuilt, so "counts" is "both live" there.
//
//   1  trim
//   2  one FW-BW step from a pivot (largest outdegree among the live nodes, smallest id on ties): fw and bw is one SCC -- on a web graph the
//      giant one.  The live rest gets the colours 1 + fw + 2 bw, the partition the next trim respects.
//   3  rounds of: trim; colour = id on the live nodes; colour to the fixpoint (colour[v] = the largest live node that reaches v); the roots
//      (colour[r] == r) become backward seeds; bw within equal colour to the fixpoint; every bw node is retired, its colour naming its SCC
//      (the nodes of colour r that reach r are exactly those that r reaches and that reach r).  The colours left behind are the next partition.
//   4  until no node is live.  Every round retires the SCC of the largest live node at least.
//   A retirement is two per-node kernels: an atomic minimum of the members' ids on rep[key] (key: the pivot or the colour; that node is a
//   member and still all ones), then rep[x] = rep[key]: rep[x] ends as the smallest node of x's SCC, so parent[x] = rep[x] is what the
//   numbering of bvg_components takes (number_components, bvg_host.h): component c is the one whose smallest node is the c-th smallest among
//   the components' smallest nodes.  THIS IS NOT THE REFERENCE'S NUMBERING, which is Tarjan's emission order (a component is numbered when
//   its root is popped); the partition, the count, the sizes after sortBySize (up to the order of ties: here by smallest node) and the buckets are.
//   Buckets (computeBuckets): a node is in a bucket exactly when its SCC has at least one arc (a self-loop counts) and no arc leaving it --
//   one last sweep sets "has an arc" / "has a leaving arc" on the flags byte of rep[u].
//
// Sweeps.  A plan of one batch is decoded once and stays resident for the whole call: a sweep is then one kernel launch.  With several
// batches every sweep decodes every batch again; the kernel is rerun on the resident batch until it changes nothing there, at most
// kMaxReruns times (a stated default, NOT measured), so that what propagates inside a batch does not cost whole sweeps.
//
// Fixpoint rule.  A propagation (fw, bw, colour) has converged only when a COMPLETE sweep, from the first batch to the last, performed no
// write.  A CU's vector L1 is not refreshed by another CU's stores, so a plain load inside a kernel may return what the location held when
// the kernel began (L1 is invalidated between kernels).  Every update is monotone -- a flag bit is only set, a colour only grows -- so a
// stale value is an older one: it can cause a needless atomic (counted as a write: one more sweep) or hide an update made by another
// wavefront of the SAME launch -- which set the change flag, so another sweep follows.  In a sweep without any write nothing changed, every
// load returned the final value, and every arc was seen satisfied.  The fixpoints are unique (reachability; the largest reaching node)
// and the partition into SCCs is unique, so neither lane order, nor the order of the atomics, nor the pivot, nor the batch size can reach
// the result; rep[] is a minimum over a fixed set.  Flag bits of one node are set with an atomic OR on the aligned 32-bit word that holds the
// byte (two lanes may set different bits of one byte); per-node kernels, in which only thread x touches byte x, store the byte.
#include <cstdint>
#include <cstring>

#include "bvg_arcwalk.h"
#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

// none<T>() (bvg_arcwalk.h): rep: live; colour: retired
enum : int { kTrim, kFw, kBw, kColour, kBucket };                                 // modes of the sweep kernel
enum : unsigned { fIn = 1, fOut = 2, fFw = 4, fBw = 8, fArc = 1, fLeave = 2 };    // flag bits (the bucket sweep reuses the trim bits, on representatives)
enum : unsigned { mOob = 1, mWrote = 2 };                                         // what a lane of the sweep kernel met: a target outside [0, n); a write that counts for the fixpoint
enum : int { kCtlBad, kCtlChanged, kCtlCount, kCtlRoots, kCtlMaxDeg, kCtlPivot, kCtlWords = 8 };   // control words (unsigned long long) the host reads back

__device__ __forceinline__ void set_flag(uint8_t* flags, int64_t x, unsigned bits) {
    __hip_atomic_fetch_or((unsigned*)flags + (x >> 2), bits << (8 * (unsigned)(x & 3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wavefront per 64 consecutive lists of the batch [lo, lo + cnt) (four per workgroup); the arcs of the lists whose source takes part
// (live; kFw: has fw; kBw: has no bw yet) are walked as bvg_arcwalk.h describes.  `key` is colour[] (kBucket: rep[]).  What an arc gives
// its SOURCE (has-live-out, bw, the bucket bits) is collected per list in LDS and written once per list.  A target outside [0, n) is a
// malformed stream: it is flagged and never used as an index.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) scc_sweep_kernel(const uint64_t* cum, int64_t lo, int64_t cnt, const int64_t* succ, int64_t n, const T* key, T* colour,
                                                        uint8_t* flags, unsigned long long* ctl) {
    __shared__ ArcWalk walk_s[4];
    __shared__ T key_s[4][64];
    __shared__ unsigned hit_s[4][64];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ArcWalk& walk = walk_s[w]; T* keys = key_s[w]; unsigned* hit = hit_s[w];
    unsigned met = 0;                      // what this lane met (mOob, mWrote).  One word: see bvg_arcwalk.h on what a walk's functor captures
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const int64_t i = x0 + lane;
        const bool valid = i < cnt;
        const uint64_t b = valid ? cum[i] : 0, e = valid ? cum[i + 1] : 0;
        const int64_t u = lo + i;
        T ku = none<T>();
        if (valid && e > b) {
            ku = key[u];
            if (MODE == kFw && ku != none<T>() && !(flags[u] & fFw)) ku = none<T>();
            if (MODE == kBw && ku != none<T>() && (flags[u] & fBw)) ku = none<T>();
        }
        const bool act = ku != none<T>();
        const uint64_t total = walk.begin(lane, act, b, e, [&] { keys[lane] = ku; hit[lane] = 0; });
        if (total == 0) continue;                                            // (uniform: no list of this group takes part)
        walk.for_each_arc(lane, total, [&](int l, uint64_t at) {
            const int64_t y = succ[at];
            if (y < 0 || y >= n) { met |= mOob; return; }
            const T cu = keys[l];
            if (MODE == kTrim) {
                if (y != lo + x0 + l && key[y] == cu) {
                    if (!hit[l]) hit[l] = 1;
                    if (!(flags[y] & fIn)) set_flag(flags, y, fIn);
                }
            } else if (MODE == kFw) {
                if (key[y] == cu && !(flags[y] & fFw)) { set_flag(flags, y, fFw); met |= mWrote; }
            } else if (MODE == kBw) {
                if (!hit[l] && key[y] == cu && (flags[y] & fBw)) hit[l] = 1;
            } else if (MODE == kColour) {
                const T cv = colour[y];
                if (cv != none<T>() && cv < cu) { __hip_atomic_fetch_max(colour + y, cu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); met |= mWrote; }
            } else {
                const unsigned h = key[y] != cu ? fArc | fLeave : fArc;
                if ((hit[l] & h) != h) atomicOr(hit + l, h);
            }
        });
        __builtin_amdgcn_wave_barrier();                                     // (every lane's hit[] writes before the lists' own lanes read them)
        if (act && hit[lane]) {
            if (MODE == kTrim) set_flag(flags, u, fOut);
            else if (MODE == kBw) { set_flag(flags, u, fBw); met |= mWrote; }
            else if (MODE == kBucket) { if ((flags[ku] & hit[lane]) != hit[lane]) set_flag(flags, (int64_t)ku, hit[lane]); }
        }
        walk.end();
    }
    if (met & mOob) atomicOr(ctl + kCtlBad, 1ull);
    if (__ballot(met & mWrote) && lane == 0 && ctl[kCtlChanged] == 0) atomicOr(ctl + kCtlChanged, 1ull);
}

template <typename T> __global__ void scc_init_kernel(T* rep, T* colour, uint8_t* flags, int64_t n) {
    BVG_FOR(x, n) { rep[x] = none<T>(); colour[x] = 0; flags[x] = 0; }
}

// after a trim sweep: a live node without a live in-arc or without a live out-arc is an SCC of its own; the two bits are cleared for the next
// pass.  ctl[kCtlCount] += the nodes retired (one atomic per wavefront)
template <typename T> __global__ void __launch_bounds__(256) scc_trim_retire_kernel(T* rep, T* colour, uint8_t* flags, int64_t n, unsigned long long* ctl) {
    for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x; x0 < n; x0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform per workgroup: the ballot below)
        const int64_t x = x0 + threadIdx.x;
        bool gone = false;
        if (x < n && colour[x] != none<T>()) {
            const unsigned f = flags[x];
            gone = (f & (fIn | fOut)) != (fIn | fOut);
            if (gone) { rep[x] = (T)x; colour[x] = none<T>(); }
            flags[x] = 0;                                                    // (fw and bw are clear whenever a trim runs)
        }
        const uint64_t g = __ballot(gone);
        if (g && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(g)) atomicAdd(ctl + kCtlCount, (unsigned long long)__builtin_popcountll(g));
    }
}

// the pivot over the outdegrees of a batch: the largest outdegree among the live nodes, then the smallest live node that has it
template <typename T> __global__ void scc_maxdeg_kernel(const int32_t* deg, int64_t lo, int64_t cnt, const T* colour, unsigned long long* ctl) {
    BVG_FOR(i, cnt) if (colour[lo + i] != none<T>() && (unsigned long long)deg[i] > ctl[kCtlMaxDeg]) atomicMax(ctl + kCtlMaxDeg, (unsigned long long)deg[i]);
}
template <typename T> __global__ void scc_pivot_kernel(const int32_t* deg, int64_t lo, int64_t cnt, const T* colour, unsigned long long* ctl) {
    BVG_FOR(i, cnt) if (colour[lo + i] != none<T>() && (unsigned long long)deg[i] == ctl[kCtlMaxDeg] && (unsigned long long)(lo + i) < ctl[kCtlPivot])
        atomicMin(ctl + kCtlPivot, (unsigned long long)(lo + i));
}
__global__ void scc_seed_kernel(uint8_t* flags, int64_t pivot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[pivot] = fFw | fBw;
}

// Retirement, first half.  Members: fw and bw (FWBW: the step from the pivot, key = the pivot) or bw (a colouring round, key = the colour).
// rep[key] = the smallest member (key is a member and live: all ones before); ctl[kCtlCount] += members, ctl[kCtlRoots] += members that
// are their own key.  Membership is read from the flags alone, which no thread of this kernel writes.
template <typename T, bool FWBW> __global__ void __launch_bounds__(256) scc_min_kernel(T* rep, const T* colour, const uint8_t* flags, int64_t n, T pivot, unsigned long long* ctl) {
    for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x; x0 < n; x0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform per workgroup)
        const int64_t x = x0 + threadIdx.x;
        bool in = false, root = false;
        if (x < n) {
            const unsigned f = flags[x];
            in = FWBW ? (f & (fFw | fBw)) == (fFw | fBw) : (f & fBw) != 0;
            if (in) {
                const T k = FWBW ? pivot : colour[x];
                root = k == (T)x;
                if (rep[k] > (T)x) __hip_atomic_fetch_min(rep + k, (T)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a stale rep[k] is larger: a wasted atomic)
            }
        }
        const uint64_t m = __ballot(in), rt = __ballot(root);
        if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) {
            atomicAdd(ctl + kCtlCount, (unsigned long long)__builtin_popcountll(m));
            if (rt) atomicAdd(ctl + kCtlRoots, (unsigned long long)__builtin_popcountll(rt));
        }
    }
}

// Retirement, second half: a member takes rep[key] (the key itself holds it already) and leaves; fw and bw are cleared on every node.  FWBW:
// the live rest is coloured 1 + fw + 2 bw (no SCC crosses these three classes)
template <typename T, bool FWBW> __global__ void scc_retire_kernel(T* rep, T* colour, uint8_t* flags, int64_t n, T pivot) {
    BVG_FOR(x, n) {
        if (colour[x] == none<T>()) continue;
        const unsigned f = flags[x];
        const bool in = FWBW ? (f & (fFw | fBw)) == (fFw | fBw) : (f & fBw) != 0;
        if (in) {
            const T k = FWBW ? pivot : colour[x];
            if (k != (T)x) rep[x] = rep[k];                                  // (thread k does not write rep[k])
            colour[x] = none<T>();
        } else if (FWBW) colour[x] = (T)(1 + ((f >> 2) & 3));
        flags[x] = 0;
    }
}

template <typename T> __global__ void scc_own_colour_kernel(T* colour, int64_t n) {
    BVG_FOR(x, n) if (colour[x] != none<T>()) colour[x] = (T)x;
}
template <typename T> __global__ void scc_roots_kernel(const T* colour, uint8_t* flags, int64_t n) {
    BVG_FOR(x, n) if (colour[x] == (T)x) flags[x] = fBw;
}
// after the bucket sweep: x is in a bucket when its SCC has an arc and none that leaves it
template <typename T> __global__ void scc_buckets_kernel(const T* rep, const uint8_t* flags, int64_t n, uint8_t* out) {
    BVG_FOR(x, n) out[x] = (flags[rep[x]] & (fArc | fLeave)) == fArc ? 1 : 0;
}

}  // namespace

}  // namespace bvg

namespace {

using bvghost::Batch;

constexpr int kMaxReruns = 8;       // of the kernel on one resident batch of several, while it still changes something (a stated default, not measured)

enum : int { kSweeps, kDecodes, kTrimPasses, kTrimmed, kFwBwSize, kRounds, kColourComponents, kResident };   // bvg_scc's counters

template <typename T> struct SccRun {
    bvg_graph* g; bvghost::SweepPlan sp; int64_t n;
    T* rep; T* colour; uint8_t* flags; unsigned long long* ctl;
    uint64_t counters[BVG_SCC_COUNTERS] = {};
    unsigned long long h[kCtlWords] = {};                                    // the control words as last read

    int zero_ctl() { HIPCHK(hipMemsetAsync(ctl, 0, kCtlWords * 8, g->stream)); return 0; }
    int read_ctl() {                                                         // BVG_E_EOF: a successor outside [0, n) was met
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        return h[kCtlBad] ? BVG_E_EOF : 0;
    }
    template <int MODE> void launch(const Batch& b) {
        const int64_t cnt = b.hi - b.lo;
        hipLaunchKernelGGL((scc_sweep_kernel<T, MODE>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const uint64_t*)sp.cum(), b.lo, cnt, (const int64_t*)sp.succ(), n,
                           (const T*)(MODE == kBucket ? rep : colour), colour, flags, ctl);
    }
    // one complete sweep of a mode without a fixpoint (trim, buckets): nothing is read back
    template <int MODE> int sweep_plain() {
        for (const Batch& b : sp.batches) { const int rc = sp.load(g, b, &counters[kDecodes]); if (rc) return rc; launch<MODE>(b); HIPCHK(hipGetLastError()); }
        counters[kSweeps]++;
        return 0;
    }
    // a propagation to its fixpoint: complete sweeps until one performs no write
    template <int MODE> int propagate() {
        for (bool wrote = true; wrote;) {
            wrote = false;
            for (const Batch& b : sp.batches) {
                int rc = sp.load(g, b, &counters[kDecodes]); if (rc) return rc;
                for (int run = 0;; run++) {
                    rc = zero_ctl(); if (rc) return rc;
                    launch<MODE>(b);
                    rc = read_ctl(); if (rc) return rc;
                    if (!h[kCtlChanged]) break;
                    wrote = true;
                    if (sp.single() || run + 1 >= kMaxReruns) break;              // (one batch: the next launch IS the next sweep)
                }
            }
            counters[kSweeps]++;
        }
        return 0;
    }
    // trim passes until one retires nothing; *live is kept
    int trim(uint64_t* live) {
        for (;;) {
            int rc = zero_ctl(); if (rc) return rc;
            rc = sweep_plain<kTrim>(); if (rc) return rc;
            hipLaunchKernelGGL((scc_trim_retire_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, rep, colour, flags, n, ctl);
            rc = read_ctl(); if (rc) return rc;
            counters[kTrimPasses]++;
            counters[kTrimmed] += h[kCtlCount]; *live -= h[kCtlCount];
            if (!h[kCtlCount] || !*live) return 0;
        }
    }
    // the default pivot: the outdegrees of every batch once more (its `deg` piece of the workspace is free once the batch is decoded); -1: no node is live
    int pick_pivot(int64_t* pivot) {
        int32_t* const deg = (int32_t*)(sp.base + sp.o_deg);
        int rc = zero_ctl(); if (rc) return rc;
        const unsigned long long top = ~0ull;
        HIPCHK(hipMemcpyAsync(ctl + kCtlPivot, &top, 8, hipMemcpyHostToDevice, g->stream));
        for (int pass = 0; pass < 2; pass++)
            for (const Batch& b : sp.batches) {
                const int64_t cnt = b.hi - b.lo;
                outdegrees_of(g, b.lo, b.hi, deg);
                if (pass == 0) hipLaunchKernelGGL((scc_maxdeg_kernel<T>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const int32_t*)deg, b.lo, cnt, (const T*)colour, ctl);
                else hipLaunchKernelGGL((scc_pivot_kernel<T>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const int32_t*)deg, b.lo, cnt, (const T*)colour, ctl);
            }
        rc = read_ctl(); if (rc) return rc;
        *pivot = h[kCtlPivot] == top ? -1 : (int64_t)h[kCtlPivot];
        return 0;
    }
    // members -> rep, everything else keeps going; h[kCtlCount] / h[kCtlRoots]: the members / the SCCs retired
    template <bool FWBW> int retire(T pivot) {
        int rc = zero_ctl(); if (rc) return rc;
        hipLaunchKernelGGL((scc_min_kernel<T, FWBW>), dim3(grid(n, 256)), dim3(256), 0, g->stream, rep, (const T*)colour, (const uint8_t*)flags, n, pivot, ctl);
        hipLaunchKernelGGL((scc_retire_kernel<T, FWBW>), dim3(grid(n, 256)), dim3(256), 0, g->stream, rep, colour, flags, n, pivot);
        return read_ctl();
    }
};

template <typename T> int scc_t(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, uint8_t* buckets, uint64_t* counters, bool dev) {
    const int64_t n = g->sh->p.nodes;
    const bool dbgt = dbg_on();
    Stopwatch sw;
    DevArray<T> rep, colour; DevArray<uint8_t> fl, dbuck; DevArray<unsigned long long> ctl;
    if (rep.alloc((size_t)n) || colour.alloc((size_t)n) || fl.alloc(((size_t)n + 3) & ~(size_t)3) || ctl.alloc(kCtlWords)) return BVG_E_NOMEM;
    uint8_t* d_buckets = buckets;
    if ((flags & BVG_SCC_BUCKETS) && !dev) { if (dbuck.alloc((size_t)n)) return BVG_E_NOMEM; d_buckets = dbuck; }
    SccRun<T> r;
    r.g = g; r.n = n; r.rep = rep; r.colour = colour; r.flags = fl; r.ctl = ctl;
    hipLaunchKernelGGL((scc_init_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, r.rep, r.colour, r.flags, n);
    index_first(g);
    uint64_t per = 0;                                                       // (of what is free once the per-node arrays are there)
    int rc = arc_budget(n, kMaxBatchArcs, "BVG_SCC_BATCH_ARCS", &per); if (rc) return rc;
    rc = r.sp.build(g, per); if (rc) return rc;
    r.counters[kResident] = r.sp.single() ? 1 : 0;
    uint64_t live = (uint64_t)n;
    {
        DevArray<uint8_t> ws;                                                    // (this scope: gone before the numbering pass, which needs the memory)
        if (!r.sp.batches.empty()) { if (ws.alloc(r.sp.bytes)) return BVG_E_NOMEM; r.sp.bind(ws.get()); }
        rc = r.trim(&live); if (rc) return rc;
        // the FW-BW step
        int64_t pivot = -1; bool want_step = live != 0;
        if (const char* k = knob("BVG_SCC_PIVOT")) {
            if (!strcmp(k, "none")) want_step = false;
            else if (isdigit((unsigned char)k[0]) && atoll(k) < n) pivot = atoll(k);
        }
        if (want_step && pivot >= 0) {                                      // (a pivot given by hand may have been trimmed: no step then)
            T c = 0;
            HIPCHK(hipMemcpyAsync(&c, r.colour + pivot, sizeof(T), hipMemcpyDeviceToHost, g->stream));
            HIPCHK(hipStreamSynchronize(g->stream));
            if (c == none<T>()) want_step = false;
        } else if (want_step) { rc = r.pick_pivot(&pivot); if (rc) return rc; want_step = pivot >= 0; }
        if (want_step) {
            hipLaunchKernelGGL(scc_seed_kernel, dim3(1), dim3(64), 0, g->stream, r.flags, pivot);
            rc = r.template propagate<kFw>(); if (rc) return rc;
            rc = r.template propagate<kBw>(); if (rc) return rc;
            rc = r.template retire<true>((T)pivot); if (rc) return rc;
            r.counters[kFwBwSize] = r.h[kCtlCount]; live -= r.h[kCtlCount];
        }
        // colouring rounds
        while (live) {
            rc = r.trim(&live); if (rc) return rc;
            if (!live) break;
            r.counters[kRounds]++;
            hipLaunchKernelGGL((scc_own_colour_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, r.colour, n);
            rc = r.template propagate<kColour>(); if (rc) return rc;
            hipLaunchKernelGGL((scc_roots_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, (const T*)r.colour, r.flags, n);
            rc = r.template propagate<kBw>(); if (rc) return rc;
            rc = r.template retire<false>((T)0); if (rc) return rc;
            if (!r.h[kCtlCount] || r.h[kCtlCount] > live) return BVG_E_STATE;   // (every round retires the SCC of the largest live node at least)
            r.counters[kColourComponents] += r.h[kCtlRoots]; live -= r.h[kCtlCount];
        }
        if (flags & BVG_SCC_BUCKETS) {                                      // (every flags byte is 0 by now)
            rc = r.zero_ctl(); if (rc) return rc;
            rc = r.template sweep_plain<kBucket>(); if (rc) return rc;
            hipLaunchKernelGGL((scc_buckets_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, (const T*)r.rep, (const uint8_t*)r.flags, n, d_buckets);
            rc = r.read_ctl(); if (rc) return rc;
        }
        HIPCHK(hipStreamSynchronize(g->stream));
    }
    colour.reset(); fl.reset();                                              // the numbering takes 12 bytes per node of its own
    const double t_scc = sw.lap();
    if (counters) memcpy(counters, r.counters, sizeof r.counters);
    uint64_t count = 0;
    rc = number_components(g, rep.get(), sizeof(T) == 8, (flags & BVG_SCC_SORT_BY_SIZE) ? BVG_CC_SORT_BY_SIZE : 0u, comp, sizes, sizes_cap, n_components, dev, &count);
    if (rc && rc != BVG_E_CAPACITY) return rc;
    if ((flags & BVG_SCC_BUCKETS) && !dev) HIPCHK(hipMemcpy(buckets, d_buckets, (size_t)n, hipMemcpyDeviceToHost));
    if (dbgt) fprintf(stderr, "[bvg] scc: %zu batches of <= %llu arcs (%llu arcs), %llu sweeps, %llu decodes, %llu trim passes (%llu nodes), fw-bw %llu nodes, %llu rounds (%llu components): "
                      "%.1f ms, numbering %.1f ms (%llu components)\n", r.sp.batches.size(), (unsigned long long)per, (unsigned long long)r.sp.arcs, (unsigned long long)r.counters[kSweeps],
                      (unsigned long long)r.counters[kDecodes], (unsigned long long)r.counters[kTrimPasses], (unsigned long long)r.counters[kTrimmed], (unsigned long long)r.counters[kFwBwSize],
                      (unsigned long long)r.counters[kRounds], (unsigned long long)r.counters[kColourComponents], t_scc, sw.lap(), (unsigned long long)count);
    return rc;
}

int scc_impl(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, uint8_t* buckets, uint64_t* counters, bool dev) {
    if (!g || !n_components) return BVG_E_ARG;
    if (flags & ~(uint32_t)(BVG_SCC_SORT_BY_SIZE | BVG_SCC_BUCKETS)) return BVG_E_ARG;
    if ((flags & BVG_SCC_BUCKETS) && !buckets) return BVG_E_ARG;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    Shared* sh = g->sh;
    *n_components = 0;
    if (counters) memset(counters, 0, BVG_SCC_COUNTERS * sizeof(uint64_t));
    if (sh->p.nodes == 0) return 0;
    if (!comp) return BVG_E_ARG;
    HIPCHK(hipSetDevice(sh->device));
    return (sh->wide || g->tun.force_wide) ? scc_t<uint64_t>(g, flags, comp, sizes, sizes_cap, n_components, buckets, counters, dev)
                                           : scc_t<uint32_t>(g, flags, comp, sizes, sizes_cap, n_components, buckets, counters, dev);
}

}  // namespace

int bvg_scc(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, uint8_t* buckets, uint64_t* counters) {
    return guarded([&] { return scc_impl(g, flags, comp, sizes, sizes_cap, n_components, buckets, counters, false); });
}
int bvg_scc_dev(bvg_graph* g, uint32_t flags, void* d_comp, void* d_sizes, uint64_t sizes_cap, uint64_t* n_components, void* d_buckets, uint64_t* counters) {
    return guarded([&] { return scc_impl(g, flags, (int64_t*)d_comp, (int64_t*)d_sizes, sizes_cap, n_components, (uint8_t*)d_buckets, counters, true); });
}
