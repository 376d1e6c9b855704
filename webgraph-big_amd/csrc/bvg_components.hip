// bvg_components.hip — weakly connected components on the device (algo/ConnectedComponents.java).
//
// The reference runs ParallelBreadthFirstVisit.visitAll() over a symmetric graph (ParallelBreadthFirstVisit.java:272-337): nodes are
// scanned in increasing order and a new round starts at every node not visited yet, so component c is the one whose smallest node is the
// c-th smallest among the components' smallest nodes.  Here the same partition and the same numbering come from a concurrent union-find
// over a parent array (one element per node) that consumes the decode one arc-bounded batch at a time: no transpose, no symmetric copy,
// no CSR of the whole graph in HBM.  Union-find is symmetric, so hooking every arc of a directed graph gives its weak components
// (= compute(new UnionImmutableGraph(g, gT)), the reference's `main -t`).
//
//   init      parent[x] = x
//   hook      per arc (u, v) of a materialised batch: find both roots (path halving), link the larger root under the smaller with a
//             compare-and-swap, retry from the value a failed CAS returns.  A root only ever gets a smaller parent, so every final root
//             is the smallest node of its component: the reference's numbering with no extra pass.
//   compress  parent[x] = find(x) (a read-only walk); flag[x] = x is a root
//   number    rank = exclusive scan of the flags; comp[x] = rank[parent[x]]; the count is the scan total
//   sizes     histogram of comp, one atomic per run of equal labels inside a wavefront (the giant component makes one address hot)
//   sort      ConnectedComponents.sortBySize: stable radix sort of (n - size, old index), the permutation inverted, comp remapped
//
// Concurrency.  parent[] is read and halved with plain loads and stores: a CU's vector L1 is never refreshed by another CU's stores,
// so a read may be stale, and the agent-scope CAS of a link is the authoritative re-read.  Values only ever move to ancestors
// (parent[x] <= x always, and a halving store writes an ancestor of x), so a stale read is an older ancestor: it costs a longer walk
// or a failed CAS, never a wrong partition, and every retry moves to a smaller id, so none spins.  (Agent-scope atomic loads, which
// bypass L1, made the hook 1.7 times slower on the eu-like stand-in: DESIGN.md.)  A CAS succeeds only on a root, and a halving store touches only a node that is no root any more, so the two never
// overwrite each other's link.  Roots are read with loads first and the CAS is issued only when they differ: at most n - 1 CASes
// succeed, so the atomic count scales with nodes, not arcs.
#include <cstdint>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "bvg_arcwalk.h"
#include "bvg_host.h"
#include "../../include/bvgraph_hip.h"

namespace bvg {

namespace {

// plain loads and stores (L1-cached): a stale value is an older ancestor, and the CAS in unite() is the authoritative re-read
template <typename T> __device__ __forceinline__ T ld_parent(const T* p) { return *p; }
template <typename T> __device__ __forceinline__ void st_parent(T* p, T v) { *p = v; }

// root of x with path halving: parent[x] <- parent[parent[x]] on the way up (benign races: both values are ancestors of x).
// HALVE = false: a read-only walk (compress: there a halving store could overwrite a node's root, just written by its own thread,
// with an ancestor further down)
template <typename T, bool HALVE = true> __device__ __forceinline__ T find_root_from(T* parent, T x, T p) {   // (p: parent[x] as read)
    while (p != x) {
        const T gp = ld_parent(parent + p);
        if (gp == p) return p;
        if (HALVE) st_parent(parent + x, gp);
        x = gp;
        p = ld_parent(parent + x);
    }
    return x;
}
template <typename T, bool HALVE = true> __device__ __forceinline__ T find_root(T* parent, T x) { return find_root_from<T, HALVE>(parent, x, ld_parent(parent + x)); }

// union of the trees of roots a and b (any order): the larger root goes under the smaller.  A failed CAS returns the value that
// took its place (the authoritative re-read): the larger root has been linked meanwhile, so both roots are looked up again.
template <typename T> __device__ __forceinline__ void unite(T* parent, T a, T b) {
    while (a != b) {
        const T hi = a > b ? a : b, lo = a > b ? b : a;
        T expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = find_root(parent, expect);
        b = find_root(parent, lo);
    }
}

template <typename T> __global__ void cc_init_kernel(T* parent, int64_t n) {
    BVG_FOR(x, n) parent[x] = (T)x;
}

// One wavefront per 64 consecutive nodes of the batch [lo, lo + cnt) (four per workgroup), its arcs walked as bvg_arcwalk.h describes: the
// root of every source is found once per list (LDS); per arc, find the target's root and unite when the roots differ.  A target outside
// [0, n) is a malformed stream: it is flagged (*bad) and not followed.
template <typename T> __global__ void __launch_bounds__(256) cc_hook_kernel(const uint64_t* cum, int64_t lo, int64_t cnt, const int64_t* succ, int64_t n,
                                                                            T* parent, unsigned* bad) {
    __shared__ ArcWalk walk_s[4];
    __shared__ T root_s[4][64];
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ArcWalk& walk = walk_s[w]; T* roots = root_s[w];
    bool oob = false;
    for (int64_t x0 = ((int64_t)blockIdx.x * 4 + w) * 64; x0 < cnt; x0 += (int64_t)gridDim.x * 256) {   // (whole wavefronts: no workgroup barrier)
        const int64_t i = x0 + lane;
        const bool valid = i < cnt;
        const uint64_t b = valid ? cum[i] : 0, e = valid ? cum[i + 1] : 0;
        const bool act = e > b;
        const uint64_t total = walk.begin(lane, act, b, e, [&] { roots[lane] = act ? find_root(parent, (T)(lo + i)) : (T)0; });   // (no arcs: never read)
        if (total == 0) continue;                                            // (uniform: no list of this group has an arc)
        walk.for_each_arc(lane, total, [&](int l, uint64_t at) {
            const int64_t y = succ[at];
            if (y < 0 || y >= n) { oob = true; return; }
            const T ru = roots[l];
            const T pv = ld_parent(parent + y);
            if (pv == ru) return;                                            // (the common case once the source's component is hooked: one load)
            const T rv = find_root_from(parent, (T)y, pv);
            if (ru != rv) unite(parent, ru, rv);
        });
        if (oob) atomicOr(bad, 1u);
        walk.end();
    }
}

// parent[x] = root of x; flag[x] = 1 for the roots.  Only thread x writes parent[x], and with the root, so the label kernel reads
// every node's root in one load; the other threads' walks through x see the old or the new value, both ancestors
template <typename T> __global__ void cc_compress_kernel(T* parent, int64_t n, int32_t* flag) {
    BVG_FOR(x, n) {
        const T r = find_root<T, false>(parent, (T)x);
        st_parent(parent + x, r);
        flag[x] = r == (T)x ? 1 : 0;
    }
}

template <typename T> __global__ void cc_label_kernel(const T* parent, int64_t n, const uint64_t* rank, int64_t* comp) {
    BVG_FOR(x, n) comp[x] = (int64_t)rank[parent[x]];
}

// sizes[comp[x]] += 1: consecutive nodes mostly share a label, so each wavefront adds one count per run of equal labels among its
// 64 lanes (atomics run at the memory side: 64 lanes on one hot address would serialise there)
__global__ void __launch_bounds__(256) cc_sizes_kernel(const int64_t* comp, int64_t n, unsigned long long* sizes) {
    const unsigned lane = threadIdx.x & 63;
    for (int64_t x0 = (int64_t)blockIdx.x * blockDim.x; x0 < n; x0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform per workgroup: ballots below)
    const int64_t x = x0 + threadIdx.x;
    const bool in = x < n;
    const int64_t c = in ? comp[x] : -1;
    const int64_t prev = __shfl_up(c, 1, 64);
    const bool head = in && (lane == 0 || prev != c);
    const uint64_t heads = __ballot(head);
    const uint64_t live = __ballot(in);
    if (head) {
        const uint64_t above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
        const unsigned next = above ? (unsigned)__builtin_ctzll(above) : 64u - (unsigned)__builtin_clzll(live);   // (live: the low lanes)
        atomicAdd(sizes + c, (unsigned long long)(next - lane));
    }
    }
}

// sort key of component i: n - size (ascending = size descending); values: the old index (increasing, so a stable sort orders ties by it)
__global__ void cc_sort_keys_kernel(const unsigned long long* sizes, uint64_t count, uint64_t n, uint64_t* keys, uint64_t* idx) {
    BVG_FOR(i, count) {
        keys[i] = n - (uint64_t)sizes[i];
        idx[i] = (uint64_t)i;
    }
}

// new index of old component order[j] is j; sizes in the new order
__global__ void cc_invert_kernel(const uint64_t* keys_sorted, const uint64_t* order, uint64_t count, uint64_t n, uint64_t* newidx, unsigned long long* sizes) {
    BVG_FOR(j, count) {
        newidx[order[j]] = (uint64_t)j;
        sizes[j] = (unsigned long long)(n - keys_sorted[j]);
    }
}

__global__ void cc_remap_kernel(int64_t* comp, int64_t n, const uint64_t* newidx) {
    BVG_FOR(x, n) comp[x] = (int64_t)newidx[comp[x]];
}

}  // namespace

}  // namespace bvg

namespace {


// compress + number + sizes + sort over a parent array whose trees are complete (the batch buffer is gone by now): what bvg_components
// and bvg_scc (there parent[x] is the smallest node of x's component already) share through number_components (bvg_host.h).
// 0 or BVG_E_CAPACITY (sizes_cap below the count; comp and the count written all the same); *count_out: the count
template <typename T> int number_t(bvg_graph* g, T* d_parent, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, bool dev, uint64_t* count_out) {
    const int64_t n = g->sh->p.nodes;
    DevArray<int32_t> flag; DevArray<uint64_t> rank, tmp; DevArray<int64_t> dcomp;
    if (flag.alloc((size_t)n) || rank.alloc((size_t)n + 1) || tmp.alloc(scan_tmp_elems(n))) return BVG_E_NOMEM;
    int64_t* d_comp = comp;
    if (!dev) { if (dcomp.alloc((size_t)n)) return BVG_E_NOMEM; d_comp = dcomp; }
    hipLaunchKernelGGL((cc_compress_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, d_parent, n, flag.get());
    launch_exclusive_scan(flag.get(), rank.get(), n, tmp.get(), g->stream);
    hipLaunchKernelGGL((cc_label_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, (const T*)d_parent, n, rank.get(), d_comp);
    uint64_t count = 0;
    HIPCHK(hipMemcpyAsync(&count, rank.get() + n, 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (n_components) *n_components = count;
    const bool want_sizes = sizes != nullptr || (flags & BVG_CC_SORT_BY_SIZE);
    const bool cap_ok = sizes == nullptr || sizes_cap >= count;
    if (want_sizes && count) {
        DevArray<unsigned long long> dsz;
        unsigned long long* d_sizes = (dev && sizes && cap_ok) ? (unsigned long long*)sizes : nullptr;
        if (!d_sizes) { if (dsz.alloc(count)) return BVG_E_NOMEM; d_sizes = dsz; }
        HIPCHK(hipMemsetAsync(d_sizes, 0, count * 8, g->stream));
        hipLaunchKernelGGL(cc_sizes_kernel, dim3(grid(n, 256)), dim3(256), 0, g->stream, (const int64_t*)d_comp, n, d_sizes);
        if (flags & BVG_CC_SORT_BY_SIZE) {
            const unsigned bits = 64u - (unsigned)__builtin_clzll((unsigned long long)n);       // keys n - size <= n - 1
            size_t sort_b = 0;
            if (rocprim::radix_sort_pairs(nullptr, sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)count, 0u, bits, g->stream) != hipSuccess)
                return BVG_E_HIP;
            DevArray<uint64_t> keys, keys2, idx, idx2; DevArray<uint8_t> st;                             // (idx2 doubles as the inverse permutation)
            if (keys.alloc(count) || keys2.alloc(count) || idx.alloc(count) || idx2.alloc(count) || st.alloc(sort_b)) return BVG_E_NOMEM;
            hipLaunchKernelGGL(cc_sort_keys_kernel, dim3(grid((int64_t)count, 256)), dim3(256), 0, g->stream, (const unsigned long long*)d_sizes, count, (uint64_t)n,
                               keys.get(), idx.get());
            if (rocprim::radix_sort_pairs(st.get(), sort_b, (const uint64_t*)keys.get(), keys2.get(), (const uint64_t*)idx.get(), idx2.get(), (size_t)count, 0u, bits, g->stream) != hipSuccess)
                return BVG_E_HIP;
            hipLaunchKernelGGL(cc_invert_kernel, dim3(grid((int64_t)count, 256)), dim3(256), 0, g->stream, keys2.get(), idx2.get(), count, (uint64_t)n,
                               idx.get(), d_sizes);
            hipLaunchKernelGGL(cc_remap_kernel, dim3(grid(n, 256)), dim3(256), 0, g->stream, d_comp, n, idx.get());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(g->stream));
        }
        if (sizes && cap_ok) {
            if (!dev) HIPCHK(hipMemcpyAsync(sizes, d_sizes, count * 8, hipMemcpyDeviceToHost, g->stream));
            else if ((void*)d_sizes != (void*)sizes) HIPCHK(hipMemcpyAsync(sizes, d_sizes, count * 8, hipMemcpyDeviceToDevice, g->stream));
        }
        HIPCHK(hipStreamSynchronize(g->stream));
    }
    if (!dev) HIPCHK(hipMemcpy(comp, d_comp, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipGetLastError());
    *count_out = count;
    return cap_ok ? 0 : BVG_E_CAPACITY;
}

template <typename T> int components_t(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, bool dev) {
    Shared* sh = g->sh; const int64_t n = sh->p.nodes;
    const bool dbgt = dbg_on();
    Stopwatch sw;
    index_first(g);
    DevArray<T> parent;
    if (parent.alloc((size_t)n)) return BVG_E_NOMEM;
    T* const d_parent = parent;
    hipLaunchKernelGGL((cc_init_kernel<T>), dim3(grid(n, 256)), dim3(256), 0, g->stream, d_parent, n);
    uint64_t per = 0;                                                       // (of what is free once the parent array is there)
    int rc = arc_budget(n, kMaxBatchArcs, "BVG_CC_BATCH_ARCS", &per); if (rc) return rc;
    SweepPlan sp;
    rc = sp.build(g, per); if (rc) return rc;
    const double t_plan = sw.lap();
    double t_dec = 0, t_hook = 0;
    DevArray<unsigned> d_bad;
    if (d_bad.alloc(64)) return BVG_E_NOMEM;
    HIPCHK(hipMemsetAsync(d_bad.get(), 0, sizeof(unsigned), g->stream));
    if (!sp.batches.empty()) {
        DevArray<uint8_t> ws;                                                    // (this scope: gone before the numbering pass, which needs the memory)
        if (ws.alloc(sp.bytes)) return BVG_E_NOMEM;                         // parent array + the largest batch: does not fit
        sp.bind(ws.get());
        for (const Batch& b : sp.batches) {
            const int64_t cnt = b.hi - b.lo;
            sw.lap();
            rc = sp.decode(g, b); if (rc) return rc;
            if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_dec += sw.lap(); }
            hipLaunchKernelGGL((cc_hook_kernel<T>), dim3(grid(cnt, 256)), dim3(256), 0, g->stream, (const uint64_t*)sp.cum(), b.lo, cnt, (const int64_t*)sp.succ(), n, d_parent,
                               d_bad.get());
            HIPCHK(hipGetLastError());
            if (dbgt) { HIPCHK(hipStreamSynchronize(g->stream)); t_hook += sw.lap(); }
        }
    }
    unsigned bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad.get(), sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (bad) return BVG_E_EOF;                                              // a successor outside [0, n): malformed stream
    sw.lap();
    uint64_t count = 0;
    rc = number_t<T>(g, d_parent, flags, comp, sizes, sizes_cap, n_components, dev, &count);
    if (rc && rc != BVG_E_CAPACITY) return rc;
    if (dbgt) fprintf(stderr, "[bvg] components: plan %.1f ms (%zu batches of <= %llu arcs, %llu arcs), decode %.1f ms, hook %.1f ms, finish %.1f ms (%llu components)\n",
                      t_plan, sp.batches.size(), (unsigned long long)per, (unsigned long long)sp.arcs, t_dec, t_hook, sw.lap(), (unsigned long long)count);
    return rc;
}

int components_impl(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, bool dev) {
    if (!g) return BVG_E_ARG;
    if (flags & ~(uint32_t)BVG_CC_SORT_BY_SIZE) return BVG_E_ARG;
    if (g->node_base != 0) return BVG_E_ARG;                 // a shard's targets leave its node range: the whole graph only
    Shared* sh = g->sh;
    if (n_components) *n_components = 0;
    if (sh->p.nodes == 0) return 0;
    if (!comp) return BVG_E_ARG;
    HIPCHK(hipSetDevice(sh->device));
    const bool wide = sh->wide || g->tun.force_wide;
    return wide ? components_t<uint64_t>(g, flags, comp, sizes, sizes_cap, n_components, dev) : components_t<uint32_t>(g, flags, comp, sizes, sizes_cap, n_components, dev);
}

}  // namespace

namespace bvghost {
int number_components(bvg_graph* g, void* d_parent, bool wide, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, bool dev,
                      uint64_t* count_out) {
    return wide ? number_t<uint64_t>(g, (uint64_t*)d_parent, flags, comp, sizes, sizes_cap, n_components, dev, count_out)
                : number_t<uint32_t>(g, (uint32_t*)d_parent, flags, comp, sizes, sizes_cap, n_components, dev, count_out);
}
}  // namespace bvghost

int bvg_components(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components) {
    return guarded([&] { return components_impl(g, flags, comp, sizes, sizes_cap, n_components, false); });
}
int bvg_components_dev(bvg_graph* g, uint32_t flags, void* d_comp, void* d_sizes, uint64_t sizes_cap, uint64_t* n_components) {
    return guarded([&] { return components_impl(g, flags, (int64_t*)d_comp, (int64_t*)d_sizes, sizes_cap, n_components, true); });
}
