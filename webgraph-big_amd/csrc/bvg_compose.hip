// bvg_compose.hip — Transform.compose on the device (Transform.java:1666-1775, the unlabelled form): the Boolean product of two graphs,
// row x of the result = the sorted union of N1(y) over the successors y of x in g0, from two CSRs in HBM to a CSR in HBM.  The contract
// is the one of include/bvgraph_hip.h ("Compose"); DESIGN.md 7k has the reasons and what was measured.
//
// The reference keeps a hash set per node.  So does this: every row is hashed ON CHIP by the one wavefront or workgroup that owns it from
// its first product to its last successor, so memory grows with the sources and the result and never with the products (cnr-2000 with
// its transpose has 15.6 G of them).  The stages:
//   1  BOUND    ub[x] = the sum of outdeg1(y) over y in N0(x), y < n1 (64 bits): the products of the row, an upper bound of its length.
//   2  TIERS    by ub, on the host (ub[] is read back: 8 bytes per node):
//        tier 0  ub <= kLimit0   one wavefront per row (workgroups of one wavefront), a table of at most kSlots0 keys in LDS;
//        tier 1  ub <= kLimit1   one workgroup of kThreads1 per row, a table of at most kSlots1 keys in LDS;
//        tier 2  the rest        one workgroup per row, its table carved from a workspace in HBM of bounded size; the rows run in batches
//                                that fit the budget (a row whose table alone exceeds it: a batch, and an allocation, of its own).
//      A table has 2 pow2ceil(bound) slots (tier 2: bound = min(ub, n), a row holds no more than n keys; the LDS tiers at least 64), so it
//      is never more than half full and a probe sequence ends by construction; every probe loop is capped at `slots` steps all the same,
//      and a cap that is hit raises a flag that the host returns as BVG_E_HIP.  Every index is masked by the table size.
//   3  SYMBOLIC each row's products are inserted (open addressing, linear probing, one compare-and-swap per probe), the NEW keys counted:
//               the row's length.  launch_exclusive_scan -> adj_off; the total is read back once.
//   4  NUMERIC  inserted again.  LDS tiers: the keys are moved to the front of the table, sorted there by a bitonic network over the row's
//               length, and written to adj.  Tier 2: a new key is appended to the row's place in adj as it is
//               inserted, and the owning workgroup then sorts the row in place by the same network over the row's length.
// No wavefront waits on another workgroup: the only synchronisation is the workgroup barrier and atomics on the owner's own table.
// The result is a sorted CSR, so it is the same whatever order the insertions took.
#include <cstdint>

#include "bvg_host.h"
#include "bvg_compose_shared.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

// ---- stage 1
__global__ void compose_bound_kernel(ComposeArgs a, uint64_t* ub) {
    BVG_FOR(x, a.n) {
        uint64_t s = 0;
        if (x < a.n0) for (uint64_t i = a.off0[x], e = a.off0[x + 1]; i < e; i++) {
            const int64_t y = a.adj0[i];
            if (y >= 0 && y < a.n1) s += a.off1[y + 1] - a.off1[y];
        }
        ub[x] = s;
    }
}

// ---- stages 3 and 4: the rows of one tier's list, one workgroup a row.  GLOBAL: the table lies in `ws` at tab_off[r] (tier 2).
template <int THREADS, uint32_t SLOTS, bool GLOBAL>
__global__ void __launch_bounds__(THREADS) compose_rows_kernel(ComposeArgs a, const uint32_t* rows, uint32_t nrows, unsigned long long* ws, const uint64_t* tab_off, int numeric) {
    __shared__ unsigned long long lds[GLOBAL ? 1 : SLOTS];
    __shared__ unsigned fresh;                                                 // new keys of the row so far
    constexpr int WAVES = THREADS / 64;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int64_t x = (int64_t)rows[r];
        const uint64_t ub = a.ub[x];
        uint64_t slots;
        unsigned long long* tab;
        if (GLOBAL) { slots = table_slots2(ub, a.n); tab = ws + tab_off[r]; }   // cleared by the host before the launch
        else {
            slots = 2 * pow2ceil(ub); if (slots < kMinSlots) slots = kMinSlots; if (slots > SLOTS) slots = SLOTS;   // (the host sends no row with 2 ub > SLOTS here)
            tab = lds;
            for (uint32_t i = threadIdx.x; i < (uint32_t)slots; i += THREADS) tab[i] = kEmpty;
        }
        if (threadIdx.x == 0) fresh = 0;
        __syncthreads();
        const uint64_t mask = slots - 1;
        const unsigned bits = 63u - (unsigned)__clzll((long long)slots);
        const uint64_t row_lo = numeric ? a.out_off[x] : 0, row_len = numeric ? a.out_off[x + 1] - row_lo : 0;
        // a wavefront takes 64 successors y of x at a time, one per lane, then the lists N1(y) one after another, 64 keys a step
        const uint64_t lo = a.off0[x], hi = a.off0[x + 1];
        unsigned mine = 0;
        for (uint64_t base = lo + (uint64_t)wave * 64; base < hi; base += (uint64_t)WAVES * 64) {
            const uint64_t idx = base + lane;
            const int64_t y = idx < hi ? a.adj0[idx] : -1;
            const bool in = y >= 0 && y < a.n1;                                // a successor g1 does not have contributes nothing
            const uint64_t s = in ? a.off1[y] : 0, len = in ? a.off1[y + 1] - s : 0;
            unsigned long long live = __ballot(len != 0);
            while (live) {
                const int j = __ffsll((long long)live) - 1;
                live &= live - 1;
                const uint64_t sj = __shfl(s, j, 64), lj = __shfl(len, j, 64);
                for (uint64_t k = lane; k < lj; k += 64) {
                    const unsigned long long z = (unsigned long long)a.adj1[sj + k];
                    if (table_insert(tab, mask, bits, z, a.err)) {
                        if (GLOBAL && numeric) {
                            const uint64_t pos = atomicAdd(&fresh, 1u);
                            if (pos < row_len) a.out_adj[row_lo + pos] = (int64_t)z;
                        } else mine++;
                    }
                }
            }
        }
        if (!(GLOBAL && numeric)) {
            for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
            if (lane == 0 && mine) atomicAdd(&fresh, mine);
        }
        __syncthreads();
        if (!numeric) {
            if (threadIdx.x == 0) a.cnt[x] = (int32_t)fresh;                   // at most n1 < 2^31
        } else {
            if (threadIdx.x == 0 && fresh != row_len) atomicOr(a.err + 1, 1u);
            if (GLOBAL) group_sort<THREADS>((unsigned long long*)(a.out_adj + row_lo), row_len);
            else {
                // the keys to the front of the table, in any order: every thread takes its slots into registers and, all slots read, the
                // keys go where an LDS counter deals them (one addition per wavefront and step).  Then the sort is over the row, not the table.
                constexpr int PER = SLOTS / THREADS > 0 ? SLOTS / THREADS : 1;
                unsigned long long keep[PER];
#pragma unroll
                for (int q = 0; q < PER; q++) { const uint32_t i = (uint32_t)q * THREADS + threadIdx.x; keep[q] = i < slots ? tab[i] : kEmpty; }
                if (threadIdx.x == 0) fresh = 0;                               // (thread 0 has compared it with the row's length above)
                __syncthreads();
#pragma unroll
                for (int q = 0; q < PER; q++) {
                    const bool has = keep[q] != kEmpty;
                    const unsigned long long m = __ballot(has);
                    unsigned at = 0;
                    if (lane == 0 && m) at = atomicAdd(&fresh, (unsigned)__popcll(m));
                    at = __shfl(at, 0, 64) + (unsigned)__popcll(m & ((1ull << lane) - 1));
                    if (has && at < slots) tab[at] = keep[q];
                }
                __syncthreads();
                const uint64_t len = row_len < slots ? row_len : slots;
                group_sort<THREADS>(tab, len);
                for (uint64_t i = threadIdx.x; i < len; i += THREADS) a.out_adj[row_lo + i] = (int64_t)tab[i];
            }
        }
        __syncthreads();                                                       // the table and `fresh` are the next row's
    }
}

// both passes over the three tiers' lists (d_rows: tier 0's, tier 1's, tier 2's rows one after another)
int run_pass(const ComposeArgs& a, const uint32_t* d_rows, const uint64_t count[3], const std::vector<Tier2Batch>& batches, unsigned long long* ws, const uint64_t* d_tab_off, int numeric) {
    auto blocks = [](uint64_t rows) { return dim3((unsigned)(rows < kMaxGrid ? rows : kMaxGrid)); };
    if (count[0]) hipLaunchKernelGGL((compose_rows_kernel<kThreads0, kSlots0, false>), blocks(count[0]), dim3(kThreads0), 0, 0, a, d_rows, (uint32_t)count[0], nullptr, nullptr, numeric);
    if (count[1]) hipLaunchKernelGGL((compose_rows_kernel<kThreads1, kSlots1, false>), blocks(count[1]), dim3(kThreads1), 0, 0, a, d_rows + count[0], (uint32_t)count[1], nullptr, nullptr, numeric);
    const uint32_t* rows2 = d_rows + count[0] + count[1];
    for (const Tier2Batch& b : batches) {
        HIPCHK(hipMemsetAsync(ws, 0xFF, (size_t)b.slots * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL((compose_rows_kernel<kThreads2, 1, true>), blocks(b.hi - b.lo), dim3(kThreads2), 0, 0, a, rows2 + b.lo, b.hi - b.lo, ws, d_tab_off + b.lo, numeric);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int compose_csr(const Source& g0, const Source& g1, bvg_compose_report* report, std::unique_ptr<bvg_text>& out) {
    const int64_t n = g0.n > g1.n ? g0.n : g1.n;
    if ((uint64_t)n > kMaxElems || g0.m > kMaxElems || g1.m > kMaxElems) return BVG_E_UNSUPPORTED;
    int forced = -1;
    if (const char* v = knob("BVG_COMPOSE_TIER")) if (*v >= '0' && *v <= '2' && !v[1]) forced = *v - '0';
    const uint64_t budget = knob_u64("BVG_COMPOSE_WS", kDefaultBudget);
    uint64_t max_arcs = knob_u64("BVG_COMPOSE_MAX_ARCS", kMaxElems);
    if (max_arcs > kMaxElems) max_arcs = kMaxElems;

    bvg_compose_report rep{};
    rep.limit[0] = kLimit0; rep.limit[1] = kLimit1;
    std::unique_ptr<bvg_text> t = new_csr(g0.device);
    t->nodes = n;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    DevArray<uint64_t> ub, tmp, tab_off; DevArray<int32_t> cnt; DevArray<uint32_t> rows; DevArray<unsigned> err; DevArray<unsigned long long> ws;
    if (t->d_off.alloc(nn + 1) || ub.alloc(nn) || cnt.alloc(nn) || rows.alloc(nn) || tmp.alloc(scan_tmp_elems((int64_t)nn)) || err.alloc(2)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(t->d_off.get(), 0, (nn + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemset(cnt.get(), 0, nn * sizeof(int32_t)));
    HIPCHK(hipMemset(err.get(), 0, 2 * sizeof(unsigned)));
    ComposeArgs a{g0.off, g0.adj, g0.n, g1.off, g1.adj, g1.n, n, ub.get(), cnt.get(), t->d_off.get(), nullptr, err.get()};

    uint64_t count[3] = {0, 0, 0}, total = 0;
    std::vector<Tier2Batch> batches;
    const bool dbgt = dbg_on();                                         // BVG_DEBUG: the wall clock of every stage (a synchronisation each)
    Stopwatch sw; double ms_bound = 0, ms_tiers = 0, ms_symbolic = 0, ms_alloc = 0;
    if (n > 0) {
        // stages 1 and 2
        hipLaunchKernelGGL(compose_bound_kernel, dim3(grid(n, 256)), dim3(256), 0, 0, a, ub.get());
        std::vector<uint64_t> h_ub((size_t)n);
        HIPCHK(hipMemcpy(h_ub.data(), ub.get(), (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (dbgt) ms_bound = sw.lap();
        TierPlan plan;
        plan_tiers(h_ub, n, kLimit0, kLimit1, forced, budget / sizeof(unsigned long long), plan);
        rep.products = plan.products;
        for (int i = 0; i < 3; i++) rep.rows[i] = count[i] = plan.count[i];
        if (!plan.rows.empty()) HIPCHK(hipMemcpy(rows.get(), plan.rows.data(), plan.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        // tier 2's batches: tables side by side in the workspace, as many rows as the budget holds
        batches = std::move(plan.batches);
        if (count[2]) {
            if (ws.alloc((size_t)plan.ws_slots) || tab_off.alloc((size_t)count[2])) return BVG_E_NOMEM;
            HIPCHK(hipMemcpy(tab_off.get(), plan.tab.data(), plan.tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
        rep.batches = batches.size();
        if (dbgt) ms_tiers = sw.lap();
        // stage 3
        int rc = run_pass(a, rows.get(), count, batches, ws.get(), tab_off.get(), 0); if (rc) return rc;
        launch_exclusive_scan(cnt.get(), t->d_off.get(), n, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&total, t->d_off.get() + n, sizeof total, hipMemcpyDeviceToHost));
        unsigned h_err[2] = {0, 0};
        HIPCHK(hipMemcpy(h_err, err.get(), sizeof h_err, hipMemcpyDeviceToHost));
        if (h_err[0]) return BVG_E_HIP;
        if (dbgt) ms_symbolic = sw.lap();
    }
    rep.arcs = total;
    if (total > max_arcs) { if (report) *report = rep; return BVG_E_UNSUPPORTED; }
    if (t->adj_base.alloc((size_t)total)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base; t->arcs = total;
    if (dbgt) ms_alloc = sw.lap();
    if (total) {
        // stage 4
        a.out_adj = t->d_adj;
        int rc = run_pass(a, rows.get(), count, batches, ws.get(), tab_off.get(), 1); if (rc) return rc;
        unsigned h_err[2] = {0, 0};
        HIPCHK(hipMemcpy(h_err, err.get(), sizeof h_err, hipMemcpyDeviceToHost));
        if (h_err[0] || h_err[1]) return BVG_E_HIP;
    }
    HIPCHK(hipDeviceSynchronize());
    if (dbgt) fprintf(stderr, "[bvg] compose: bounds + read back %.3f ms, tier lists + tables %.3f ms, symbolic pass + scan %.3f ms, result allocation %.3f ms, numeric pass %.3f ms\n",
                      ms_bound, ms_tiers, ms_symbolic, ms_alloc, sw.lap());
    if (report) *report = rep;
    out = std::move(t);
    return 0;
}

}  // namespace

// what bvg_lcompose.hip runs of the above as it is (bvg_compose_shared.h)
void compose_launch_bounds(const ComposeArgs& a, uint64_t* ub) { hipLaunchKernelGGL(compose_bound_kernel, dim3(grid(a.n, 256)), dim3(256), 0, 0, a, ub); }
int compose_symbolic_pass(const ComposeArgs& a, const uint32_t* d_rows, const uint64_t count[3], const std::vector<Tier2Batch>& batches, unsigned long long* ws, const uint64_t* d_tab_off) {
    return run_pass(a, d_rows, count, batches, ws, d_tab_off, 0);
}

}  // namespace bvghost

extern "C" int bvg_compose(const bvg_transform_src* g0, const bvg_transform_src* g1, bvg_compose_report* report, bvg_text** out) {
    if (!out || !one_source(g0) || !one_source(g1)) return BVG_E_ARG;
    if (source_device(g0) != source_device(g1)) return BVG_E_ARG;
    return guarded([&]() -> int {
        Source s0, s1;
        int rc = resolve(g0, s0); if (rc) return rc;
        const bool same = g0->graph == g1->graph && g0->csr == g1->csr;       // g o g: resolved once
        if (!same) { rc = resolve(g1, s1); if (rc) return rc; }
        std::unique_ptr<bvg_text> t;
        rc = compose_csr(s0, same ? s0 : s1, report, t);
        if (hipDeviceSynchronize() != hipSuccess && !rc) { (void)hipGetLastError(); rc = BVG_E_HIP; }
        if (rc) return rc;
        return finish(t, out);
    });
}
