// bvg_lcompose.hip — Transform.compose(ArcLabelledImmutableGraph, ArcLabelledImmutableGraph, LabelSemiring) on the device (Transform.java:1792-1918):
// the sparse matrix product of two arc-labelled graphs over a semiring, from two labelled CSRs in HBM to a labelled CSR in HBM.  The contract is
// the one of include/bvgraph_hip.h ("Labelled compose"); DESIGN.md 7m has the reasons.
//
// The architecture is bvg_compose.hip's, and three of its four stages ARE bvg_compose.hip's: the bound per row, the tiers and
// batches dealt on the host (bvg_compose_shared.h: plan_tiers, with this file's limits) and the symbolic pass over the sources' CSRs, which gives
// every row's length and so the result's offsets -- the structure of the result is the unlabelled product's.  What is new is the numeric pass:
//   a slot is 16 bytes, a key and a 64-bit value (two arrays: keys[slots], values[slots]).  The owner of the row -- one wavefront (tier 0, LDS),
//   one workgroup (tier 1, LDS), one workgroup with its table in the bounded HBM workspace (tier 2) -- clears both arrays before the barrier that
//   precedes the first insert: keys to all-ones, values to the zero of the semiring's add among non-negative integers (all-ones for min,
//   all-zeros for max and +; tier 2: hipMemsetAsync before the launch).  A product (x -> y labelled a, y -> z labelled b) finds or claims the slot
//   of z by compare-and-swap exactly as the unlabelled insert does and then applies add to the slot's value with ONE atomic (64-bit unsigned
//   min, max or add) of a (x) b.  Every key that exists has received at least one product, so a slot's initial value never reaches the result.
//   After the barrier that follows the last insert every value is FINALISED to its int32: the range check against the result's class, the count
//   of arcs out of range and the atomicMin of (row << 32 | successor) over them.  A node is below 2^31 and a finalised label is below 2^31, so
//   key << 32 | label is one 64-bit word whose order is the key's: the packed words are moved to the front of the table (LDS tiers) or laid in
//   the row's own place in adj (tier 2, where every claimed slot was listed as it was claimed, as bvg_compose lists the new keys, so that nothing
//   scans a table of up to 2^20 slots), sorted by bvg_compose's bitonic network unchanged, and split into adj and labels.
// No wavefront waits on another workgroup; every probe loop is capped at the table size (flag -> BVG_E_HIP); every index is masked.
#include <cstdint>

#include "bvg_host.h"
#include "bvg_compose_shared.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

// a slot is 16 bytes: tier 0 keeps bvg_compose's 512 slots (8 KiB a wavefront), tier 1 its 64 KiB (4 096 slots): DESIGN.md 7m
constexpr uint32_t kLSlots0 = 512, kLSlots1 = 4096;
constexpr uint64_t kLLimit0 = kLSlots0 / 2, kLLimit1 = kLSlots1 / 2;
static_assert(kLLimit0 <= kLimit0 && kLLimit1 <= kLimit1, "the symbolic pass of bvg_compose.hip runs over this file's tier lists");
constexpr unsigned long long kClamp = 1ull << 32;  // of a PLUS_TIMES product: above every label in range, and 2^31 of them stay below 2^63
constexpr uint64_t kNoSlot = ~0ull;
constexpr uint64_t kLDefaultBudget = 2 * kDefaultBudget;   // bytes of tier 2's workspace: as many SLOTS as bvg_compose's, so as many rows a batch

struct LabelArgs {
    const int32_t* lab0; const int32_t* lab1;   // the sources' labels, in successor order
    int32_t* out_lab;                           // the result's
    int semiring;
    unsigned long long max_label;               // the largest label of the result's class
    unsigned long long* range;                  // [0] arcs out of range, [1] the smallest row << 32 | successor among them (all-ones: none)
};

__device__ __forceinline__ bool add_is_min(int s) { return s == BVG_SEMIRING_MIN_PLUS || s == BVG_SEMIRING_MIN_MAX; }
// a (x) b, exact: labels are below 2^31
__device__ __forceinline__ unsigned long long multiply(int s, unsigned long long a, unsigned long long b) {
    if (s == BVG_SEMIRING_MIN_PLUS || s == BVG_SEMIRING_MAX_PLUS) return a + b;
    if (s == BVG_SEMIRING_MAX_MIN) return a < b ? a : b;
    if (s == BVG_SEMIRING_MIN_MAX) return a > b ? a : b;
    const unsigned long long p = a * b;
    return p > kClamp ? kClamp : p;
}
// a word of tier 2's table as the atomics on it left it: read where they act (L2), not through a line this CU may hold
__device__ __forceinline__ unsigned long long peek(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void accumulate(int s, unsigned long long* v, unsigned long long p) {
    if (add_is_min(s)) atomicMin(v, p);
    else if (s == BVG_SEMIRING_PLUS_TIMES) atomicAdd(v, p);
    else atomicMax(v, p);
}

// the slot of z, claimed when z is new (*fresh = 1); kNoSlot when the cap was hit (flagged).  table_insert's probe sequence.
__device__ __forceinline__ uint64_t table_slot(unsigned long long* tab, uint64_t mask, unsigned bits, unsigned long long z, unsigned* err, unsigned* fresh) {
    uint64_t i = ((z * 0x9E3779B97F4A7C15ull) >> (64u - bits)) & mask;
    for (uint64_t step = 0; step <= mask; step++, i = (i + 1) & mask) {
        const unsigned long long old = atomicCAS(&tab[i], kEmpty, z);
        if (old == kEmpty) { *fresh = 1; return i; }
        if (old == z) { *fresh = 0; return i; }
    }
    atomicOr(err, 1u);
    *fresh = 0;
    return kNoSlot;
}

// what a thread has seen out of range
struct Range { unsigned long long count = 0, first = ~0ull; };
// key << 32 | label of a finished slot of row x
__device__ __forceinline__ unsigned long long finalise(const LabelArgs& l, int64_t x, unsigned long long key, unsigned long long v, Range& r) {
    if (v > l.max_label) {
        r.count++;
        const unsigned long long at = ((unsigned long long)x << 32) | key;
        if (at < r.first) r.first = at;
    }
    return (key << 32) | (v & 0x7FFFFFFFull);
}

// ---- the numeric pass: the rows of one tier's list, one workgroup a row.  GLOBAL: the keys lie in `ws` at tab_off[r], the values ws_vals words behind them.
template <int THREADS, uint32_t SLOTS, bool GLOBAL>
__global__ void __launch_bounds__(THREADS) lcompose_rows_kernel(ComposeArgs a, LabelArgs l, const uint32_t* rows, uint32_t nrows, unsigned long long* ws, uint64_t ws_vals, const uint64_t* tab_off) {
    __shared__ unsigned long long lds_key[GLOBAL ? 1 : SLOTS];
    __shared__ unsigned long long lds_val[GLOBAL ? 1 : SLOTS];
    __shared__ unsigned fresh;                                                 // new keys of the row so far; then the words dealt so far
    constexpr int WAVES = THREADS / 64;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long zero = add_is_min(l.semiring) ? ~0ull : 0ull;
    Range range;
    for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int64_t x = (int64_t)rows[r];
        const uint64_t ub = a.ub[x];
        uint64_t slots;
        unsigned long long *tab, *val;
        if (GLOBAL) { slots = table_slots2(ub, a.n); tab = ws + tab_off[r]; val = tab + ws_vals; }   // cleared by the host before the launch
        else {
            slots = 2 * pow2ceil(ub); if (slots < kMinSlots) slots = kMinSlots; if (slots > SLOTS) slots = SLOTS;   // (the host sends no row with 2 ub > SLOTS here)
            tab = lds_key; val = lds_val;
            for (uint32_t i = threadIdx.x; i < (uint32_t)slots; i += THREADS) { tab[i] = kEmpty; val[i] = zero; }
        }
        if (threadIdx.x == 0) fresh = 0;
        __syncthreads();
        const uint64_t mask = slots - 1;
        const unsigned bits = 63u - (unsigned)__clzll((long long)slots);
        const uint64_t row_lo = a.out_off[x], row_len = a.out_off[x + 1] - row_lo;
        // a wavefront takes 64 successors y of x at a time, one per lane, then the lists N1(y) one after another, 64 products a step
        const uint64_t lo = a.off0[x], hi = a.off0[x + 1];
        unsigned mine = 0;
        for (uint64_t base = lo + (uint64_t)wave * 64; base < hi; base += (uint64_t)WAVES * 64) {
            const uint64_t idx = base + lane;
            const int64_t y = idx < hi ? a.adj0[idx] : -1;
            const bool in = y >= 0 && y < a.n1;                                // a successor g1 does not have contributes nothing
            const uint64_t s = in ? a.off1[y] : 0, len = in ? a.off1[y + 1] - s : 0;
            const uint32_t la = in ? (uint32_t)l.lab0[idx] : 0u;
            unsigned long long live = __ballot(len != 0);
            while (live) {
                const int j = __ffsll((long long)live) - 1;
                live &= live - 1;
                const uint64_t sj = __shfl(s, j, 64), lj = __shfl(len, j, 64);
                const unsigned long long aj = __shfl(la, j, 64);
                for (uint64_t k = lane; k < lj; k += 64) {
                    const unsigned long long z = (unsigned long long)a.adj1[sj + k];
                    const unsigned long long p = multiply(l.semiring, aj, (unsigned long long)(uint32_t)l.lab1[sj + k]);
                    unsigned isnew;
                    const uint64_t at = table_slot(tab, mask, bits, z, a.err, &isnew);
                    if (at != kNoSlot) {
                        if (GLOBAL && isnew) {                                 // tier 2: the claimed slots are listed in the row's place in adj, as bvg_compose lists the keys
                            const uint64_t pos = atomicAdd(&fresh, 1u);
                            if (pos < row_len) a.out_adj[row_lo + pos] = (int64_t)at;
                        } else mine += isnew;
                        accumulate(l.semiring, &val[at & mask], p);
                    }
                }
            }
        }
        for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0 && mine) atomicAdd(&fresh, mine);
        __syncthreads();                                                       // every insert and every accumulation of the row is done
        if (threadIdx.x == 0 && fresh != row_len) atomicOr(a.err + 1, 1u);
        if (GLOBAL) {
            // every listed slot is replaced by its packed word (the thread that reads position i writes it), and the words are sorted where they lie.
            // The table was written by atomics, which act in L2: it is read there, not through a line this CU may hold
            unsigned long long* out = (unsigned long long*)(a.out_adj + row_lo);
            for (uint64_t i = threadIdx.x; i < row_len; i += THREADS) {
                const uint64_t at = out[i] & mask;
                out[i] = finalise(l, x, peek(&tab[at]), peek(&val[at]), range);
            }
            __syncthreads();
            group_sort<THREADS>(out, row_len);
            // every thread splits the words it reads itself: the word at i is read before adj[i], which lies over it, is written
            for (uint64_t i = threadIdx.x; i < row_len; i += THREADS) {
                const unsigned long long w = out[i];
                a.out_adj[row_lo + i] = (int64_t)(w >> 32);
                l.out_lab[row_lo + i] = (int32_t)(uint32_t)w;
            }
        } else {
            // the finished slots to the front of the key array, as packed words in any order: every thread takes its slots into registers and, all
            // slots read, the words go where an LDS counter deals them.  Then the sort is over the row, not the table.
            constexpr int PER = SLOTS / THREADS > 0 ? SLOTS / THREADS : 1;
            unsigned long long keep[PER];
#pragma unroll
            for (int q = 0; q < PER; q++) {
                const uint32_t i = (uint32_t)q * THREADS + threadIdx.x;
                const unsigned long long key = i < slots ? tab[i] : kEmpty;
                keep[q] = key != kEmpty ? finalise(l, x, key, val[i], range) : kEmpty;
            }
            if (threadIdx.x == 0) fresh = 0;                                   // (thread 0 has compared it with the row's length above)
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
            for (uint64_t i = threadIdx.x; i < len; i += THREADS) {
                const unsigned long long w = tab[i];
                a.out_adj[row_lo + i] = (int64_t)(w >> 32);
                l.out_lab[row_lo + i] = (int32_t)(uint32_t)w;
            }
        }
        __syncthreads();                                                       // the table and `fresh` are the next row's
    }
    // what this thread saw out of range, over all its rows
    unsigned long long c = range.count;
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0 && c) atomicAdd(&l.range[0], c);
    if (range.first != ~0ull) atomicMin(&l.range[1], range.first);
}

int numeric_pass(const ComposeArgs& a, const LabelArgs& l, const uint32_t* d_rows, const uint64_t count[3], const std::vector<Tier2Batch>& batches, unsigned long long* ws, uint64_t ws_vals, const uint64_t* d_tab_off) {
    auto blocks = [](uint64_t rows) { return dim3((unsigned)(rows < kMaxGrid ? rows : kMaxGrid)); };
    if (count[0]) hipLaunchKernelGGL((lcompose_rows_kernel<kThreads0, kLSlots0, false>), blocks(count[0]), dim3(kThreads0), 0, 0, a, l, d_rows, (uint32_t)count[0], nullptr, 0, nullptr);
    if (count[1]) hipLaunchKernelGGL((lcompose_rows_kernel<kThreads1, kLSlots1, false>), blocks(count[1]), dim3(kThreads1), 0, 0, a, l, d_rows + count[0], (uint32_t)count[1], nullptr, 0, nullptr);
    const uint32_t* rows2 = d_rows + count[0] + count[1];
    const bool ones = l.semiring == BVG_SEMIRING_MIN_PLUS || l.semiring == BVG_SEMIRING_MIN_MAX;   // the values' zero is the keys' pattern
    for (const Tier2Batch& b : batches) {
        HIPCHK(hipMemsetAsync(ws, 0xFF, (size_t)b.slots * sizeof(unsigned long long), 0));
        HIPCHK(hipMemsetAsync(ws + ws_vals, ones ? 0xFF : 0x00, (size_t)b.slots * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL((lcompose_rows_kernel<kThreads2, 1, true>), blocks(b.hi - b.lo), dim3(kThreads2), 0, 0, a, l, rows2 + b.lo, b.hi - b.lo, ws, ws_vals, d_tab_off + b.lo);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int lcompose(const bvg_lgraph* l0, const bvg_lgraph* l1, int semiring, int out_width, bvg_lcompose_report* report, std::unique_ptr<bvg_lgraph>& out) {
    const bvg_text *g0 = l0->g.get(), *g1 = l1->g.get();
    const int64_t n = g0->nodes > g1->nodes ? g0->nodes : g1->nodes;
    if ((uint64_t)n > kMaxElems || g0->arcs > kMaxElems || g1->arcs > kMaxElems) return BVG_E_UNSUPPORTED;
    int forced = -1;
    if (const char* v = knob("BVG_COMPOSE_TIER")) if (*v >= '0' && *v <= '2' && !v[1]) forced = *v - '0';
    const uint64_t budget = knob_u64("BVG_COMPOSE_WS", kLDefaultBudget);
    uint64_t max_arcs = knob_u64("BVG_COMPOSE_MAX_ARCS", kMaxElems);
    if (max_arcs > kMaxElems) max_arcs = kMaxElems;

    bvg_lcompose_report rep{};
    rep.limit[0] = kLLimit0; rep.limit[1] = kLLimit1; rep.first_row = rep.first_successor = -1;
    std::unique_ptr<bvg_lgraph> t(new bvg_lgraph);
    t->g = new_csr(g0->device); t->kind = l0->kind; t->width = l0->kind == BVG_LABEL_FIXED_INT && out_width >= 0 ? out_width : l0->width;
    t->g->nodes = n;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    DevArray<uint64_t> ub, tmp, tab_off; DevArray<int32_t> cnt; DevArray<uint32_t> rows; DevArray<unsigned> err; DevArray<unsigned long long> ws, range;
    if (t->g->d_off.alloc(nn + 1) || ub.alloc(nn) || cnt.alloc(nn) || rows.alloc(nn) || tmp.alloc(scan_tmp_elems((int64_t)nn)) || err.alloc(2) || range.alloc(2)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(t->g->d_off.get(), 0, (nn + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemset(cnt.get(), 0, nn * sizeof(int32_t)));
    HIPCHK(hipMemset(err.get(), 0, 2 * sizeof(unsigned)));
    const unsigned long long h_range0[2] = {0ull, ~0ull};
    HIPCHK(hipMemcpy(range.get(), h_range0, sizeof h_range0, hipMemcpyHostToDevice));
    ComposeArgs a{g0->d_off.get(), g0->d_adj, g0->nodes, g1->d_off.get(), g1->d_adj, g1->nodes, n, ub.get(), cnt.get(), t->g->d_off.get(), nullptr, err.get()};

    TierPlan plan;
    uint64_t total = 0, ws_vals = 0;
    const bool dbgt = dbg_on();                                         // BVG_DEBUG: the wall clock of every stage (a synchronisation each)
    Stopwatch sw; double ms_bound = 0, ms_tiers = 0, ms_symbolic = 0, ms_alloc = 0;
    if (n > 0) {
        // stages 1 to 3 are bvg_compose's, over this file's limits and a budget counted in 16-byte slots
        compose_launch_bounds(a, ub.get());
        std::vector<uint64_t> h_ub((size_t)n);
        HIPCHK(hipMemcpy(h_ub.data(), ub.get(), (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (dbgt) ms_bound = sw.lap();
        plan_tiers(h_ub, n, kLLimit0, kLLimit1, forced, budget / (2 * sizeof(unsigned long long)), plan);
        rep.products = plan.products;
        for (int i = 0; i < 3; i++) rep.rows[i] = plan.count[i];
        rep.batches = plan.batches.size();
        if (!plan.rows.empty()) HIPCHK(hipMemcpy(rows.get(), plan.rows.data(), plan.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (plan.count[2]) {
            ws_vals = plan.ws_slots;                                        // keys[ws_slots], then values[ws_slots]
            if (ws.alloc((size_t)(2 * plan.ws_slots)) || tab_off.alloc((size_t)plan.count[2])) return BVG_E_NOMEM;
            HIPCHK(hipMemcpy(tab_off.get(), plan.tab.data(), plan.tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
        if (dbgt) ms_tiers = sw.lap();
        int rc = compose_symbolic_pass(a, rows.get(), plan.count, plan.batches, ws.get(), tab_off.get()); if (rc) return rc;
        launch_exclusive_scan(cnt.get(), t->g->d_off.get(), n, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&total, t->g->d_off.get() + n, sizeof total, hipMemcpyDeviceToHost));
        unsigned h_err[2] = {0, 0};
        HIPCHK(hipMemcpy(h_err, err.get(), sizeof h_err, hipMemcpyDeviceToHost));
        if (h_err[0]) return BVG_E_HIP;
        if (dbgt) ms_symbolic = sw.lap();
    }
    rep.arcs = total;
    if (total > max_arcs) { if (report) *report = rep; return BVG_E_UNSUPPORTED; }
    if (t->g->adj_base.alloc((size_t)total) || t->d_lab.alloc((size_t)total)) return BVG_E_NOMEM;
    t->g->d_adj = t->g->adj_base; t->g->arcs = total;
    if (dbgt) ms_alloc = sw.lap();
    if (total) {
        a.out_adj = t->g->d_adj;
        const unsigned long long max_label = t->kind == BVG_LABEL_GAMMA_INT ? 0x7FFFFFFFull : (1ull << t->width) - 1;
        const LabelArgs l{l0->d_lab.get(), l1->d_lab.get(), t->d_lab.get(), semiring, max_label, range.get()};
        int rc = numeric_pass(a, l, rows.get(), plan.count, plan.batches, ws.get(), ws_vals, tab_off.get()); if (rc) return rc;
        unsigned h_err[2] = {0, 0};
        HIPCHK(hipMemcpy(h_err, err.get(), sizeof h_err, hipMemcpyDeviceToHost));
        if (h_err[0] || h_err[1]) return BVG_E_HIP;
        unsigned long long h_range[2] = {0, 0};
        HIPCHK(hipMemcpy(h_range, range.get(), sizeof h_range, hipMemcpyDeviceToHost));
        if (h_range[0]) {
            rep.out_of_range = h_range[0]; rep.first_row = (int64_t)(h_range[1] >> 32); rep.first_successor = (int64_t)(h_range[1] & 0xFFFFFFFFull);
            if (report) *report = rep;
            return BVG_E_ARG;
        }
    }
    HIPCHK(hipDeviceSynchronize());
    if (dbgt) fprintf(stderr, "[bvg] lcompose: bounds + read back %.3f ms, tier lists + tables %.3f ms, symbolic pass + scan %.3f ms, result allocation %.3f ms, numeric pass %.3f ms\n",
                      ms_bound, ms_tiers, ms_symbolic, ms_alloc, sw.lap());
    if (report) *report = rep;
    out = std::move(t);
    return 0;
}

}  // namespace
}  // namespace bvghost

extern "C" int bvg_lcompose(const bvg_lgraph* g0, const bvg_lgraph* g1, int semiring, int out_width, bvg_lcompose_report* report, bvg_lgraph** out) {
    if (!out || !g0 || !g1 || semiring < BVG_SEMIRING_MIN_PLUS || semiring > BVG_SEMIRING_PLUS_TIMES || out_width < -1 || out_width > 31) return BVG_E_ARG;
    if (g0->kind != g1->kind || g0->width != g1->width || g0->g->device != g1->g->device) return BVG_E_ARG;
    if (g0->kind == BVG_LABEL_FIXED_INT_LIST || g0->kind == BVG_LABEL_FIXED_LONG_LIST) return BVG_E_UNSUPPORTED;
    if (g0->kind != BVG_LABEL_GAMMA_INT && g0->kind != BVG_LABEL_FIXED_INT) return BVG_E_ARG;
    if (g0->kind == BVG_LABEL_GAMMA_INT && out_width != -1) return BVG_E_ARG;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(g0->g->device));
        std::unique_ptr<bvg_lgraph> t;
        int rc = lcompose(g0, g1, semiring, out_width, report, t);
        if (hipDeviceSynchronize() != hipSuccess && !rc) { (void)hipGetLastError(); rc = BVG_E_HIP; }
        if (rc) return rc;
        *out = t.release();
        return 0;
    });
}
