// bvg_compose_shared.h — what the two graph products share: bvg_compose.hip (the Boolean product) and bvg_lcompose.hip (the product
// over a semiring, 7m).  The constants, the hash table's insert, the workgroup's sort, the dealing of the rows to the tiers and of tier 2's rows to
// batches, and the two stages of bvg_compose.hip that the labelled product runs as they are: the bounds and the symbolic pass.  Internal.
#pragma once
#include <cstdint>
#include <vector>

#include "bvg_host.h"

namespace bvghost {

struct ComposeArgs {
    const uint64_t* off0; const int64_t* adj0; int64_t n0;
    const uint64_t* off1; const int64_t* adj1; int64_t n1;
    int64_t n;
    const uint64_t* ub;              // [n]
    int32_t* cnt;                    // [n] the rows' lengths (symbolic pass)
    const uint64_t* out_off; int64_t* out_adj;   // the result (numeric pass)
    unsigned* err;                   // [0] a probe cap was hit, [1] a row's two passes disagree
};

struct Tier2Batch { uint32_t lo, hi; uint64_t slots; };   // rows [lo, hi) of tier 2's list, and the slots of their tables together

// ---- bvg_compose.hip: stage 1 (ub[x] for every row, a.ub is not read) and stage 3 (the symbolic pass over the three tiers' lists: a.cnt[x] = the
// row's length).  The lists may come from limits below bvg_compose's own (a row is only ever sent to a tier whose table holds it); tier 2's tables
// are 8-byte slots at ws + d_tab_off[r], cleared here.
void compose_launch_bounds(const ComposeArgs& a, uint64_t* ub);
int compose_symbolic_pass(const ComposeArgs& a, const uint32_t* d_rows, const uint64_t count[3], const std::vector<Tier2Batch>& batches, unsigned long long* ws, const uint64_t* d_tab_off);

namespace {

constexpr uint64_t kMaxElems = 0x7FFFFFFFull;      // what one prefix sum (launch_exclusive_scan) takes
constexpr unsigned long long kEmpty = ~0ull;       // no node id: a slot without a key, and the key that sorts behind every node
constexpr uint32_t kSlots0 = 512, kSlots1 = 8192;  // keys of an LDS table: 4 KiB per wavefront, 64 KiB per workgroup
constexpr uint64_t kLimit0 = kSlots0 / 2, kLimit1 = kSlots1 / 2;
constexpr int kThreads0 = 64, kThreads1 = 512, kThreads2 = 512;
constexpr uint32_t kMinSlots = 64;                 // of an LDS table
constexpr uint64_t kDefaultBudget = 256ull << 20;  // bytes of tier 2's workspace
constexpr unsigned kMaxGrid = 1u << 16;            // workgroups of a launch; each strides over its rows

__host__ __device__ __forceinline__ uint64_t pow2ceil(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }
__host__ __device__ __forceinline__ uint64_t table_slots2(uint64_t ub, int64_t n) { return 2 * pow2ceil(ub < (uint64_t)n ? ub : (uint64_t)n); }   // tier 2

// ---- the table.  1: z is new, 0: it was there (or the cap was hit: flagged)
__device__ __forceinline__ int table_insert(unsigned long long* tab, uint64_t mask, unsigned bits, unsigned long long z, unsigned* err) {
    uint64_t i = ((z * 0x9E3779B97F4A7C15ull) >> (64u - bits)) & mask;       // multiplicative: the high bits depend on every bit of z
    for (uint64_t step = 0; step <= mask; step++, i = (i + 1) & mask) {
        const unsigned long long old = atomicCAS(&tab[i], kEmpty, z);
        if (old == kEmpty) return 1;
        if (old == z) return 0;
    }
    atomicOr(err, 1u);
    return 0;
}

// a[0, len) ascending, by the whole workgroup: the bitonic network whose every comparison puts the smaller key at the lower index
// (a flip, then halving strides), so positions at and beyond len stand for keys above all others and are never touched
template <int THREADS> __device__ __forceinline__ void group_sort(unsigned long long* a, uint64_t len) {
    const uint64_t p = pow2ceil(len);
    for (uint64_t k = 2; k <= p; k <<= 1) {
        for (uint64_t j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (uint64_t t = threadIdx.x; t < (p >> 1); t += THREADS) {
                const uint64_t lo = (t / j) * (j << 1) + (t % j);
                const uint64_t hi = flip ? ((lo & ~(k - 1)) | ((k - 1) - (lo & (k - 1)))) : lo + j;
                if (hi < len) {
                    const unsigned long long u = a[lo], v = a[hi];
                    if (u > v) { a[lo] = v; a[hi] = u; }
                }
            }
            __syncthreads();
        }
    }
}

uint64_t knob_u64(const char* name, uint64_t dflt) { const char* v = knob(name); return v && *v ? strtoull(v, nullptr, 10) : dflt; }

// ---- stage 2, on the host: the rows with a bound > 0 dealt to the tiers by their bounds (`forced`: no row below that tier), tier 0's, tier 1's and
// tier 2's rows one after another in `rows`; tier 2's batches: tables side by side in the workspace, as many rows as `cap` slots hold (a row whose
// table alone exceeds it: a batch of its own); tab[i] = where in its batch's workspace the table of tier 2's row i begins, in slots
struct TierPlan {
    uint64_t products = 0, count[3] = {0, 0, 0}, ws_slots = 0;
    std::vector<uint32_t> rows; std::vector<uint64_t> tab; std::vector<Tier2Batch> batches;
};
void plan_tiers(const std::vector<uint64_t>& h_ub, int64_t n, uint64_t limit0, uint64_t limit1, int forced, uint64_t cap, TierPlan& p) {
    uint64_t* count = p.count;
    auto tier_of = [&](uint64_t u) { int tr = u <= limit0 ? 0 : u <= limit1 ? 1 : 2; return forced > tr ? forced : tr; };
    for (int64_t x = 0; x < n; x++) if (h_ub[(size_t)x]) { p.products += h_ub[(size_t)x]; count[tier_of(h_ub[(size_t)x])]++; }
    std::vector<uint32_t>& h_rows = p.rows;
    h_rows.resize((size_t)(count[0] + count[1] + count[2]));
    uint64_t at[3] = {0, count[0], count[0] + count[1]};
    for (int64_t x = 0; x < n; x++) if (h_ub[(size_t)x]) h_rows[(size_t)at[tier_of(h_ub[(size_t)x])]++] = (uint32_t)x;
    if (count[2]) {
        std::vector<uint64_t>& h_tab = p.tab;
        h_tab.resize((size_t)count[2]);
        const uint32_t* r2 = h_rows.data() + count[0] + count[1];
        Tier2Batch b{0, 0, 0};
        for (uint32_t i = 0; i < (uint32_t)count[2]; i++) {
            const uint64_t slots = table_slots2(h_ub[r2[i]], n);
            if (b.hi > b.lo && b.slots + slots > cap) { p.batches.push_back(b); b = Tier2Batch{i, i, 0}; }
            h_tab[i] = b.slots; b.slots += slots; b.hi = i + 1;
        }
        p.batches.push_back(b);
        for (const Tier2Batch& q : p.batches) if (q.slots > p.ws_slots) p.ws_slots = q.slots;
    }
}

}  // namespace
}  // namespace bvghost
