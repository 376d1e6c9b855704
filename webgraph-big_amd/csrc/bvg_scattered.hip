// bvg_scattered.hip — scattered arc lists on the device (ScatteredArcsASCIIGraph.java): arc lists whose identifiers are arbitrary 64-bit
// numbers.  Every newly seen identifier gets the next node number, offending lines are counted and skipped.  The contract -- tokens,
// identifiers, what a line registers, the categories, the report -- is the one of include/bvgraph_hip.h ("scattered arc lists").
//
// "Number the identifiers in order of first appearance" without a serial pass:
//   S1  CLASSIFY.  The tiles, the line events and the comment state of bvg_text.hip (bvg_text_shared.h), with the lenient token rule: a
//       token starts at a byte above 32 whose predecessor is not.  Two passes (count; prefix sums over the tiles; write): one lane per
//       token start reads the identifier from global memory -> vals[token], meta[token] = byte offset << 4 | what is wrong with it; every
//       break writes tb[line].  Then one lane per line looks at the line's first two tokens: what the line registers (0, 1 or 2
//       OCCURRENCES) and whether it holds an arc; whatever offends goes into the one 64-bit minimum (offset << 4 | reason).  Prefix sums
//       over the lines place the occurrences (identifier, byte offset of its token) and the arcs in text order.
//   S2  INSERT.  An open-addressing table in HBM of {key, first offset} slots: the key is claimed with a 64-bit compare-and-swap, the
//       offset lowered with a 64-bit minimum.  The byte offset of a token is its order of appearance, so the minimum per key is the first
//       appearance whatever the lanes' order.  A hub identifier must not serialise its occurrences on one address: the slot's offset is read
//       before the atomic, which is skipped when it is not above the lane's (the value only falls; 2.4 x on a text with a hub on a
//       quarter of its lines, DESIGN.md 7n -- skipping lanes whose left neighbour holds the same identifier gained nothing on top and
//       is not done).  The identifier equal to the empty marker lives in a word of its own.  Every probe loop ends after `slots` steps and raises a flag (BVG_E_STATE): it never spins.
//   S3  NUMBER.  The occupied slots are collected (one atomic per wavefront) and the distinct (first offset, slot) pairs sorted by offset
//       (rocPRIM): position = node number.  ids[node] = the slot's key, and the node number replaces the offset in the slot.
//   S4  LOOK UP.  One lane per arc probes for both ends and writes (source, target) in place of the identifiers; a dropped loop becomes
//       the (nodes, nodes) pair that pairs_to_csr (bvg_text.hip) drops, BVG_TEXT_SYMMETRIZE adds the reverse pair.  pairs_to_csr does the rest.
// GIVEN NUMBERING: S2 / S3 become "insert known_ids[i] with value i" (a claim that fails on an equal key is the duplicate), and a miss in S4
// is UNKNOWN_SOURCE / UNKNOWN_TARGET.
#include <cstdint>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "bvg_host.h"
#include "bvg_text_shared.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

enum : unsigned { kTokOk = 0, kTokBad = 1, kTokBig = 2 };            // what is wrong with a token
constexpr unsigned long long kEmptyKey = ~0ull;                      // a slot without a key: the identifier -1 lives outside the table
constexpr unsigned long long kMiss = ~0ull;                          // no node number
constexpr uint64_t kMinSlots = 256;
constexpr uint64_t kMaxElems = 0x7FFFFFFFull;                        // what one prefix sum (launch_exclusive_scan) takes

// the scalars on the device
enum { kSErr = 0, kSBadSource, kSBadTarget, kSNoTarget, kSTooLarge, kSTrailing, kSUnknownSource, kSUnknownTarget, kSLoops,
       kSDistinct, kSSpecial, kSInternal, kSDuplicate, kSCollected, kSLine, kSCount };

struct ScatArgs {
    const uint8_t* text; uint64_t nbytes;
    const uint8_t* state_in;                              // comment state at the start of every tile
    int32_t* cnt_tok; int32_t* cnt_brk;                   // count pass out
    const uint64_t* tok_base; const uint64_t* brk_base;   // write pass in
    int64_t* vals; uint64_t* meta; uint64_t* tb;          // write pass out: vals[tokens], meta[tokens], tb[breaks]
};

// the identifier that starts at p, read from left to right: the first thing wrong decides
__device__ __forceinline__ unsigned parse_identifier(const uint8_t* text, uint64_t nbytes, uint64_t p, int64_t* out) {
    const bool neg = text[p] == '-';
    if (neg) p++;
    uint64_t m = 0; int sig = 0;
    for (; p < nbytes; p++) {
        const unsigned c = text[p];
        if (c <= 32) break;
        const unsigned d = c - '0';
        if (d >= 10u) return kTokBad;
        if (sig == 0 && d == 0) continue;                                  // leading zeros
        if (++sig > 19) return kTokBig;
        m = m * 10 + d;                                                    // 19 digits stay below 10^19 < 2^64
    }
    if (m > (neg ? 1ull << 63 : (1ull << 63) - 1)) return kTokBig;
    *out = (int64_t)(neg ? 0 - m : m);
    return kTokOk;
}

// S1, the count pass (WRITE = false) and the write pass (WRITE = true)
template <bool WRITE>
__global__ void __launch_bounds__(kThreads) scat_pass_kernel(ScatArgs a) {
    __shared__ uint32_t lds[kThreads];
    const uint64_t tile = blockIdx.x;
    const uint64_t base = tile * kTile + (uint64_t)threadIdx.x * kChunk;
    Chunk c; c.load(a.text, a.nbytes, base);
    const bool comment = lane_in_comment(c, a.state_in, tile, lds);
    // the lane's counts: tokens in the low half, breaks in the high half (a tile holds at most 2048 / 4096)
    uint32_t mine = 0;
    {
        unsigned prev = c.prev; bool com = comment;
#pragma unroll
        for (int i = 0; i < kChunk; i++) {
            const unsigned ch = c.b[i];
            if (i < c.len) {
                if (is_break(ch, prev)) { mine += 1u << 16; com = false; }
                else if (ch == '#' && (prev == '\r' || prev == '\n')) com = true;
                else if (!com && ch > 32 && prev <= 32) mine += 1;
            }
            prev = ch;
        }
    }
    const uint32_t incl = block_scan<true>(mine, lds);
    if (!WRITE) {
        if (threadIdx.x == kThreads - 1) { a.cnt_tok[tile] = (int32_t)(incl & 0xFFFFu); a.cnt_brk[tile] = (int32_t)(incl >> 16); }
        return;
    }
    uint64_t tok = a.tok_base[tile] + ((incl - mine) & 0xFFFFu), line = a.brk_base[tile] + ((incl - mine) >> 16);
    unsigned prev = c.prev; bool com = comment;
    for (int i = 0; i < c.len; i++) {
        const unsigned ch = c.b[i];
        const uint64_t p = base + (uint64_t)i;
        if (is_break(ch, prev)) { a.tb[line] = tok; line++; com = false; }
        else if (ch == '#' && (prev == '\r' || prev == '\n')) com = true;
        else if (!com && ch > 32 && prev <= 32) {
            int64_t v = 0;
            const unsigned why = parse_identifier(a.text, a.nbytes, p, &v);
            a.vals[tok] = v; a.meta[tok] = p << 4 | why;
            tok++;
        }
        prev = ch;
    }
}

// S1, the lines: line l holds the tokens [tb[l - 1], tb[l]) (tb[-1] = 0; the unterminated last line is l == nb and ends at ntok)
__global__ void scat_lines_kernel(const uint64_t* tb, uint64_t nb, uint64_t ntok, const uint64_t* meta, int32_t* nocc, int32_t* arcf, unsigned long long* s) {
    BVG_FOR(i, nb + 1) {
        const uint64_t l = (uint64_t)i;
        const uint64_t t0 = l ? tb[l - 1] : 0, cnt = (l < nb ? tb[l] : ntok) - t0;
        int32_t n = 0, arc = 0;
        if (cnt) {
            const uint64_t src = meta[t0];
            if (src & 15u) {
                const bool big = (src & 15u) == kTokBig;
                atomicAdd(s + (big ? kSTooLarge : kSBadSource), 1ull);
                report(s + kSErr, src >> 4, big ? BVG_SCATTERED_TOO_LARGE : BVG_SCATTERED_BAD_SOURCE);
            } else if (cnt == 1) {
                n = 1;
                atomicAdd(s + kSNoTarget, 1ull);
                report(s + kSErr, src >> 4, BVG_SCATTERED_NO_TARGET);
            } else {
                const uint64_t tgt = meta[t0 + 1];
                if (tgt & 15u) {
                    const bool big = (tgt & 15u) == kTokBig;
                    n = 1;
                    atomicAdd(s + (big ? kSTooLarge : kSBadTarget), 1ull);
                    report(s + kSErr, tgt >> 4, big ? BVG_SCATTERED_TOO_LARGE : BVG_SCATTERED_BAD_TARGET);
                } else {
                    n = 2; arc = 1;
                    if (cnt > 2) atomicAdd(s + kSTrailing, 1ull);
                }
            }
        }
        nocc[l] = n; arcf[l] = arc;
    }
}
// ... and their occurrences and arcs, in text order
__global__ void scat_occurrences_kernel(const uint64_t* tb, uint64_t nb, const int64_t* vals, const uint64_t* meta, const int32_t* nocc, const uint64_t* occ_base,
                                        const uint64_t* arc_base, unsigned long long* occ_id, uint64_t* occ_off, uint64_t* src, uint64_t* dst, uint32_t* arc_occ) {
    BVG_FOR(i, nb + 1) {
        const uint64_t l = (uint64_t)i;
        const int32_t n = nocc[l];
        if (!n) continue;
        const uint64_t t0 = l ? tb[l - 1] : 0, ob = occ_base[l];
        occ_id[ob] = (unsigned long long)vals[t0]; occ_off[ob] = meta[t0] >> 4;
        if (n == 2) {
            occ_id[ob + 1] = (unsigned long long)vals[t0 + 1]; occ_off[ob + 1] = meta[t0 + 1] >> 4;
            const uint64_t ab = arc_base[l];
            src[ab] = (uint64_t)vals[t0]; dst[ab] = (uint64_t)vals[t0 + 1]; arc_occ[ab] = (uint32_t)ob;
        }
    }
}

__device__ __forceinline__ uint64_t mix64(uint64_t k) {                   // (the finaliser of MurmurHash3)
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// the table: slot h = tab[2 h] (the key), tab[2 h + 1] (the first offset; after S3 the node number).  `slots` is a power of two.
// The slot of `id`, claimed when nobody has: its index, or `slots` when the probe ran out; *claimed: this call put the key there
__device__ __forceinline__ uint64_t claim_slot(unsigned long long* tab, uint64_t slots, unsigned long long id, bool* claimed) {
    uint64_t h = mix64(id) & (slots - 1);
    for (uint64_t probe = 0; probe < slots; probe++, h = (h + 1) & (slots - 1)) {
        unsigned long long k = tab[2 * h];
        if (k == kEmptyKey) {
            k = atomicCAS(tab + 2 * h, kEmptyKey, id);
            if (k == kEmptyKey) { *claimed = true; return h; }
        }
        if (k == id) return h;
    }
    return slots;
}
// the value in the slot of `id`, or kMiss
__device__ __forceinline__ unsigned long long find_value(const unsigned long long* tab, uint64_t slots, unsigned long long special, unsigned long long id) {
    if (id == kEmptyKey) return special;
    uint64_t h = mix64(id) & (slots - 1);
    for (uint64_t probe = 0; probe < slots; probe++, h = (h + 1) & (slots - 1)) {
        const unsigned long long k = tab[2 * h];
        if (k == id) return tab[2 * h + 1];
        if (k == kEmptyKey) return kMiss;
    }
    return kMiss;
}

// S2
__global__ void scat_insert_kernel(const unsigned long long* occ_id, const uint64_t* occ_off, uint64_t nocc, unsigned long long* tab, uint64_t slots, unsigned long long* s) {
    unsigned long long mine = 0;
    BVG_FOR(i, nocc) {
        const unsigned long long id = occ_id[i];
        unsigned long long* first = s + kSSpecial;
        if (id != kEmptyKey) {
            bool claimed = false;
            const uint64_t h = claim_slot(tab, slots, id, &claimed);
            if (h == slots) { s[kSInternal] = 1; continue; }
            mine += claimed;
            first = tab + 2 * h + 1;
        }
        const unsigned long long off = occ_off[i];
        if (*first > off) atomicMin(first, off);                           // the value only falls: nothing to do when it is there already
    }
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(s + kSDistinct, mine);
}
// given numbering: known[i] -> i
__global__ void scat_insert_known_kernel(const unsigned long long* known, uint64_t n, unsigned long long* tab, uint64_t slots, unsigned long long* s) {
    BVG_FOR(i, n) {
        const unsigned long long id = known[i];
        if (id == kEmptyKey) {
            if (atomicCAS(s + kSSpecial, kMiss, (unsigned long long)i) != kMiss) s[kSDuplicate] = 1;
            continue;
        }
        bool claimed = false;
        const uint64_t h = claim_slot(tab, slots, id, &claimed);
        if (h == slots) s[kSInternal] = 1;
        else if (claimed) tab[2 * h + 1] = (unsigned long long)i;
        else s[kSDuplicate] = 1;
    }
}

// S3: the occupied slots, (first offset, slot) each, in any order; the identifier outside the table is slot `slots`.  Every wavefront's
// lanes run the same number of steps (the loop variable is the wavefront's), so the ballot sees all of them.
__global__ void __launch_bounds__(256) scat_collect_kernel(const unsigned long long* tab, uint64_t slots, unsigned long long* s, uint64_t cap, uint64_t* key_out, uint64_t* slot_out) {
    const unsigned lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < slots; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t h = base + lane;
        const bool full = h < slots && tab[2 * h] != kEmptyKey;
        const uint64_t m = ballot(full);
        if (!m) continue;
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(s + kSCollected, (unsigned long long)__popcll(m));
        at = __shfl(at, 0, 64) + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
        if (full && at < cap) { key_out[at] = tab[2 * h + 1]; slot_out[at] = h; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && s[kSSpecial] != kMiss) {
        const unsigned long long at = atomicAdd(s + kSCollected, 1ull);
        if (at < cap) { key_out[at] = s[kSSpecial]; slot_out[at] = slots; }
    }
}
__global__ void scat_number_kernel(const uint64_t* slot_sorted, uint64_t nodes, unsigned long long* tab, uint64_t slots, unsigned long long* s, int64_t* ids) {
    BVG_FOR(r, nodes) {
        const uint64_t h = slot_sorted[r];
        if (h >= slots) { ids[r] = (int64_t)kEmptyKey; s[kSSpecial] = (unsigned long long)r; }
        else { ids[r] = (int64_t)tab[2 * h]; tab[2 * h + 1] = (unsigned long long)r; }
    }
}

// S4: the pairs' identifiers -> node numbers, in place; pair j came from the occurrences arc_occ[j] and arc_occ[j] + 1
__global__ void scat_lookup_kernel(uint64_t* src, uint64_t* dst, uint64_t np, bool sym, bool no_loops, bool given, uint64_t drop, const unsigned long long* tab, uint64_t slots,
                                   const uint32_t* arc_occ, const uint64_t* occ_off, unsigned long long* s) {
    const unsigned long long special = s[kSSpecial];
    BVG_FOR(i, np) {
        const uint64_t j = (uint64_t)i;
        unsigned long long a = find_value(tab, slots, special, src[j]), b = find_value(tab, slots, special, dst[j]);
        if (a == kMiss || b == kMiss) {
            if (!given) s[kSInternal] = 1;
            else if (a == kMiss) { atomicAdd(s + kSUnknownSource, 1ull); report(s + kSErr, occ_off[arc_occ[j]], BVG_SCATTERED_UNKNOWN_SOURCE); }
            else { atomicAdd(s + kSUnknownTarget, 1ull); report(s + kSErr, occ_off[(uint64_t)arc_occ[j] + 1], BVG_SCATTERED_UNKNOWN_TARGET); }
            a = b = drop;
        } else if (no_loops && a == b) {
            atomicAdd(s + kSLoops, 1ull);
            a = b = drop;
        }
        src[j] = a; dst[j] = b;
        if (sym) { src[j + np] = b; dst[j + np] = a; }
    }
}

unsigned bits_of(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 1u; }

uint64_t slots_for(uint64_t keys) {                                        // a power of two, load at most 0.75
    uint64_t slots = kMinSlots;
    while (slots - slots / 4 < keys) slots <<= 1;
    return slots;
}

// the wall clock of every stage on stderr (BVG_DEBUG): the device is drained first
struct StageClock {
    Stopwatch w; const bool on = dbg_on();
    void lap(const char* what) { if (on) { (void)hipDeviceSynchronize(); fprintf(stderr, "[bvg] scattered %-10s %9.3f ms\n", what, w.lap()); } }
};

int scattered_impl(const uint8_t* d_text, uint64_t nbytes, uint32_t flags, const unsigned long long* d_known, int64_t n_known, bool given, int device,
                   bvg_text** out, bvg_scattered_report* rep, bvg_text_error* err) {
    const uint64_t tiles = (nbytes + kTile - 1) / kTile, tl = tiles ? tiles : 1;
    if (tiles > kMaxElems) return BVG_E_UNSUPPORTED;                       // 8 TiB of text
    if (n_known > (1ll << 40)) return BVG_E_NOMEM;                         // (what pairs_to_csr would say of so many nodes)
    const bool sym = (flags & BVG_TEXT_SYMMETRIZE) != 0, nol = (flags & BVG_TEXT_NO_LOOPS) != 0, strict = (flags & BVG_TEXT_STRICT) != 0;
    StageClock clock;
    DevArray<unsigned long long> scal;
    if (scal.alloc(kSCount)) return BVG_E_NOMEM;
    unsigned long long* d_s = scal.get();
    unsigned long long h_s[kSCount] = {};
    h_s[kSErr] = kNoError; h_s[kSSpecial] = kMiss;
    HIPCHK(hipMemcpy(d_s, h_s, sizeof h_s, hipMemcpyHostToDevice));

    // ---- S1: tokens and breaks
    DevArray<uint64_t> occ_off, s0, d0; DevArray<unsigned long long> occ_id; DevArray<uint32_t> arc_occ;
    uint64_t nocc = 0, np0 = 0, nbrk = 0;
    {
        DevArray<uint8_t> ev, state; DevArray<int32_t> ctok, cbrk, lnocc, larc; DevArray<uint64_t> btok, bbrk, tmp, tb, meta, occ_base, arc_base; DevArray<int64_t> vals;
        if (ctok.alloc(tl) || cbrk.alloc(tl) || btok.alloc(tl + 1) || bbrk.alloc(tl + 1) || tmp.alloc(scan_tmp_elems((int64_t)tl)) || ev.alloc(tl) || state.alloc(tl)) return BVG_E_NOMEM;
        HIPCHK(hipMemset(btok.get(), 0, (tl + 1) * sizeof(uint64_t))); HIPCHK(hipMemset(bbrk.get(), 0, (tl + 1) * sizeof(uint64_t)));
        ScatArgs a{};
        a.text = d_text; a.nbytes = nbytes; a.state_in = state.get(); a.cnt_tok = ctok.get(); a.cnt_brk = cbrk.get(); a.tok_base = btok.get(); a.brk_base = bbrk.get();
        uint64_t ntok = 0;
        if (tiles) {
            hipLaunchKernelGGL(text_events_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, 0, d_text, nbytes, ev.get());
            hipLaunchKernelGGL(text_state_kernel, dim3(1), dim3(kThreads), 0, 0, ev.get(), tiles, state.get());
            hipLaunchKernelGGL((scat_pass_kernel<false>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
            launch_exclusive_scan(a.cnt_tok, btok.get(), (int64_t)tiles, tmp.get(), nullptr);
            launch_exclusive_scan(a.cnt_brk, bbrk.get(), (int64_t)tiles, tmp.get(), nullptr);
            HIPCHK(hipMemcpy(&ntok, btok.get() + tiles, sizeof ntok, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(&nbrk, bbrk.get() + tiles, sizeof nbrk, hipMemcpyDeviceToHost));
        }
        const uint64_t nl = nbrk + 1;                                      // the lines, the one behind the last break included
        if (nl > kMaxElems) return BVG_E_UNSUPPORTED;
        if (vals.alloc(ntok) || meta.alloc(ntok) || tb.alloc(nl)) return BVG_E_NOMEM;
        a.vals = vals.get(); a.meta = meta.get(); a.tb = tb.get();
        if (tiles) hipLaunchKernelGGL((scat_pass_kernel<true>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
        clock.lap("tokens");
        tmp.reset();
        if (lnocc.alloc(nl) || larc.alloc(nl) || occ_base.alloc(nl + 1) || arc_base.alloc(nl + 1) || tmp.alloc(scan_tmp_elems((int64_t)nl))) return BVG_E_NOMEM;
        hipLaunchKernelGGL(scat_lines_kernel, dim3(grid((int64_t)nl, 256)), dim3(256), 0, 0, tb.get(), nbrk, ntok, meta.get(), lnocc.get(), larc.get(), d_s);
        launch_exclusive_scan(lnocc.get(), occ_base.get(), (int64_t)nl, tmp.get(), nullptr);
        launch_exclusive_scan(larc.get(), arc_base.get(), (int64_t)nl, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&nocc, occ_base.get() + nl, sizeof nocc, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&np0, arc_base.get() + nl, sizeof np0, hipMemcpyDeviceToHost));
        const uint64_t np = sym ? 2 * np0 : np0;
        if (nocc > kMaxElems || np > kMaxElems) return BVG_E_UNSUPPORTED;  // (the prefix sum of pairs_to_csr takes fewer than 2^31 elements)
        if (occ_id.alloc(nocc) || occ_off.alloc(nocc) || s0.alloc(np) || d0.alloc(np) || arc_occ.alloc(np0)) return BVG_E_NOMEM;
        hipLaunchKernelGGL(scat_occurrences_kernel, dim3(grid((int64_t)nl, 256)), dim3(256), 0, 0, tb.get(), nbrk, vals.get(), meta.get(), lnocc.get(), occ_base.get(),
                           arc_base.get(), occ_id.get(), occ_off.get(), s0.get(), d0.get(), arc_occ.get());
        clock.lap("lines");
    }
    const uint64_t np = sym ? 2 * np0 : np0;

    // ---- S2, S3: the table and the node numbers
    std::unique_ptr<bvg_text> t(new bvg_text);
    t->device = device;
    int64_t nodes = 0;
    const uint64_t slots = slots_for(given ? (uint64_t)n_known : nocc);
    DevArray<unsigned long long> tab;
    if (tab.alloc(2 * slots)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(tab.get(), 0xFF, 2 * slots * sizeof(unsigned long long)));       // every key kEmptyKey, every offset above all others
    if (given) {
        nodes = n_known;
        if (t->ids.alloc((size_t)nodes)) return BVG_E_NOMEM;
        if (nodes) {
            HIPCHK(hipMemcpy(t->ids.get(), d_known, (size_t)nodes * sizeof(int64_t), hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(scat_insert_known_kernel, dim3(grid(nodes, 256)), dim3(256), 0, 0, d_known, (uint64_t)nodes, tab.get(), slots, d_s);
        }
        HIPCHK(hipMemcpy(h_s, d_s, sizeof h_s, hipMemcpyDeviceToHost));
        if (h_s[kSInternal]) return BVG_E_STATE;
        if (h_s[kSDuplicate]) return BVG_E_ARG;
        clock.lap("known ids");
    } else {
        if (nocc) hipLaunchKernelGGL(scat_insert_kernel, dim3(grid((int64_t)nocc, 256)), dim3(256), 0, 0, occ_id.get(), occ_off.get(), nocc, tab.get(), slots, d_s);
        HIPCHK(hipMemcpy(h_s, d_s, sizeof h_s, hipMemcpyDeviceToHost));
        if (h_s[kSInternal]) return BVG_E_STATE;
        clock.lap("insert");
        nodes = (int64_t)(h_s[kSDistinct] + (h_s[kSSpecial] != kMiss ? 1 : 0));
        if (t->ids.alloc((size_t)nodes)) return BVG_E_NOMEM;
        if (nodes) {
            const uint64_t n = (uint64_t)nodes;
            DevArray<uint64_t> k0, k1, v0, v1; DevArray<uint8_t> stmp;
            if (k0.alloc(n) || k1.alloc(n) || v0.alloc(n) || v1.alloc(n)) return BVG_E_NOMEM;
            const uint64_t wg = slots / 256 < (1u << 16) ? slots / 256 : (1u << 16);
            hipLaunchKernelGGL(scat_collect_kernel, dim3((unsigned)wg), dim3(256), 0, 0, tab.get(), slots, d_s, n, k0.get(), v0.get());
            size_t sb = 0;
            const unsigned bits = bits_of(nbytes);
            HIPCHK(rocprim::radix_sort_pairs(nullptr, sb, (const uint64_t*)k0.get(), k1.get(), (const uint64_t*)v0.get(), v1.get(), (size_t)n, 0u, bits, (hipStream_t)0));
            if (stmp.alloc(sb)) return BVG_E_NOMEM;
            HIPCHK(rocprim::radix_sort_pairs(stmp.get(), sb, (const uint64_t*)k0.get(), k1.get(), (const uint64_t*)v0.get(), v1.get(), (size_t)n, 0u, bits, (hipStream_t)0));
            hipLaunchKernelGGL(scat_number_kernel, dim3(grid(nodes, 256)), dim3(256), 0, 0, v1.get(), n, tab.get(), slots, d_s, t->ids.get());
            HIPCHK(hipMemcpy(h_s, d_s, sizeof h_s, hipMemcpyDeviceToHost));
            if (h_s[kSCollected] != n) return BVG_E_STATE;
        }
        clock.lap("number");
    }
    occ_id.reset();

    // ---- S4
    if (np0) hipLaunchKernelGGL(scat_lookup_kernel, dim3(grid((int64_t)np0, 256)), dim3(256), 0, 0, s0.get(), d0.get(), np0, sym, nol, given, (uint64_t)nodes, tab.get(), slots,
                                arc_occ.get(), occ_off.get(), d_s);
    HIPCHK(hipMemcpy(h_s, d_s, sizeof h_s, hipMemcpyDeviceToHost));
    if (h_s[kSInternal]) return BVG_E_STATE;
    clock.lap("look up");
    tab.reset(); occ_off.reset(); arc_occ.reset();

    // ---- the report
    bvg_scattered_report r{};
    unsigned char last = '\n';
    if (nbytes) HIPCHK(hipMemcpy(&last, d_text + nbytes - 1, 1, hipMemcpyDeviceToHost));
    r.lines = nbrk + (last != '\n' && last != '\r' ? 1 : 0);
    r.bad_source = h_s[kSBadSource]; r.bad_target = h_s[kSBadTarget]; r.no_target = h_s[kSNoTarget]; r.too_large = h_s[kSTooLarge]; r.trailing = h_s[kSTrailing];
    r.unknown_source = h_s[kSUnknownSource]; r.unknown_target = h_s[kSUnknownTarget]; r.dropped_loops = h_s[kSLoops];
    r.arcs = np0 - r.unknown_source - r.unknown_target - r.dropped_loops;
    if (h_s[kSErr] != kNoError) {
        r.first_byte = h_s[kSErr] >> 4; r.first_reason = (int32_t)(h_s[kSErr] & 15u);
        const int rc = line_of(d_text, r.first_byte, d_s + kSLine, &r.first_line); if (rc) return rc;
    }
    if (rep) *rep = r;
    if (strict && r.first_reason) {
        if (err) { err->byte = r.first_byte; err->line = r.first_line; err->reason = r.first_reason; err->reserved = 0; }
        return BVG_E_IO;
    }
    const int rc = pairs_to_csr(s0, d0, np, nodes, t.get());
    if (rc) return rc;
    clock.lap("pairs->csr");
    *out = t.release();
    return 0;
}

int scattered_entry(const void* text, uint64_t nbytes, uint32_t flags, const void* known, int64_t n_known, int device, bvg_text** out, bvg_scattered_report* rep,
                    bvg_text_error* err, bool dev) {
    if (!out || (!text && nbytes) || n_known < 0 || (!known && n_known) || (flags & ~(uint32_t)(BVG_TEXT_SYMMETRIZE | BVG_TEXT_NO_LOOPS | BVG_TEXT_STRICT))) return BVG_E_ARG;
    *out = nullptr;
    if (err) { err->byte = 0; err->line = 0; err->reason = 0; err->reserved = 0; }
    if (rep) memset(rep, 0, sizeof *rep);
    return guarded([&]() -> int {
        int r = ensure_device(device); if (r) return r;
        DevArray<uint8_t> up; DevArray<unsigned long long> up_known;
        const uint8_t* d_text = (const uint8_t*)text;
        const unsigned long long* d_known = (const unsigned long long*)known;
        if (!dev) {
            if (up.alloc(nbytes)) return BVG_E_NOMEM;
            if (nbytes) HIPCHK(hipMemcpy(up.get(), text, nbytes, hipMemcpyHostToDevice));
            d_text = up.get();
            if (known) {
                if (up_known.alloc((size_t)n_known)) return BVG_E_NOMEM;
                if (n_known) HIPCHK(hipMemcpy(up_known.get(), known, (size_t)n_known * sizeof(int64_t), hipMemcpyHostToDevice));
                d_known = up_known.get();
            }
        }
        r = scattered_impl(d_text, nbytes, flags, d_known, n_known, known != nullptr, device, out, rep, err);
        if (hipDeviceSynchronize() != hipSuccess && !r) r = BVG_E_HIP;
        return r;
    });
}

int ids_get(bvg_text* t, void* ids, uint64_t cap, hipMemcpyKind kind) {
    if (!t) return BVG_E_ARG;
    if (!t->ids.get()) return BVG_E_UNSUPPORTED;
    if (ids && cap < (uint64_t)t->nodes) return BVG_E_CAPACITY;               // nothing is written
    HIPCHK(hipSetDevice(t->device));
    if (ids && t->nodes) HIPCHK(hipMemcpy(ids, t->ids.get(), (size_t)t->nodes * sizeof(int64_t), kind));
    return 0;
}

}  // namespace
}  // namespace bvghost

extern "C" {

int bvg_scattered_parse(const void* text, uint64_t nbytes, uint32_t flags, const int64_t* known_ids, int64_t n_known, int device, bvg_text** out, bvg_scattered_report* rep,
                        bvg_text_error* err) {
    return scattered_entry(text, nbytes, flags, known_ids, n_known, device, out, rep, err, false);
}
int bvg_scattered_parse_dev(const void* d_text, uint64_t nbytes, uint32_t flags, const void* d_known_ids, int64_t n_known, int device, bvg_text** out, bvg_scattered_report* rep,
                            bvg_text_error* err) {
    return scattered_entry(d_text, nbytes, flags, d_known_ids, n_known, device, out, rep, err, true);
}
int bvg_scattered_ids(bvg_text* t, int64_t* ids, uint64_t cap) { return ids_get(t, ids, cap, hipMemcpyDeviceToHost); }
int bvg_scattered_ids_dev(bvg_text* t, void* d_ids, uint64_t cap) { return ids_get(t, d_ids, cap, hipMemcpyDeviceToDevice); }

}  // extern "C"
