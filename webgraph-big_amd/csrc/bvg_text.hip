// bvg_text.hip — text graphs on the device: ASCIIGraph (ASCIIGraph.java: a node count, then one line of successors per node) and arc
// lists (ArcListASCIIGraph.java / ScatteredArcsASCIIGraph.java: one `source TAB target` line per arc), both ways.  The contract --
// byte classes, line breaks, the refusals and their reasons -- is the one of include/bvgraph_hip.h ("text graphs").
//
// PARSING is scan-and-scatter over the bytes, in tiles of kTile bytes, one workgroup each, kChunk bytes per lane:
//   T0  (arc lists) the last line event of every tile -- a line break, or a `#` that opens a comment line -- and from those the
//       comment state every tile starts in;
//   T1  per tile: token starts (a digit whose predecessor is no digit) and line breaks, counted;
//   --  prefix sums over the tiles (launch_exclusive_scan): every token gets its index, every break its line;
//   T2  one lane per token start reads the digits from global memory (tokens straddle lanes and tiles freely) and writes the value to
//       vals[token index]; every break writes tb[line] = the tokens before it.  Whatever is wrong goes into ONE 64-bit minimum,
//       (byte offset << 4 | reason): the smallest offset wins, so the report does not depend on the order of anything;
//   T3  checks that need a neighbour (a list that does not increase; an arc line without exactly two numbers) run over tokens / lines,
//       keep the smallest offending index, and that index is turned into a byte offset by one lane walking one tile (error path only).
// An ASCIIGraph is then done: adj = the tokens behind the header, adj_off[x] = tb[x] - 1.  An arc list goes on: (source, target) pairs,
// the reverse pairs with BVG_TEXT_SYMMETRIZE, two stable radix sorts (rocPRIM; by target, then by source), duplicates and dropped loops
// flagged, a prefix sum for the positions, one lower bound per node for adj_off.
//
// FORMATTING: items (a successor and its space; a node's line feed; an arc's whole line) get their byte lengths from the leading-zero
// count and a table of the powers of ten, a prefix sum places them, and every workgroup assembles the text of kItems consecutive
// items in LDS and writes it out in whole aligned dwords (the up to three bytes at either edge, which share a dword with a neighbour
// workgroup, singly).
#include <cstdint>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "bvg_host.h"
#include "bvg_text_shared.h"
#include "../../include/bvgraph_hip.h"

namespace bvghost {
namespace {

constexpr int64_t kMaxNodes = 1ll << 40;                            // beyond: adj_off alone would not fit any device (BVG_E_NOMEM)

__device__ __forceinline__ bool is_digit(unsigned c) { return c - '0' < 10u; }
__device__ __forceinline__ bool is_other(unsigned c) { return c > 32 && !is_digit(c); }

struct ParseArgs {
    const uint8_t* text; uint64_t nbytes;
    const uint8_t* state_in;            // arc lists: comment state at the start of every tile
    int32_t* cnt_tok; int32_t* cnt_brk; // T1 out
    const uint64_t* tok_base; const uint64_t* brk_base;   // T2 in
    int64_t* vals; uint64_t* tb;        // T2 out: vals[tokens], tb[breaks]
    int64_t n;                          // ASCIIGraph: the header's node count (lines 1 .. n are looked at)
    int64_t shift;                      // arc lists
    unsigned long long* err;            // the 64-bit minimum
    unsigned long long* max_id;         // arc lists: the largest shifted id
};

// value of the token that starts at p: 0 ok, else BVG_TEXT_TOO_LARGE
__device__ __forceinline__ unsigned parse_token(const uint8_t* text, uint64_t nbytes, uint64_t p, int64_t* out) {
    while (p < nbytes && text[p] == '0') p++;
    uint64_t v = 0; int sig = 0; bool big = false;
    for (; p < nbytes; p++) {
        const unsigned d = (unsigned)text[p] - '0';
        if (d >= 10u) break;
        if (++sig > 19) { big = true; break; }
        v = v * 10 + d;                                                   // 19 digits stay below 10^19 < 2^64
    }
    if (big || v > 0x7FFFFFFFFFFFFFFFull) { *out = INT64_MAX; return BVG_TEXT_TOO_LARGE; }
    *out = (int64_t)v;
    return 0;
}

// T1 (WRITE = false) and T2 (WRITE = true)
template <bool ARCS, bool WRITE>
__global__ void __launch_bounds__(kThreads) text_pass_kernel(ParseArgs a) {
    __shared__ uint32_t lds[kThreads];
    const uint64_t tile = blockIdx.x;
    const uint64_t base = tile * kTile + (uint64_t)threadIdx.x * kChunk;
    Chunk c; c.load(a.text, a.nbytes, base);
    bool comment = false;
    if (ARCS) comment = lane_in_comment(c, a.state_in, tile, lds);
    // the lane's counts: tokens in the low half, breaks in the high half (a tile holds at most 2048 / 4096)
    uint32_t mine = 0;
    {
        unsigned prev = c.prev; bool com = comment;
#pragma unroll
        for (int i = 0; i < kChunk; i++) {
            const unsigned ch = c.b[i];
            if (i < c.len) {
                if (is_break(ch, prev)) { mine += 1u << 16; com = false; }
                else if (ARCS && ch == '#' && (prev == '\r' || prev == '\n')) com = true;
                else if (!com && is_digit(ch) && !is_digit(prev)) mine += 1;
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
    uint64_t top = 0; bool any = false;
    for (int i = 0; i < c.len; i++) {
        const unsigned ch = c.b[i];
        const uint64_t p = base + (uint64_t)i;
        const bool looked = ARCS ? true : (line >= 1 && line <= (uint64_t)a.n);   // the header has been read already; nobody reads behind line n + 1
        if (is_break(ch, prev)) { a.tb[line] = tok; line++; com = false; }
        else if (ARCS && ch == '#' && (prev == '\r' || prev == '\n')) com = true;
        else if (!com) {
            if (is_digit(ch)) {
                if (!is_digit(prev)) {
                    int64_t v; unsigned why = parse_token(a.text, a.nbytes, p, &v);
                    if (ARCS && !why) {
                        if ((a.shift < 0 && v < -a.shift) || (a.shift > 0 && v > INT64_MAX - a.shift)) why = BVG_TEXT_SHIFT_RANGE;
                        else { v += a.shift; top = (uint64_t)v > top ? (uint64_t)v : top; any = true; }
                    }
                    if (!ARCS && !why && v >= a.n) why = BVG_TEXT_NOT_NODE;
                    a.vals[tok] = v;
                    tok++;
                    if (why && looked) report(a.err, p, why);
                }
            } else if (looked && is_other(ch)) report(a.err, p, BVG_TEXT_BAD_BYTE);
        }
        prev = ch;
    }
    if (ARCS) {
        // one atomic per wavefront
        for (int d = 32; d; d >>= 1) { const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)top, d, 64); top = o > top ? o : top; }
        if (ballot(any) && (threadIdx.x & 63u) == 0) atomicMax(a.max_id, (unsigned long long)top);
    }
}

// The header of an ASCIIGraph: line 0, digits only.  One lane (the line is a few bytes).  out[0] = n, out[1] = the error key or kNoError.
__global__ void text_header_kernel(const uint8_t* text, uint64_t nbytes, unsigned long long* out) {
    uint64_t p = 0; unsigned prev = '\n';
    unsigned long long key = kNoError;
    for (; p < nbytes; p++) {
        const unsigned ch = text[p];
        if (is_break(ch, prev)) break;
        if (!is_digit(ch)) { key = p << 4 | (is_other(ch) ? BVG_TEXT_BAD_BYTE : BVG_TEXT_BAD_HEADER); break; }
        prev = ch;
    }
    int64_t v = 0;
    if (key == kNoError) {
        if (p == 0) key = 0 << 4 | BVG_TEXT_BAD_HEADER;
        else if (parse_token(text, nbytes, 0, &v)) key = 0 << 4 | BVG_TEXT_TOO_LARGE;
    }
    out[0] = (unsigned long long)v; out[1] = key;
}

__device__ __forceinline__ uint64_t upper_bound64(const uint64_t* a, uint64_t n, uint64_t key) {   // first index with a[i] > key
    uint64_t l = 0, r = n;
    while (l < r) { const uint64_t m = (l + r) >> 1; if (a[m] <= key) l = m + 1; else r = m; }
    return l;
}
__device__ __forceinline__ uint64_t lower_bound64(const uint64_t* a, uint64_t n, uint64_t key) {   // first index with a[i] >= key
    uint64_t l = 0, r = n;
    while (l < r) { const uint64_t m = (l + r) >> 1; if (a[m] < key) l = m + 1; else r = m; }
    return l;
}

// T3, ASCIIGraph: tokens [2, ntok) against their predecessor when both stand in one list.  tb[0 .. nb): tokens before every break looked at.
__global__ void text_increasing_kernel(const int64_t* vals, uint64_t ntok, const uint64_t* tb, uint64_t nb, unsigned long long* bad_tok) {
    BVG_FOR(i, ntok) {
        const uint64_t t = (uint64_t)i;
        if (t < 2 || vals[t - 1] < vals[t]) continue;
        const uint64_t l = upper_bound64(tb, nb, t);                       // breaks with tb <= t: t stands in line l
        if (l == 0 || tb[l - 1] == t) continue;                            // (the header's token; the first of its line)
        atomicMin(bad_tok, (unsigned long long)t);
    }
}
// T3, arc lists: line l holds tb[l] - tb[l - 1] tokens (tb[-1] = 0; the unterminated last line is l == nb and ends at ntok): 0 or 2, or it is refused
__global__ void text_fields_kernel(const uint64_t* tb, uint64_t nb, uint64_t ntok, unsigned long long* bad_line) {
    BVG_FOR(i, nb + 1) {
        const uint64_t l = (uint64_t)i;
        const uint64_t cnt = (l < nb ? tb[l] : ntok) - (l ? tb[l - 1] : 0);
        if (cnt != 0 && cnt != 2) atomicMin(bad_line, (unsigned long long)l);
    }
}
// error path: the byte offset of token `index` (which = 0) or of break `index` (which = 1); one lane walks the one tile that holds it
template <bool ARCS>
__global__ void text_locate_kernel(const uint8_t* text, uint64_t nbytes, const uint8_t* state_in, const uint64_t* tok_base, const uint64_t* brk_base, uint64_t tiles,
                                   int which, uint64_t index, unsigned long long* out) {
    const uint64_t* basev = which ? brk_base : tok_base;
    const uint64_t tile = upper_bound64(basev, tiles + 1, index) - 1;      // base[tile] <= index < base[tile + 1]
    *out = nbytes;
    if (tile >= tiles) return;
    uint64_t tok = tok_base[tile], brk = brk_base[tile];
    bool com = ARCS && state_in[tile] == kEvComment;
    const uint64_t lo = tile * kTile, hi = lo + kTile < nbytes ? lo + kTile : nbytes;
    unsigned prev = lo ? text[lo - 1] : '\n';
    for (uint64_t p = lo; p < hi; p++) {
        const unsigned ch = text[p];
        if (is_break(ch, prev)) { if (which && brk == index) { *out = p; return; } brk++; com = false; }
        else if (ARCS && ch == '#' && (prev == '\r' || prev == '\n')) com = true;
        else if (!com && is_digit(ch) && !is_digit(prev)) { if (!which && tok == index) { *out = p; return; } tok++; }
        prev = ch;
    }
}
__global__ void text_adj_off_kernel(const uint64_t* tb, int64_t n, uint64_t* adj_off) {   // adj_off[x] = tb[x] - 1 (the header's token)
    BVG_FOR(x, n + 1) adj_off[x] = tb[x] - 1;
}

// ---- arc lists behind the token pass
// pairs from the tokens: (vals[2 i], vals[2 i + 1]); with `sym` the reverse pair at i + np; a loop under `no_loops` becomes (drop, drop), which sorts last
__global__ void text_pairs_kernel(const int64_t* vals, uint64_t np, bool sym, bool no_loops, uint64_t drop, uint64_t* src, uint64_t* dst) {
    BVG_FOR(i, np) {
        uint64_t s = (uint64_t)vals[2 * i], t = (uint64_t)vals[2 * i + 1];
        if (no_loops && s == t) s = t = drop;
        src[i] = s; dst[i] = t;
        if (sym) { src[i + np] = t; dst[i + np] = s; }
    }
}
__global__ void text_unique_kernel(const uint64_t* src, const uint64_t* dst, uint64_t np, uint64_t drop, int32_t* keep) {
    BVG_FOR(i, np) keep[i] = src[i] != drop && (i == 0 || src[i] != src[i - 1] || dst[i] != dst[i - 1]);
}
__global__ void text_compact_kernel(const uint64_t* dst, const int32_t* keep, const uint64_t* pos, uint64_t np, int64_t* adj) {
    BVG_FOR(i, np) if (keep[i]) adj[pos[i]] = (int64_t)dst[i];
}
__global__ void text_arc_off_kernel(const uint64_t* src, const uint64_t* pos, uint64_t np, int64_t n, uint64_t* adj_off) {
    BVG_FOR(x, n + 1) adj_off[x] = pos[lower_bound64(src, np, (uint64_t)x)];   // pos[np] = the arcs kept
}

// ---- formatting
__constant__ uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                    100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                    100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};
// decimal digits of v: 1233 / 4096 ~ log10(2) turns the bit length into a guess that is right or one too small
__device__ __forceinline__ int digits10(uint64_t v) {
    v |= 1;                                      // (0 has one digit; setting the last bit never changes a count)
    const int bits = 64 - (int)__builtin_clzll(v);
    const int g = (bits * 1233) >> 12;
    return g + (v >= kPow10[g] ? 1 : 0);
}

constexpr int kItems = 512;                      // items per workgroup of the writing pass
constexpr int kMaxItemBytes = 42;                // an arc line: 2 x (19 digits + 1)... 20-digit headroom for either end
enum { kFmtAscii = BVG_TEXT_ASCII, kFmtArcs = BVG_TEXT_ARCS };

struct FormatArgs {
    int kind; int64_t first_node, nodes; const uint64_t* off; const int64_t* adj; int64_t shift; uint64_t arcs;
    uint64_t items;                              // ASCII: arcs + nodes (item off[x] + x .. off[x + 1] + x: the arcs of node x, then its line feed); arcs: arcs
};
// node of item k, and whether k is the node's line feed (ASCII) / node of arc k (arcs)
__device__ __forceinline__ int64_t fmt_node_ascii(const FormatArgs& a, uint64_t k, bool* lf) {
    int64_t l = 0, r = a.nodes;                  // last x with off[x] + x <= k
    while (r - l > 1) { const int64_t m = (l + r) >> 1; if (a.off[m] - a.off[0] + (uint64_t)m <= k) l = m; else r = m; }
    *lf = k == a.off[l + 1] - a.off[0] + (uint64_t)l;
    return l;
}
__device__ __forceinline__ int64_t fmt_node_arcs(const FormatArgs& a, uint64_t k) {
    return (int64_t)upper_bound64(a.off, (uint64_t)a.nodes + 1, k + a.off[0]) - 1;
}
__device__ __forceinline__ bool fmt_shifted(int64_t v, int64_t shift, uint64_t* out) {     // v + shift inside [0, 2^63 - 1]
    if (v < 0 || (shift < 0 && v < -shift) || (shift > 0 && v > INT64_MAX - shift)) return false;
    *out = (uint64_t)(v + shift);
    return true;
}

__global__ void format_len_kernel(FormatArgs a, int32_t* len, unsigned* bad) {
    BVG_FOR(i, a.items) {
        const uint64_t k = (uint64_t)i;
        int32_t l = 1;
        if (a.kind == kFmtAscii) {
            bool lf; const int64_t x = fmt_node_ascii(a, k, &lf);
            if (!lf) {
                const int64_t v = a.adj[k - (uint64_t)x];
                if (v < 0) { atomicOr(bad, 1u); } else l = digits10((uint64_t)v) + 1;
            }
        } else {
            const int64_t x = fmt_node_arcs(a, k);
            uint64_t s = 0, t = 0;
            if (!fmt_shifted(a.first_node + x, a.shift, &s) || !fmt_shifted(a.adj[k], a.shift, &t)) atomicOr(bad, 1u);
            l = digits10(s) + digits10(t) + 2;
        }
        len[k] = l;
    }
}

__device__ __forceinline__ void put_number(unsigned char* q, uint64_t v, int nd, unsigned char after) {   // nd digits of v, then `after`
    q[nd] = after;
    for (int i = nd - 1; i >= 0; i--) { q[i] = (unsigned char)('0' + v % 10); v /= 10; }
}

// pos[items + 1]: byte positions; out + pos[k] receives item k
__global__ void __launch_bounds__(256) format_write_kernel(FormatArgs a, const uint64_t* pos, uint8_t* out) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[kItems * kMaxItemBytes + 8];
    const uint64_t k0 = (uint64_t)blockIdx.x * kItems, k1 = k0 + kItems < a.items ? k0 + kItems : a.items;
    const uint64_t b0 = pos[k0], b1 = pos[k1];
    const unsigned mis = (unsigned)((uintptr_t)(out + b0) & 3u);          // the tile starts `mis` bytes into a dword of the output
    for (uint64_t k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
        unsigned char* q = tile + mis + (pos[k] - b0);
        if (a.kind == kFmtAscii) {
            bool lf; const int64_t x = fmt_node_ascii(a, k, &lf);
            if (lf) *q = '\n';
            else { const uint64_t v = (uint64_t)a.adj[k - (uint64_t)x]; put_number(q, v, digits10(v), ' '); }
        } else {
            const int64_t x = fmt_node_arcs(a, k);
            const uint64_t s = (uint64_t)(a.first_node + x + a.shift), t = (uint64_t)(a.adj[k] + a.shift);
            const int ds = digits10(s);
            put_number(q, s, ds, '\t'); put_number(q + ds + 1, t, digits10(t), '\n');
        }
    }
    __syncthreads();
    const uint64_t total = b1 - b0;
    // bytes [head, head + 4 * words) of the tile's text are whole dwords of the output
    const uint64_t head = mis ? (4 - mis < total ? 4 - mis : total) : 0;
    const uint64_t words = (total - head) >> 2, tail = head + (words << 2);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out + b0 + head);
    const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tile + mis + head);   // mis + head is 0 or 4
    for (uint64_t w = threadIdx.x; w < words; w += blockDim.x) o32[w] = t32[w];
    if (threadIdx.x < head) out[b0 + threadIdx.x] = tile[mis + threadIdx.x];
    if (threadIdx.x >= 64 && tail + (threadIdx.x - 64) < total) out[b0 + tail + (threadIdx.x - 64)] = tile[mis + tail + (threadIdx.x - 64)];
}

unsigned bits_of(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 1u; }

int text_status(unsigned reason) { return reason == BVG_TEXT_NOT_INCREASING || reason == BVG_TEXT_SHIFT_RANGE ? BVG_E_ARG : BVG_E_IO; }

// fills *err from a key; the line is counted on the device (error path only)
int refuse(const uint8_t* d_text, uint64_t key, unsigned long long* d_scratch, bvg_text_error* err) {
    const uint64_t byte = key >> 4; const unsigned reason = (unsigned)(key & 15u);
    int64_t line = 0;
    const int r = line_of(d_text, byte, d_scratch, &line); if (r) return r;
    if (err) { err->byte = byte; err->line = line; err->reason = (int32_t)reason; err->reserved = 0; }
    return text_status(reason);
}

}  // namespace

// pairs -> CSR, shared with bvg_transform.hip: np (source, target) pairs in s0 / d0 (both are used up), a pair to be dropped holding `nodes` at
// both ends (no id reaches it, so it sorts last).  Two stable radix sorts (by target, then by source), duplicates and dropped pairs flagged,
// a prefix sum for the positions, one lower bound per node for adj_off.  Fills t->nodes, arcs, d_off, adj.
int pairs_to_csr(DevArray<uint64_t>& s0, DevArray<uint64_t>& d0, uint64_t np, int64_t nodes, bvg_text* t) {
    if (nodes > kMaxNodes) return BVG_E_NOMEM;
    t->nodes = nodes;
    if (t->d_off.alloc((size_t)nodes + 1)) return BVG_E_NOMEM;
    if (np == 0) {
        HIPCHK(hipMemset(t->d_off, 0, ((size_t)nodes + 1) * sizeof(uint64_t)));
        if (t->adj_base.alloc(1)) return BVG_E_NOMEM;
        t->d_adj = t->adj_base; t->arcs = 0;
        return 0;
    }
    if (np > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                      // the prefix sum below takes fewer than 2^31 elements
    DevArray<uint64_t> s1, d1, pos, ptmp; DevArray<uint8_t> stmp; DevArray<int32_t> keep;
    if (s1.alloc(np) || d1.alloc(np)) return BVG_E_NOMEM;
    const uint64_t drop = (uint64_t)nodes;
    const unsigned bits = bits_of(drop);
    size_t sb = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, sb, (const uint64_t*)d0.get(), d1.get(), (const uint64_t*)s0.get(), s1.get(), (size_t)np, 0u, bits, (hipStream_t)0));
    if (stmp.alloc(sb)) return BVG_E_NOMEM;
    // stable LSD: by target, then by source
    HIPCHK(rocprim::radix_sort_pairs(stmp.get(), sb, (const uint64_t*)d0.get(), d1.get(), (const uint64_t*)s0.get(), s1.get(), (size_t)np, 0u, bits, (hipStream_t)0));
    HIPCHK(rocprim::radix_sort_pairs(stmp.get(), sb, (const uint64_t*)s1.get(), s0.get(), (const uint64_t*)d1.get(), d0.get(), (size_t)np, 0u, bits, (hipStream_t)0));
    stmp.reset(); s1.reset(); d1.reset();
    if (keep.alloc(np) || pos.alloc(np + 1) || ptmp.alloc(scan_tmp_elems((int64_t)np))) return BVG_E_NOMEM;
    hipLaunchKernelGGL(text_unique_kernel, dim3(grid((int64_t)np, 256)), dim3(256), 0, 0, s0.get(), d0.get(), np, drop, keep.get());
    launch_exclusive_scan(keep.get(), pos.get(), (int64_t)np, ptmp.get(), nullptr);
    uint64_t kept = 0;
    HIPCHK(hipMemcpy(&kept, pos.get() + np, sizeof kept, hipMemcpyDeviceToHost));
    if (t->adj_base.alloc(kept)) return BVG_E_NOMEM;
    t->d_adj = t->adj_base; t->arcs = kept;
    hipLaunchKernelGGL(text_compact_kernel, dim3(grid((int64_t)np, 256)), dim3(256), 0, 0, d0.get(), keep.get(), pos.get(), np, t->d_adj);
    hipLaunchKernelGGL(text_arc_off_kernel, dim3(grid(nodes + 1, 256)), dim3(256), 0, 0, s0.get(), pos.get(), np, nodes, t->d_off.get());
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

namespace {

int parse_impl(bool arcs_mode, const uint8_t* d_text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err) {
    const uint64_t tiles = (nbytes + kTile - 1) / kTile, tl = tiles ? tiles : 1;
    if (tiles > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                   // 8 TiB of text
    DevArray<unsigned long long> scal; DevArray<uint8_t> ev, state; DevArray<int32_t> ctok, cbrk; DevArray<uint64_t> btok, bbrk, tmp, tb; DevArray<int64_t> vals;
    if (scal.alloc(8)) return BVG_E_NOMEM;
    unsigned long long* d_s = scal.get();                 // [0] n [1] header key [2] error key [3] max id [4] T3 index [5] located [6] line count
    unsigned long long h_s[8] = {0, kNoError, kNoError, 0, kNoError, 0, 0, 0};
    HIPCHK(hipMemcpy(d_s, h_s, sizeof h_s, hipMemcpyHostToDevice));
    ParseArgs a{};
    a.text = d_text; a.nbytes = nbytes; a.shift = shift; a.err = d_s + 2; a.max_id = d_s + 3;
    int64_t n = 0;
    if (!arcs_mode) {
        hipLaunchKernelGGL(text_header_kernel, dim3(1), dim3(1), 0, 0, d_text, nbytes, d_s);
        HIPCHK(hipMemcpy(h_s, d_s, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (h_s[1] != kNoError) return refuse(d_text, h_s[1], d_s + 6, err);
        n = (int64_t)h_s[0];
    }
    a.n = n;
    if (ctok.alloc(tl) || cbrk.alloc(tl) || btok.alloc(tl + 1) || bbrk.alloc(tl + 1) || tmp.alloc(scan_tmp_elems((int64_t)tl))) return BVG_E_NOMEM;
    HIPCHK(hipMemset(btok.get(), 0, (tl + 1) * sizeof(uint64_t))); HIPCHK(hipMemset(bbrk.get(), 0, (tl + 1) * sizeof(uint64_t)));
    a.cnt_tok = ctok.get(); a.cnt_brk = cbrk.get(); a.tok_base = btok.get(); a.brk_base = bbrk.get();
    uint64_t ntok = 0, nbrk = 0;
    if (tiles) {
        if (arcs_mode) {
            if (ev.alloc(tiles) || state.alloc(tiles)) return BVG_E_NOMEM;
            hipLaunchKernelGGL(text_events_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, 0, d_text, nbytes, ev.get());
            hipLaunchKernelGGL(text_state_kernel, dim3(1), dim3(kThreads), 0, 0, ev.get(), tiles, state.get());
            a.state_in = state.get();
            hipLaunchKernelGGL((text_pass_kernel<true, false>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
        } else hipLaunchKernelGGL((text_pass_kernel<false, false>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
        launch_exclusive_scan(a.cnt_tok, btok.get(), (int64_t)tiles, tmp.get(), nullptr);
        launch_exclusive_scan(a.cnt_brk, bbrk.get(), (int64_t)tiles, tmp.get(), nullptr);
        HIPCHK(hipMemcpy(&ntok, btok.get() + tiles, sizeof ntok, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&nbrk, bbrk.get() + tiles, sizeof nbrk, hipMemcpyDeviceToHost));
    }
    if (vals.alloc(ntok + 1) || tb.alloc(nbrk + 1)) return BVG_E_NOMEM;
    a.vals = vals.get(); a.tb = tb.get();
    if (tiles) {
        if (arcs_mode) hipLaunchKernelGGL((text_pass_kernel<true, true>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
        else hipLaunchKernelGGL((text_pass_kernel<false, true>), dim3((unsigned)tiles), dim3(kThreads), 0, 0, a);
    }
    // what the neighbour checks look at: ASCIIGraph -- the tokens before break n (all of them when the text ends early)
    // (n = 0 asks for no line at all: the header may even lack its line break)
    const bool complete = arcs_mode || n == 0 || nbrk >= (uint64_t)n + 1;
    uint64_t look_tok = ntok, look_brk = nbrk;
    if (!arcs_mode && complete) {
        look_brk = n ? (uint64_t)n + 1 : 0; look_tok = 1;
        if (n) HIPCHK(hipMemcpy(&look_tok, tb.get() + n, sizeof look_tok, hipMemcpyDeviceToHost));
    }
    if (arcs_mode) hipLaunchKernelGGL(text_fields_kernel, dim3(grid((int64_t)nbrk + 1, 256)), dim3(256), 0, 0, tb.get(), nbrk, ntok, d_s + 4);
    else if (look_tok > 2) hipLaunchKernelGGL(text_increasing_kernel, dim3(grid((int64_t)look_tok, 256)), dim3(256), 0, 0, vals.get(), look_tok, tb.get(), look_brk, d_s + 4);
    HIPCHK(hipMemcpy(h_s, d_s, sizeof h_s, hipMemcpyDeviceToHost));
    uint64_t key = h_s[2];
    if (h_s[4] != kNoError) {
        // the smallest offending token (ASCIIGraph), line (arc lists) -> its byte offset
        int which = 0; uint64_t index = h_s[4]; unsigned reason = BVG_TEXT_NOT_INCREASING; uint64_t at = nbytes; bool locate = true;
        if (arcs_mode) {
            reason = BVG_TEXT_ARC_FIELDS;
            uint64_t tbl[2] = {0, ntok};                                    // tb[l - 1], tb[l]
            if (index) HIPCHK(hipMemcpy(&tbl[0], tb.get() + index - 1, sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (index < nbrk) HIPCHK(hipMemcpy(&tbl[1], tb.get() + index, sizeof(uint64_t), hipMemcpyDeviceToHost));
            if (tbl[1] - tbl[0] == 1) { which = 1; locate = index < nbrk; }  // one number: at the break that ends the line (at the end of the text without one)
            else index = tbl[0] + 2;                                        // three or more: at the third
        }
        if (locate) {
            if (arcs_mode) hipLaunchKernelGGL((text_locate_kernel<true>), dim3(1), dim3(1), 0, 0, d_text, nbytes, a.state_in, a.tok_base, a.brk_base, tiles, which, index, d_s + 5);
            else hipLaunchKernelGGL((text_locate_kernel<false>), dim3(1), dim3(1), 0, 0, d_text, nbytes, a.state_in, a.tok_base, a.brk_base, tiles, which, index, d_s + 5);
            HIPCHK(hipMemcpy(&at, d_s + 5, sizeof at, hipMemcpyDeviceToHost));
        }
        const uint64_t k2 = at << 4 | reason;
        if (k2 < key) key = k2;
    }
    if (!complete) { const uint64_t k3 = nbytes << 4 | BVG_TEXT_EOF; if (k3 < key) key = k3; }
    if (key != kNoError) return refuse(d_text, key, d_s + 6, err);

    std::unique_ptr<bvg_text> t(new bvg_text);
    t->device = device;
    if (!arcs_mode) {
        if (n > kMaxNodes) return BVG_E_NOMEM;
        t->nodes = n; t->arcs = look_tok - 1;
        if (t->d_off.alloc((size_t)n + 1)) return BVG_E_NOMEM;
        if (n == 0) HIPCHK(hipMemset(t->d_off, 0, sizeof(uint64_t)));
        else hipLaunchKernelGGL(text_adj_off_kernel, dim3(grid(n + 1, 256)), dim3(256), 0, 0, tb.get(), n, t->d_off.get());
        HIPCHK(hipDeviceSynchronize());
        t->adj_base = std::move(vals); t->d_adj = t->adj_base + 1;                  // behind the header's token
        *out = t.release();
        return 0;
    }
    // ---- arc list: pairs -> sort -> unique -> CSR
    const uint64_t np0 = ntok / 2;
    const bool sym = (flags & BVG_TEXT_SYMMETRIZE) != 0, nol = (flags & BVG_TEXT_NO_LOOPS) != 0;
    const uint64_t np = sym ? 2 * np0 : np0;
    uint64_t top = h_s[3];
    if (np0 && top >= (uint64_t)kMaxNodes) return BVG_E_NOMEM;
    int64_t nodes = np0 ? (int64_t)top + 1 : 0;
    if (min_nodes > nodes) nodes = min_nodes;
    if (nodes > kMaxNodes) return BVG_E_NOMEM;
    if (np > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                      // the prefix sum of pairs_to_csr takes fewer than 2^31 elements
    DevArray<uint64_t> s0, d0;
    if (np) {
        if (s0.alloc(np) || d0.alloc(np)) return BVG_E_NOMEM;
        hipLaunchKernelGGL(text_pairs_kernel, dim3(grid((int64_t)np0, 256)), dim3(256), 0, 0, vals.get(), np0, sym, nol, (uint64_t)nodes, s0.get(), d0.get());
    }
    const int r = pairs_to_csr(s0, d0, np, nodes, t.get());
    if (r) return r;
    *out = t.release();
    return 0;
}

int parse_entry(bool arcs_mode, const void* text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err, bool dev) {
    if (!out || (!text && nbytes) || min_nodes < 0 || shift == INT64_MIN || (flags & ~(uint32_t)(BVG_TEXT_SYMMETRIZE | BVG_TEXT_NO_LOOPS))) return BVG_E_ARG;   // (-shift must exist)
    *out = nullptr;
    if (err) { err->byte = 0; err->line = 0; err->reason = 0; err->reserved = 0; }
    return guarded([&]() -> int {
        int r = ensure_device(device); if (r) return r;
        DevArray<uint8_t> up;
        const uint8_t* d_text = (const uint8_t*)text;
        if (!dev) {
            if (up.alloc(nbytes)) return BVG_E_NOMEM;
            if (nbytes) HIPCHK(hipMemcpy(up.get(), text, nbytes, hipMemcpyHostToDevice));
            d_text = up.get();
        }
        r = parse_impl(arcs_mode, d_text, nbytes, shift, flags, min_nodes, device, out, err);
        if (hipDeviceSynchronize() != hipSuccess && !r) r = BVG_E_HIP;
        return r;
    });
}

// the text of an adjacency on the device: off[nodes + 1] (any base: off[0] is subtracted), adj[off[nodes] - off[0]]
int format_dev(int kind, int64_t first_node, int64_t nodes, const uint64_t* d_off, const int64_t* d_adj, uint64_t arcs, int64_t shift,
               void* out, uint64_t cap, uint64_t* nbytes, bool dev) {
    FormatArgs a{kind, first_node, nodes, d_off, d_adj, shift, arcs, kind == kFmtAscii ? arcs + (uint64_t)nodes : arcs};
    *nbytes = 0;
    if (a.items == 0) return 0;
    if (a.items > 0x7FFFFFFFull) return BVG_E_UNSUPPORTED;                 // one call formats fewer than 2^31 items: the writers go range by range
    DevArray<int32_t> len; DevArray<uint64_t> pos, tmp; DevArray<unsigned> bad; DevArray<uint8_t> text;
    if (len.alloc(a.items) || pos.alloc(a.items + 1) || tmp.alloc(scan_tmp_elems((int64_t)a.items)) || bad.alloc(1)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(bad.get(), 0, sizeof(unsigned)));
    hipLaunchKernelGGL(format_len_kernel, dim3(grid((int64_t)a.items, 256)), dim3(256), 0, 0, a, len.get(), bad.get());
    launch_exclusive_scan(len.get(), pos.get(), (int64_t)a.items, tmp.get(), nullptr);
    uint64_t total = 0; unsigned hb = 0;
    HIPCHK(hipMemcpy(&total, pos.get() + a.items, sizeof total, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hb, bad.get(), sizeof hb, hipMemcpyDeviceToHost));
    if (hb) return BVG_E_ARG;                                              // a negative successor, or an id the shift takes out of [0, 2^63 - 1]
    *nbytes = total;
    if (!out || cap < total) return BVG_E_CAPACITY;
    uint8_t* d_out = (uint8_t*)out;
    if (!dev) { if (text.alloc(total)) return BVG_E_NOMEM; d_out = text.get(); }
    hipLaunchKernelGGL(format_write_kernel, dim3((unsigned)((a.items + kItems - 1) / kItems)), dim3(256), 0, 0, a, pos.get(), d_out);
    if (!dev) HIPCHK(hipMemcpy(out, d_out, total, hipMemcpyDeviceToHost));
    else HIPCHK(hipDeviceSynchronize());
    return 0;
}

int format_graph(int kind, bvg_graph* g, int64_t from, int64_t to, int64_t shift, void* out, uint64_t cap, uint64_t* nbytes, bool dev) {
    if (!g || !nbytes || shift == INT64_MIN) return BVG_E_ARG;
    bvg_params p; int r = bvg_info(g, &p); if (r) return r;
    if (from < 0 || to > p.nodes || from > to) return BVG_E_ARG;
    return guarded([&]() -> int {
        *nbytes = 0;
        if (from == to) return 0;
        HIPCHK(hipSetDevice(g->sh->device));
        const int64_t cnt = to - from;
        DevArray<int32_t> deg; DevArray<uint64_t> cum, tmp; DevArray<int64_t> succ;
        if (deg.alloc((size_t)cnt) || cum.alloc((size_t)cnt + 1) || tmp.alloc(scan_tmp_elems(cnt))) return BVG_E_NOMEM;
        const Shared* sh = g->sh;
        launch_outdegrees(sh->d_graph, sh->nbytes, sh->offs, from, to, sh->p.outdegree_coding, deg.get(), nullptr, g->stream);
        launch_exclusive_scan(deg.get(), cum.get(), cnt, tmp.get(), g->stream);
        uint64_t m = 0;
        HIPCHK(hipMemcpyAsync(&m, cum.get() + cnt, sizeof m, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        if (succ.alloc(m)) return BVG_E_NOMEM;
        if (m) { uint64_t got = 0; const int rc = bvg_decode_range_dev(g, from, to, nullptr, succ.get(), m, &got); if (rc) return rc; }   // straight into the formatter's input
        HIPCHK(hipStreamSynchronize(g->stream));
        return format_dev(kind, from + (int64_t)g->node_base, cnt, cum.get(), succ.get(), m, shift, out, cap, nbytes, dev);
    });
}

}  // namespace
}  // namespace bvghost

extern "C" {

int bvg_text_parse_ascii(const void* text, uint64_t nbytes, int device, bvg_text** out, bvg_text_error* err) {
    return parse_entry(false, text, nbytes, 0, 0, 0, device, out, err, false);
}
int bvg_text_parse_ascii_dev(const void* d_text, uint64_t nbytes, int device, bvg_text** out, bvg_text_error* err) {
    return parse_entry(false, d_text, nbytes, 0, 0, 0, device, out, err, true);
}
int bvg_text_parse_arcs(const void* text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err) {
    return parse_entry(true, text, nbytes, shift, flags, min_nodes, device, out, err, false);
}
int bvg_text_parse_arcs_dev(const void* d_text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err) {
    return parse_entry(true, d_text, nbytes, shift, flags, min_nodes, device, out, err, true);
}

void bvg_text_close(bvg_text* t) { delete t; }

int bvg_text_info(const bvg_text* t, int64_t* nodes, uint64_t* arcs) {
    if (!t) return BVG_E_ARG;
    if (nodes) *nodes = t->nodes;
    if (arcs) *arcs = t->arcs;
    return 0;
}

static int text_get(bvg_text* t, void* adj_off, uint64_t off_cap, void* adj, uint64_t adj_cap, hipMemcpyKind kind) {
    if (!t) return BVG_E_ARG;
    if ((adj_off && off_cap < (uint64_t)t->nodes + 1) || (adj && adj_cap < t->arcs)) return BVG_E_CAPACITY;   // nothing is written
    HIPCHK(hipSetDevice(t->device));
    if (adj_off) HIPCHK(hipMemcpy(adj_off, t->d_off, ((size_t)t->nodes + 1) * sizeof(uint64_t), kind));
    if (adj && t->arcs) HIPCHK(hipMemcpy(adj, t->d_adj, (size_t)t->arcs * sizeof(int64_t), kind));
    return 0;
}
int bvg_text_get(bvg_text* t, uint64_t* adj_off, uint64_t off_cap, int64_t* adj, uint64_t adj_cap) { return text_get(t, adj_off, off_cap, adj, adj_cap, hipMemcpyDeviceToHost); }
int bvg_text_get_dev(bvg_text* t, void* d_adj_off, uint64_t off_cap, void* d_adj, uint64_t adj_cap) { return text_get(t, d_adj_off, off_cap, d_adj, adj_cap, hipMemcpyDeviceToDevice); }

int bvg_text_store(bvg_text* t, const bvg_params* p, int64_t chunk_nodes, uint8_t** graph, uint64_t* graph_bytes, uint64_t** offsets) {
    if (!t || !p || !graph || !graph_bytes || !offsets) return BVG_E_ARG;
    return guarded([&]() -> int {
        bvg_params q = *p; q.nodes = t->nodes;
        int r = check_params(q); if (r) return r;
        HIPCHK(hipSetDevice(t->device));
        uint8_t* pg = nullptr; uint64_t* po = nullptr; uint64_t nbytes = 0;
        r = encode_store_dev(q, t->d_off, t->d_adj, t->nodes, chunk_nodes, nullptr, &pg, &nbytes, &po);
        if (r) return r;
        DevArray<uint8_t> d_graph; DevArray<uint64_t> d_offsets; d_graph.adopt(pg, (size_t)nbytes); d_offsets.adopt(po, (size_t)t->nodes + 1);
        HostArray<uint8_t> hg((uint8_t*)calloc((size_t)nbytes + 16, 1)); HostArray<uint64_t> ho((uint64_t*)malloc(((size_t)t->nodes + 1) * sizeof(uint64_t)));
        if (!hg || !ho) return BVG_E_NOMEM;
        if ((nbytes && hipMemcpy(hg.get(), d_graph, (size_t)nbytes, hipMemcpyDeviceToHost) != hipSuccess) ||
            hipMemcpy(ho.get(), d_offsets, ((size_t)t->nodes + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return BVG_E_HIP;
        *graph = hg.release(); *graph_bytes = nbytes; *offsets = ho.release();
        return 0;
    });
}

int bvg_text_format_ascii(bvg_graph* g, int64_t from, int64_t to, void* out, uint64_t cap, uint64_t* nbytes) { return format_graph(BVG_TEXT_ASCII, g, from, to, 0, out, cap, nbytes, false); }
int bvg_text_format_ascii_dev(bvg_graph* g, int64_t from, int64_t to, void* d_out, uint64_t cap, uint64_t* nbytes) { return format_graph(BVG_TEXT_ASCII, g, from, to, 0, d_out, cap, nbytes, true); }
int bvg_text_format_arcs(bvg_graph* g, int64_t from, int64_t to, int64_t shift, void* out, uint64_t cap, uint64_t* nbytes) { return format_graph(BVG_TEXT_ARCS, g, from, to, shift, out, cap, nbytes, false); }
int bvg_text_format_arcs_dev(bvg_graph* g, int64_t from, int64_t to, int64_t shift, void* d_out, uint64_t cap, uint64_t* nbytes) { return format_graph(BVG_TEXT_ARCS, g, from, to, shift, d_out, cap, nbytes, true); }

int bvg_text_format_csr(int kind, int64_t first_node, int64_t nodes, const uint64_t* adj_off, const int64_t* adj, int64_t shift,
                        void* out, uint64_t cap, uint64_t* nbytes) {
    if ((kind != BVG_TEXT_ASCII && kind != BVG_TEXT_ARCS) || first_node < 0 || nodes < 0 || !adj_off || !nbytes || shift == INT64_MIN) return BVG_E_ARG;
    if (nodes > INT64_MAX - first_node) return BVG_E_ARG;
    for (int64_t x = 0; x < nodes; x++) if (adj_off[x + 1] < adj_off[x]) return BVG_E_ARG;
    const uint64_t m = adj_off[nodes] - adj_off[0];
    if (m && !adj) return BVG_E_ARG;
    return guarded([&]() -> int {
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return BVG_E_HIP; }   // the calling thread's current device
        int r = ensure_device(device); if (r) return r;
        DevArray<uint64_t> off; DevArray<int64_t> a;
        if (off.alloc((size_t)nodes + 1) || a.alloc(m)) return BVG_E_NOMEM;
        HIPCHK(hipMemcpy(off.get(), adj_off, ((size_t)nodes + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (m) HIPCHK(hipMemcpy(a.get(), adj + adj_off[0], (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice));
        return format_dev(kind, first_node, nodes, off.get(), a.get(), m, kind == BVG_TEXT_ARCS ? shift : 0, out, cap, nbytes, false);
    });
}

}  // extern "C"
