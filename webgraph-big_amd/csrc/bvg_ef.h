// bvg_ef.h — the layout of an EFGraph record (reference: src/it/unimi/dsi/big/webgraph/EFGraph.java, "EF" below) as a closed form of its
// outdegree, and bounded reads of its LSB-first stream of 64-bit words.  Shared by the host (offsets derivation at load) and the kernels
// of bvg_ef.hip, so both sides compute one geometry.
//
// Record of a node with outdegree d, upper bound U, quantum 2^q; the list is stored with a terminator equal to U, so L = d + 1 elements:
//   gamma(d)                       EF:394-406: with v = d + 1, m = msb(v): m zero bits, a one bit, the low m bits of v
//   P = (U >> l) >> q pointers     EF:165-168, of ps = max(0, ceilLog2(L + (U >> l))) bits each (EF:152-154); pointer k (from 1) = k 2^q + the number
//                                  of elements whose high part is below k 2^q: the position just past the (k 2^q)-th zero of the upper bits (EF:511-513)
//   L lower fields of l bits       l = max(0, msb(U / L)) (EF:140-142)
//   (U >> l) + d + 1 upper bits    bit (e_i >> l) + i set for element i; the terminator's bit is the last one, which fixes the length
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bvgef {

__host__ __device__ __forceinline__ int ef_msb(uint64_t x) { return x ? 63 - __builtin_clzll(x) : -1; }

struct EfGeom {
    uint32_t l, ps, glen;        // lower bits per element, pointer width, bits of gamma(d)
    uint64_t P;                  // pointers
    uint64_t ptr, lower, upper;  // bit positions of the three parts
    uint64_t upper_len, end;     // bits of the upper part; the record's end
};

// msb(U / L) without the division: floor(log2(U / L)) is msb(U) - msb(L), or one less when L shifted up by that passes U
__host__ __device__ __forceinline__ uint32_t ef_lower_bits(uint64_t L, uint64_t U) {
    const int c = ef_msb(U) - ef_msb(L);
    if (c < 0) return 0;
    if ((L << c) <= U) return (uint32_t)c;
    return c > 0 ? (uint32_t)(c - 1) : 0;
}

__host__ __device__ __forceinline__ EfGeom ef_geom(uint64_t off, uint64_t d, uint64_t U, uint32_t q) {
    EfGeom g;
    const uint64_t L = d + 1;
    g.l = ef_lower_bits(L, U);
    const uint64_t zeros = U >> g.l, v = L + zeros;
    g.ps = v <= 1 ? 0 : (uint32_t)(64 - __builtin_clzll(v - 1));
    g.P = zeros >> q;
    g.glen = 2 * (uint32_t)ef_msb(L) + 1;
    g.ptr = off + g.glen;
    g.lower = g.ptr + g.P * g.ps;
    g.upper = g.lower + L * g.l;
    g.upper_len = zeros + L;
    g.end = g.upper + g.upper_len;
    return g;
}

// every read is bounded by the stream's word count: a word past the end reads as zero
__host__ __device__ __forceinline__ uint64_t ef_word(const uint64_t* w, uint64_t nwords, uint64_t i) { return i < nwords ? w[i] : 0; }

// `width` (0..64) bits at bit position pos, least significant bit first (EF:852-958)
__host__ __device__ __forceinline__ uint64_t ef_bits(const uint64_t* w, uint64_t nwords, uint64_t pos, uint32_t width) {
    if (!width) return 0;
    const uint64_t i = pos >> 6; const uint32_t s = (uint32_t)(pos & 63);
    uint64_t v = ef_word(w, nwords, i) >> s;
    if (s + width > 64) v |= ef_word(w, nwords, i + 1) << (64 - s);
    return width == 64 ? v : v & ((1ull << width) - 1);
}

// gamma(d) at pos (EF:960-989); the unary part may cross one word edge.  0 = read, 1 = the stream runs out or the code is longer than any
// outdegree's, 2 = an outdegree of 2^31 or more
__host__ __device__ __forceinline__ int ef_read_gamma(const uint64_t* w, uint64_t nwords, uint64_t pos, uint64_t* d) {
    const uint64_t i = pos >> 6; const uint32_t s = (uint32_t)(pos & 63);
    if (i >= nwords) return 1;
    uint64_t v = w[i] >> s; uint32_t m;
    if (v) m = (uint32_t)__builtin_ctzll(v);
    else {
        v = ef_word(w, nwords, i + 1);
        if (!v) return 1;
        m = 64 - s + (uint32_t)__builtin_ctzll(v);
    }
    if (m > 63) return 1;
    if (m > 31) return 2;
    const uint64_t val = ((1ull << m) | ef_bits(w, nwords, pos + m + 1, m)) - 1;
    if (val > 0x7FFFFFFFull) return 2;
    *d = val;
    return 0;
}

}  // namespace bvgef
