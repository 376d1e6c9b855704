// bvg_text_shared.h — what the two text parsers share: bvg_text.hip (ASCIIGraph and arc lists of node numbers) and
// bvg_scattered.hip (arc lists of arbitrary identifiers, 7n).  The tiling of the text (kTile bytes per workgroup, kChunk per lane), the
// line-break rule, a lane's bytes (Chunk), the workgroup scan, the line events of a tile and the comment state every tile starts in, the
// one 64-bit minimum that reports go into, and the line number of a byte offset.  Internal.
#pragma once
#include <cstdint>
#include <cstring>

#include "bvg_host.h"

namespace bvghost {
namespace {

constexpr int kThreads = 256, kChunk = 16;
constexpr uint64_t kTile = (uint64_t)kThreads * kChunk;            // 4096 bytes of text per workgroup
constexpr uint64_t kNoError = ~0ull;

enum : unsigned { kEvBreak = 0, kEvComment = 1, kEvNone = 2 };

// '\r' always breaks a line; '\n' does unless it follows '\r' (then it is a separator)
__device__ __forceinline__ bool is_break(unsigned c, unsigned prev) { return c == '\r' || (c == '\n' && prev != '\r'); }
__device__ __forceinline__ void report(unsigned long long* err, uint64_t byte, unsigned reason) { atomicMin(err, (unsigned long long)(byte << 4 | reason)); }

// inclusive scan over the workgroup's lanes (Hillis-Steele in LDS); `sum` for counts, else "the last value that is not kEvNone"
template <bool SUM>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds) {
    const unsigned t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < kThreads; d <<= 1) {
        const uint32_t left = t >= d ? lds[t - d] : (SUM ? 0u : (uint32_t)kEvNone);
        __syncthreads();
        v = SUM ? v + left : (v == kEvNone ? left : v);
        lds[t] = v;
        __syncthreads();
    }
    return v;
}

// The bytes of one lane: text[base .. base + kChunk) cut at nbytes, with the byte before them (a line feed before byte 0, so byte 0
// starts a line and a token like any other).
struct Chunk {
    unsigned char b[kChunk]; unsigned prev; int len;
    __device__ __forceinline__ void load(const uint8_t* text, uint64_t nbytes, uint64_t base) {
        len = base >= nbytes ? 0 : (nbytes - base < (uint64_t)kChunk ? (int)(nbytes - base) : kChunk);
        prev = base == 0 || base > nbytes ? '\n' : text[base - 1];
        if (len == kChunk && ((uintptr_t)(text + base) & 15u) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(text + base);
            memcpy(b, &q, 16);
        } else {
#pragma unroll
            for (int i = 0; i < kChunk; i++) b[i] = i < len ? text[base + i] : (unsigned char)' ';
        }
    }
};

// the last line event of the chunk
__device__ __forceinline__ unsigned chunk_event(const Chunk& c) {
    unsigned ev = kEvNone, prev = c.prev;
#pragma unroll
    for (int i = 0; i < kChunk; i++) {
        const unsigned ch = c.b[i];
        if (i < c.len) {
            if (is_break(ch, prev)) ev = kEvBreak;
            else if (ch == '#' && (prev == '\r' || prev == '\n')) ev = kEvComment;
        }
        prev = ch;
    }
    return ev;
}

// whether the lane's first byte lies in a comment line: the last event before it in the tile, or the state the tile starts in
__device__ __forceinline__ bool lane_in_comment(const Chunk& c, const uint8_t* state_in, uint64_t tile, uint32_t* lds) {
    const uint32_t incl = block_scan<false>(chunk_event(c), lds);
    __syncthreads();
    lds[threadIdx.x] = incl;
    __syncthreads();
    const uint32_t before = threadIdx.x ? lds[threadIdx.x - 1] : (uint32_t)kEvNone;
    const bool comment = (before == kEvNone ? (unsigned)state_in[tile] : before) == kEvComment;
    __syncthreads();
    return comment;
}

// T0
__global__ void __launch_bounds__(kThreads) text_events_kernel(const uint8_t* text, uint64_t nbytes, uint8_t* tile_ev) {
    __shared__ uint32_t lds[kThreads];
    Chunk c; c.load(text, nbytes, (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kChunk);
    const uint32_t ev = block_scan<false>(chunk_event(c), lds);
    if (threadIdx.x == kThreads - 1) tile_ev[blockIdx.x] = (uint8_t)ev;
}
// the state a tile starts in: the last event before it.  ONE workgroup scans the tiles kThreads at a time and carries the last event on:
// linear in the tiles whatever the text (a line of gigabytes is a run of tiles without an event)
__global__ void __launch_bounds__(kThreads) text_state_kernel(const uint8_t* tile_ev, uint64_t tiles, uint8_t* state_in) {
    __shared__ uint32_t lds[kThreads];
    uint32_t carry = kEvBreak;
    for (uint64_t base = 0; base < tiles; base += kThreads) {
        const uint64_t t = base + threadIdx.x;
        (void)block_scan<false>(t < tiles ? (uint32_t)tile_ev[t] : (uint32_t)kEvNone, lds);    // leaves the inclusive values in lds
        const uint32_t before = threadIdx.x ? lds[threadIdx.x - 1] : (uint32_t)kEvNone, last = lds[kThreads - 1];
        if (t < tiles) state_in[t] = (uint8_t)(before == kEvNone ? carry : before);
        if (last != kEvNone) carry = last;
        __syncthreads();
    }
}

// error path: 1 + the line breaks before byte `end`
__global__ void text_count_breaks_kernel(const uint8_t* text, uint64_t end, unsigned long long* out) {
    unsigned long long c = 0;
    BVG_FOR(i, end) { const unsigned ch = text[i]; if (is_break(ch, i ? text[i - 1] : '\n')) c++; }
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(out, c);
}

// the 1-based line of a byte offset, counted on the device (error path only)
int line_of(const uint8_t* d_text, uint64_t byte, unsigned long long* d_scratch, int64_t* line) {
    unsigned long long breaks = 0;
    HIPCHK(hipMemset(d_scratch, 0, sizeof(unsigned long long)));
    if (byte) hipLaunchKernelGGL(text_count_breaks_kernel, dim3(grid((int64_t)byte, 256 * 16)), dim3(256), 0, 0, d_text, byte, d_scratch);
    HIPCHK(hipMemcpy(&breaks, d_scratch, sizeof breaks, hipMemcpyDeviceToHost));
    *line = (int64_t)breaks + 1;
    return 0;
}

}  // namespace
}  // namespace bvghost
