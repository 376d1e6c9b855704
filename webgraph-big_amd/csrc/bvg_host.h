// bvg_host.h — what the host-side translation units of libbvgraph_hip.so share (round 6: csrc/bvg_api.hip split into plan / index / tier scheduler / C entry points):
// the handle, the block plan, the residual skip index and the functions that cross the files.  Internal: nothing here is part of the C ABI (include/bvgraph_hip.h).
//   bvg_plan.hip    parameters, handles, the block plan (node blocks of ~4 KiB of stream, halos), the packed offsets, opening a graph; arc-bounded batches and
//                   the one sweep over the whole graph that the analytics share (below: "arc-bounded batches")
//   bvg_index.hip   (kernels) + bvg_index_host.hip: the residual skip index -- granularity, the build (counting pass, dense walk, validating pass), basename.bvgidx on disk
//   bvg_sched.hip   run_decode: the tier scheduler (tier 0 + LDS classes + giants launched side by side, fail-over, what a scan learns about its blocks)
//   bvg_api.hip     the extern "C" entry points
//   bvg_arcwalk.h   (not included here: device-only) how the kernels of the analytics walk the arcs of a decoded batch, the device half of that sweep
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "bvg_kernels.h"

using namespace bvg;

// the one check of a HIP call in host code: a bvg status out of the enclosing function (whatever it owns frees itself), HIP's last error cleared
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            if (dbg_on()) fprintf(stderr, "[bvg] %s -> %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            (void)hipGetLastError();                                                          \
            return _e == hipErrorOutOfMemory ? BVG_E_NOMEM : BVG_E_HIP;                         \
        }                                                                                     \
    } while (0)


namespace bvghost {


constexpr uint32_t kDefaultBlockBits = 32768;   // ~4 KiB of compressed stream per wavefront
constexpr uint64_t kPad = 64;                   // zero bytes after the stream (8-byte loads + record overruns)
constexpr uint32_t kGiantResident = 512;        // giant workgroups (512 threads, 88 registers: 2 wavefronts per SIMD each) that can be resident at once: 2 per CU
constexpr uint32_t kGiantSlots = 768;           // their work areas: half as many again (a free one always turns up)
static uint32_t giant_slots() { if (knob("BVG_GSLOTS")) { const int v = atoi(knob("BVG_GSLOTS")); if (v >= 1 && v <= 8192) return (uint32_t)v; } return kGiantSlots; }   // (experiments)

// ---- device memory: every block the host code allocates belongs to one of these two owners, which free it when they go out of scope or when the
// handle that holds them is deleted.  Nothing else calls hipMalloc / hipFree.  A failed allocation leaves the owner empty and HIP's last error cleared.

// a typed device array: move-only, freed on every return path
template <typename T> class DevArray {
    T* p_ = nullptr; size_t n_ = 0;
public:
    DevArray() = default; DevArray(const DevArray&) = delete; DevArray& operator=(const DevArray&) = delete;
    DevArray(DevArray&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevArray& operator=(DevArray&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    ~DevArray() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    // `count` elements (0: one) in place of what it held: 0 or BVG_E_NOMEM
    int alloc(size_t count) {
        reset();
        if (hipMalloc((void**)&p_, (count ? count : 1) * sizeof(T)) != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return BVG_E_NOMEM; }
        n_ = count;
        return 0;
    }
    void adopt(T* p, size_t count = 0) { reset(); p_ = p; n_ = count; }   // a block another function allocated and handed over
    T* release() { T* q = p_; p_ = nullptr; n_ = 0; return q; }            // ... and the way a block leaves: to the caller, or to another owner's adopt()
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }
};

// host memory that leaves through the C ABI is malloc'ed (the caller frees it with bvg_free): owned like this until it is released to the caller
struct HostFree { void operator()(void* p) const { free(p); } };
template <typename T> using HostArray = std::unique_ptr<T[], HostFree>;

// a workspace kept between calls, grown on demand and never shrunk.  reserve(): the block it holds when that is large enough; otherwise that block is freed first
// and one of `bytes` taken -- or, when that fails and the caller can do with less, one of `at_least`.  0 or BVG_E_NOMEM, and then it is empty.
class DevWorkspace {
    void* p_ = nullptr; size_t bytes_ = 0;
public:
    DevWorkspace() = default; DevWorkspace(const DevWorkspace&) = delete; DevWorkspace& operator=(const DevWorkspace&) = delete;
    ~DevWorkspace() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; bytes_ = 0; }
    int reserve(size_t bytes, size_t at_least = 0) {
        if (bytes <= bytes_) return 0;
        reset();
        for (size_t want : {bytes, at_least}) {
            if (!want) break;
            if (hipMalloc(&p_, want) == hipSuccess) { bytes_ = want; return 0; }
            p_ = nullptr; (void)hipGetLastError();
        }
        return BVG_E_NOMEM;
    }
    void* get() const { return p_; }
    char* at(size_t offset) const { return (char*)p_ + offset; }
    size_t bytes() const { return bytes_; }
};

// Residual skip index of the plan blocks [blk_lo, blk_hi) (a shard builds only its own blocks; everything outside has no entries and
// is decoded index-less).  Also the record of which blocks a VALIDATING pass of the row kernel has decoded from end to end
// (fmt[b] == 1): the lean scan kernel (bvg_scan.hip) takes only those.  Immutable once published.
struct SkipIndex {
    int device = 0;
    uint32_t blk_lo = 0, blk_hi = 0;
    uint64_t total = 0; DevArray<uint64_t> d_first; DevArray<uint16_t> d_bit; DevArray<uint8_t> d_val; DevArray<uint8_t> d_fmt;   // d_val: 32- or 64-bit values (`wide`)
    bool wide = false;                        // entries hold 64-bit values (built by the 64-bit kernels); a handle running the other width ignores the index
    uint32_t skip_min = kSkipMin, skip_shift = 4;   // granularity: lists of >= skip_min residuals hold one entry per 2^skip_shift residuals (skip_granularity() when it is built)
    bool failed = false;                      // the build of [blk_lo, blk_hi) failed: no arrays; scans of those blocks run index-less.  WHY it failed decides what happens next:
    enum { kStream = 1, kResources = 2 };     //   a stream the checking kernels refuse stays refused (only bvg_build_index tries again); running out of memory (or any other HIP
    int fail_cause = 0;                       //   error) is transient: the scans try again every kRetryEvery-th time.  Several failed ranges (two shards that alternate) are kept
    struct FailedRange { uint32_t lo, hi; int cause; };         // side by side, EACH WITH ITS OWN CAUSE (round 6), so that neither pays its counting pass again because of the
    std::vector<FailedRange> failed_ranges;                     // other, and a range that ran out of memory is retried whatever made another one fail (fail_cause: the latest)
    mutable std::atomic<uint32_t> backoff{0}; // scans left before the next automatic attempt (a failed snapshot with kResources; a good partial one whose whole-graph rebuild failed)
    static constexpr uint32_t kRetryEvery = 8;
    bool covers(uint32_t lo, uint32_t hi) const {
        if (!failed) return blk_lo <= lo && hi <= blk_hi;
        for (const auto& r : failed_ranges) if (r.lo <= lo && hi <= r.hi) return true;
        return false;
    }
    int cause_of(uint32_t lo, uint32_t hi) const {            // why the failed range that covers [lo, hi) failed (0: none does)
        for (const auto& r : failed_ranges) if (r.lo <= lo && hi <= r.hi) return r.cause;
        return 0;
    }
    uint64_t gen = 0;                         // identity of this snapshot: what a handle learned about blocks (tier lists, lean / row split) holds for ONE snapshot only
    std::vector<uint64_t> h_first;            // nblk + 1 entry indices (host copy: index_bytes of a range)
    std::vector<uint8_t> h_fmt;               // host copy of d_fmt: 1 = validated by the row kernel (the lean scan kernel may take the block)
    // recorded positions of the scan kernel's extras (DecodeArgs::pos_*; count_positions, bvg_index_host.hip): counted with the index, written by the first scans of every
    // block (pos_ready), never saved -- loading an index counts them again.  They live BEHIND the skip index's own data in its four arrays (the bit per node in
    // d_val, the per-block bases in d_first, the entries in d_bit, the flags in d_fmt): these point there.  nullptr: the scan kernel searches for the positions as before.
    uint32_t* pos_refd = nullptr; uint64_t* pos_first = nullptr; uint16_t* pos_ent = nullptr; uint8_t* pos_ready = nullptr;
    std::vector<uint64_t> h_pos_first;        // nblk + 1 entry indices (host copy: index_bytes of a range); empty = no recorded positions
    SkipIndex() = default; SkipIndex(const SkipIndex&) = delete; SkipIndex& operator=(const SkipIndex&) = delete;
    ~SkipIndex() { (void)hipSetDevice(device); }
};

struct Plan {
    uint32_t block_bits = 0;
    uint32_t nblk = 0;
    DevArray<uint64_t> d_first; DevArray<uint32_t> d_halo; DevArray<uint64_t> d_mask;
    std::vector<uint64_t> h_first;
    std::vector<uint32_t> h_maxd;             // largest (list + the W lists before it) a block decodes: predicts its tier
    uint64_t version = 0;
    // residual skip index: an immutable snapshot (SkipIndex below), replaced as a whole and read through atomic_load, so a scan
    // running on another thread keeps the arrays it started with
    std::shared_ptr<struct SkipIndex> skip;
    void release() {
        std::atomic_store(&skip, std::shared_ptr<struct SkipIndex>());
        d_first.reset(); d_halo.reset(); d_mask.reset(); nblk = 0; h_first.clear(); h_maxd.clear();
    }
    int device = 0;
    Plan() = default;
    Plan(const Plan&) = delete;
    Plan& operator=(const Plan&) = delete;
    ~Plan() { (void)hipSetDevice(device); release(); }
};

struct Shared {
    int device = 0;
    bvg_params p{};
    uint8_t* d_graph = nullptr; uint64_t nbytes = 0; uint64_t padded = 0; DevArray<uint8_t> own_graph;   // d_graph: what the kernels read; own_graph holds it unless it is the caller's (bvg_open_dev)
    // the offsets index: packed (owned: 4 bytes per node + 8 per 2^kOffShift nodes) or, as a fallback, the plain 64-bit array
    Offsets offs{nullptr, nullptr, nullptr};
    DevArray<uint32_t> d_off_lo; DevArray<uint64_t> d_off_hi; DevArray<uint64_t> own_wide;   // what offs points into (a caller's plain array is not held)
    uint64_t offsets_bytes() const { return offs.lo ? ((uint64_t)p.nodes + 1) * 4 + ((((uint64_t)p.nodes + 1) >> kOffShift) + 1) * 8 : ((uint64_t)p.nodes + 1) * 8; }
    uint64_t total_bits = 0;
    bool wide = false;
    // Block plans are immutable once built and shared by reference count: a handle holds the one it decodes with for the whole
    // call, so a bvg_copy() flyweight asking for another block size (bvg_set_tuning) on another thread can never free arrays
    // under a kernel in flight.  At most one plan per block size is kept; a new size evicts the others from the table (they
    // live on until their last user returns).  The residual skip index belongs to its plan and is published through
    // Plan::skip_state (release / acquire).
    std::map<uint32_t, std::shared_ptr<Plan>> plans; std::mutex mu; std::mutex skip_mu;
    // cached shard bounds (bvg_shard_bounds): key = (k << 2) | balance
    std::map<uint64_t, std::vector<int64_t>> shard_bounds; std::mutex shard_mu;
    std::atomic<int> refs{1};
    ~Shared() { (void)hipSetDevice(device); }
};


}  // namespace bvghost
using namespace bvghost;

struct bvg_graph {
    Shared* sh = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevArray<unsigned long long> d_acc;       // 4 result words + 8 debug counters
    DevArray<uint32_t> d_fail;                // [0] count, [1..] list
    uint32_t fail_cap = 0;
    uint64_t node_base = 0;
    bvg_tuning tun{};
    DevWorkspace slow_ws;                     // tier-2 (global-memory) pools, kept between calls
    // predicted tiers run concurrently with tier 0 on high-priority side streams (their few, long blocks are the critical path)
    static constexpr int kSide = 5;            // [0] giants (global-memory kernel), [1..4] one per LDS size class
    hipStream_t side[kSide] = {}; hipEvent_t side_ev[kSide] = {};
    DevWorkspace giant_ws; DevArray<uint32_t> d_gslots;   // work areas of the giant kernel: kGiantSlots slots + their busy flags
    DevWorkspace flow_ws; uint32_t flow_waves = 0;   // scratch of the flow scan kernel (bvg_flow.hip): one slice per resident wavefront
    DevWorkspace dr_ws;                       // bvg_decode_range / bvg_successors_batch workspace, kept between calls (grown on demand)
    DevWorkspace tr_ws;                       // bvg_transpose workspace, kept between calls
    size_t tr_o_cum = 0, tr_o_succ = 0;             // where the last transpose left the graph's own CSR in it (bvg_symmetrize)
    int skip_mode = 0; uint32_t* skip_cnt = nullptr;   // transient: set while this handle builds the skip index
    std::shared_ptr<SkipIndex> skip_building;          // transient: the index the fill pass (skip_mode 2) writes
    struct Pred {
        // the work lists, one after another in d_lists: the row kernel's tier 0 and LDS classes 1-4, giants, the generic kernel, the lean scan kernel's tier 0 and classes 1-4
        enum Slot : int { kRow0, kRowC1, kRowC2, kRowC3, kRowC4, kGiant, kGeneric, kLean0, kLeanC1, kLeanC2, kLeanC3, kLeanC4, kSlots };
        uint64_t plan_version = 0, skip_gen = 0; uint32_t lo = 0, n = 0, pool0 = 0, mode = 0; DevArray<uint32_t> d_lists; uint32_t count[kSlots] = {}; uint64_t giant_need = 0;
        size_t offset(int slot) const { size_t o = 0; for (int c = 0; c < slot; c++) o += count[c]; return o; }   // of the slot's list in d_lists
        std::vector<uint8_t> learned; std::vector<uint8_t> leanfail; uint64_t learned_version = 0, learned_gen = 0; uint32_t learned_pool0 = 0, learned_mode = 0; bool dirty = false;   // tier in which a mispredicted block finally succeeded: the next scans send it there directly
    } pred2[2];                                      // [0] scans, [1] materialising calls (round 6: a handle that alternates bvg_scan and bvg_decode_range keeps what it learned for each; one slot made every change of mode start from the prediction again)
    bvg_graph() = default; bvg_graph(const bvg_graph&) = delete; bvg_graph& operator=(const bvg_graph&) = delete;
    ~bvg_graph() {                                   // (the streams first; the arrays and workspaces above free themselves after it)
        if (sh) (void)hipSetDevice(sh->device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        for (int i = 0; i < kSide; i++) { if (side[i]) { (void)hipStreamSynchronize(side[i]); (void)hipStreamDestroy(side[i]); } if (side_ev[i]) (void)hipEventDestroy(side_ev[i]); }
    }
};

// a graph as a CSR in HBM: what the text parsers (bvg_text.hip) and the transforms (bvg_transform.hip) return
struct bvg_text {
    int device = 0;
    int64_t nodes = 0; uint64_t arcs = 0;
    DevArray<uint64_t> d_off;           // adj_off[nodes + 1]
    int64_t* d_adj = nullptr;           // adj[arcs], inside adj_base
    DevArray<int64_t> adj_base;
    DevArray<int64_t> ids;              // ids[nodes]: the identifier of every node (bvg_scattered.hip); empty for every other producer
    ~bvg_text() { (void)hipSetDevice(device); }
};

// arc labels stored as a bit stream, resident on the device (bvg_labels.hip; bvg_labelled.hip reads its class and decodes through it)
struct bvg_labels {
    int device = 0, kind = 0, width = 0;
    int64_t nodes = 0;
    uint64_t nbytes = 0, padded = 0;
    DevArray<uint8_t> d_stream;
    DevArray<uint64_t> d_offsets;
    hipStream_t stream = nullptr;
    DevArray<unsigned> d_err;
    DevWorkspace cum_ws, tmp_ws;              // the prefix sums of a range and the scan's scratch (grown on demand)
    ~bvg_labels() {
        (void)hipSetDevice(device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }
};

// an arc-labelled graph as a CSR in HBM (bvg_labelled.hip, bvg_lcompose.hip)
struct bvg_lgraph {
    std::unique_ptr<bvg_text> g;        // the underlying graph
    DevArray<int32_t> d_lab;            // labels[arcs], in successor order
    int kind = 0, width = 0;
};

namespace bvghost {

// No C++ exception may cross the C ABI (a JVM behind JNI would be torn down by std::terminate): entry points that allocate
// host memory run inside this guard.
template <typename F> static int guarded(F&& f) {
    try { return f(); }
    catch (const std::bad_alloc&) { return BVG_E_NOMEM; }
    catch (const std::length_error&) { return BVG_E_ARG; }
    catch (...) { return BVG_E_STATE; }
}

// the host's own bit reader (properties-side decoding of .offsets: bvg_decode_offsets, BVGraph.java:870-898)
struct HostBits {
    const uint8_t* p; uint64_t nbits, pos = 0; bool eof = false;
    uint64_t peek() const {
        uint64_t byte = pos >> 3, nb = nbits >> 3; uint64_t hi = 0; uint8_t nx = 0;
        for (int i = 0; i < 8; i++) hi = (hi << 8) | (byte + i < nb ? p[byte + i] : 0);
        nx = byte + 8 < nb ? p[byte + 8] : 0;
        unsigned sh = (unsigned)(pos & 7);
        return sh ? (hi << sh) | ((uint64_t)nx >> (8 - sh)) : hi;
    }
    uint64_t bits(unsigned n) { if (!n) return 0; uint64_t w = peek(); pos += n; if (pos > nbits) eof = true; return w >> (64 - n); }
    uint64_t unary() {
        uint64_t z = 0;
        for (;;) {
            uint64_t w = peek();
            if (w) { unsigned lz = (unsigned)__builtin_clzll(w); pos += lz + 1; if (pos > nbits) eof = true; return z + lz; }
            pos += 64; z += 64;
            if (pos >= nbits) { eof = true; return z; }
        }
    }
    uint64_t gamma() { uint64_t m = unary(); if (m > 63) { eof = true; return 0; } return ((1ull << m) | bits((unsigned)m)) - 1; }
    uint64_t delta() { uint64_t m = gamma(); if (m > 63) { eof = true; return 0; } return ((1ull << m) | bits((unsigned)m)) - 1; }
};

struct PackedOffsets { DevArray<uint32_t> lo; DevArray<uint64_t> hi; };   // bvg_tile hands over an index it wrote in packed form: open_common takes the arrays out of it

// ---- bvg_plan.hip
uint64_t next_plan_version();
uint32_t block_bits_of(const bvg_graph* g);
int open_common(const bvg_params* p, const uint8_t* h_graph, const void* d_graph_in, uint64_t nbytes, const uint64_t* h_offsets,
                const void* d_offsets_in, int device, bvg_graph** out, PackedOffsets* packed = nullptr);
Codings codings_of(const bvg_params& p);
int check_params(const bvg_params& p);
int read_file(const std::string& path, std::vector<uint8_t>& out);
int make_handle(Shared* sh, bvg_graph** out);
void release_shared(Shared* sh);
int ensure_device(int device);
int build_plan(bvg_graph* g, uint32_t block_bits, std::shared_ptr<Plan>& out);
int read_offset(const Shared* sh, int64_t x, uint64_t* out);
int pack_offsets(Shared* sh, const uint64_t* src_dev, const uint64_t* src_host);

// ---- bvg_sched.hip
// Runs the decode kernel over the blocks intersecting [from,to); slow-path relaunches included.
// `batch` != nullptr: the blocks are the even entries of a per-call plan (one request each, bvg_successors_batch).
struct BatchPlan { const uint64_t* d_first; const uint32_t* d_halo; const uint64_t* d_mask; uint32_t requests; };

int run_decode(bvg_graph* g, int64_t from, int64_t to, bool materialise, const uint64_t* d_cum, int64_t* d_succ, int32_t* d_outdeg,
               bvg_scan_result* res, const BatchPlan* batch = nullptr, const std::shared_ptr<Plan>* use_plan = nullptr);

// ---- what the kernels of the analytics (bvg_components, bvg_bfs, bvg_hyperball) are launched with
// Every such kernel strides over its elements: a launch holds fewer than 2^32 work-items, and graphs may have more nodes than that.
#define BVG_FOR(I, N) for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < (int64_t)(N); I += (int64_t)gridDim.x * blockDim.x)
inline unsigned grid(int64_t n, int64_t per) { const int64_t b = (n + per - 1) / per; return (unsigned)(b < 1 ? 1 : (b > (1 << 18) ? (1 << 18) : b)); }   // (the kernels stride)

// an entry point of an object that holds a bvg_copy() flyweight in ->g (bvg_bfs, bvg_hyperball): the guard, and the graph's device made current
template <typename O, typename F> static int on_device(O* o, F&& f) {
    if (!o) return BVG_E_ARG;
    return guarded([&]() -> int {
        HIPCHK(hipSetDevice(o->g->sh->device));
        return f();
    });
}

// wall clock of the BVG_DEBUG splits (decode / consume): the milliseconds since the last lap
struct Stopwatch {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap() { const auto u = std::chrono::steady_clock::now(); const double ms = std::chrono::duration<double, std::milli>(u - t).count(); t = u; return ms; }
};

// ---- bvg_plan.hip: arc-bounded batches.  The graph (or any list of lists with prefix sums on the device) cut into ranges of at most `per` arcs, and
// the sweep over the whole compressed graph in such ranges that bvg_components, the sweep route of bvg_bfs_visit and bvg_hyperball_iterate
// share: index_first, arc_budget, then a SweepPlan and per batch SweepPlan::decode followed by the caller's own kernel (bvg_arcwalk.h: how the
// kernels that consume a batch arc by arc walk it).  A caller that sweeps many times (bvg_scc, bvg_geometric) calls SweepPlan::load instead: a
// plan of one batch stays resident in the workspace and is decoded once.  The caller owns the
// workspace (components: per call, freed before the numbering pass; bfs: grown on demand; hyperball: once per plan) and the order of these
// steps against its own allocations, which decides how much memory a batch takes on a full card.
constexpr int64_t kMaxBatchNodes = 1ll << 30;      // node ranges of a launch stay well below 2^32 work-items
constexpr uint64_t kMaxBatchArcs = 1ull << 32;     // 32 GiB of successors: the per-batch overhead (a plan lookup, two syncs) is already negligible
struct Batch { int64_t lo, hi; uint64_t arcs; };
void outdegrees_of(bvg_graph* g, int64_t from, int64_t to, int32_t* out);
int cut_batches(bvg_graph* g, const uint64_t* d_cum, int64_t n, uint64_t arcs, uint64_t per, std::vector<Batch>& out, uint64_t* longest_out);
int plan_batches(bvg_graph* g, uint64_t per, std::vector<Batch>& out, uint64_t* arcs_out, uint64_t* longest_out);
void index_first(bvg_graph* g);
int arc_budget(int64_t n, uint64_t cap, const char* knob_name, uint64_t* per);
struct SweepPlan {
    std::vector<Batch> batches; uint64_t arcs = 0, longest = 0; int64_t maxn = 0;   // maxn: nodes of the widest batch
    bool every_node = false;
    size_t o_tmp = 0, o_deg = 0, o_extra = 0, o_succ = 0, bytes = 0;                 // the workspace: cum (at 0), scan tmp, deg, extra, `longest` successors
    char* base = nullptr;
    int build(bvg_graph* g, uint64_t per, bool every_node = false);
    void layout(size_t extra_bytes);
    bool resident = false;                                                           // the plan's one batch is decoded in the bound workspace
    void bind(void* ws) { base = (char*)ws; resident = false; }
    bool single() const { return batches.size() == 1; }
    uint64_t* cum() const { return (uint64_t*)base; }
    int64_t* succ() const { return (int64_t*)(base + o_succ); }
    void* extra() const { return base + o_extra; }
    int decode(bvg_graph* g, const Batch& b) const;
    int load(bvg_graph* g, const Batch& b, uint64_t* decodes);
};

// ---- bvg_components.hip: the numbering that bvg_components and bvg_scc share.  d_parent (uint32 per node, uint64 when `wide`) holds trees whose roots
// are the smallest nodes of their components (bvg_scc: parent[x] is that node already).  comp[x] = the rank of x's root among the roots; sizes and,
// with BVG_CC_SORT_BY_SIZE in `flags`, the renumbering by decreasing size, as bvg_components documents them.  Needs 12 bytes per node of its own.
// Returns 0 or BVG_E_CAPACITY (sizes_cap below the count: comp and the count are written all the same); *count_out: the count.
int number_components(bvg_graph* g, void* d_parent, bool wide, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components, bool dev,
                      uint64_t* count_out);

// ---- bvg_api.hip: what bvg_successors_batch and the frontier route of bvg_bfs_visit share (described there)
int decode_range_impl(bvg_graph* g, int64_t from, int64_t to, int32_t* outdeg, int64_t* succ, uint64_t cap, uint64_t* n_succ, bool dev, bool narrow = false);
constexpr int64_t kMaxBatchRequests = 0x3FFFFFFF;
struct BatchBufs { int32_t* deg; uint64_t* first; uint64_t* cum; uint64_t* tmp; uint32_t* halo; uint64_t* mask; uint64_t* deep; size_t end; };   // device arrays of one batch; end: their bytes
struct DeepRequest { int64_t index; uint64_t at, arcs; };                  // request `index`: its list belongs at d_succ + at and holds `arcs` successors
size_t batch_bufs_bytes(int64_t count);
BatchBufs batch_bufs_at(char* base, int64_t count);
int batch_degrees(bvg_graph* g, const BatchBufs& b, const int64_t* d_nodes, int64_t count, uint64_t* total);
int batch_halos(bvg_graph* g, const BatchBufs& b, const int64_t* d_nodes, int64_t count, std::vector<DeepRequest>& deep);
int batch_decode(bvg_graph* g, const BatchBufs& b, int64_t count, int64_t* d_succ);

// The granularity of a graph's skip index: lists of >= `smin` residuals hold one entry per 2^shift residuals.  A residual pass lasts as long as its longest task, so the
// threshold matters as much as the spacing: 16 / 16 (a list of 16-23 residuals is two tasks instead of one of up to 23 steps) gains on every shape over rounds 1-3's 24 / 16
// -- w0 +7.2 %, uk +3.8 %, web +2.6 %, eu +1.5 %, eu15 +1.0 % -- for 0.1-8 % more entries.  A sparse graph's pass holds few tasks, and one entry per 8 residuals from
// lists of 8 on shortens it further: web +11.5 %, uk +5.1 %, cnr-2000 +2.3 % over 24 / 16, for 0.1-0.3 GB of entries per GB of stream; on the dense default workload 8 / 8
// is no faster than 16 / 16 and takes +80 % of an index that is half the stream already, on the reference-free w0 neither (its lists are residuals only: +30 % of resident
// bytes) -- profiles/r04_skipgran3.txt.  So: 8 / 8 below 40 arcs per node (128 bits per node when the arc count is unknown) when the graph has references, else 16 / 16.

// ---- bvg_text.hip: np (source, target) pairs on the device -> the CSR of `t` with `nodes` nodes (sorted, duplicates once; a pair whose ends are both
// `nodes` is dropped).  s0 / d0 are used up.  Fewer than 2^31 pairs (BVG_E_UNSUPPORTED beyond), at most 2^40 nodes (BVG_E_NOMEM).
int pairs_to_csr(DevArray<uint64_t>& s0, DevArray<uint64_t>& d0, uint64_t np, int64_t nodes, bvg_text* t);

// ---- bvg_transform.hip: the sources of the graph-to-graph calls (bvg_transform_*, bvg_compose).  A bvg_text is used where it lies; a bvg_graph is
// decoded once into a CSR of its own (`own`) and checked as bvg_store checks its input; a node base other than 0 is BVG_E_ARG.
struct Source {
    int device = 0; int64_t n = 0; uint64_t m = 0; const uint64_t* off = nullptr; const int64_t* adj = nullptr;
    std::unique_ptr<bvg_text> own;          // a decoded bvg_graph
};
bool one_source(const bvg_transform_src* s);                                        // exactly one of the two handles is set
int source_device(const bvg_transform_src* s);
int resolve(const bvg_transform_src* s, Source& r);
std::unique_ptr<bvg_text> new_csr(int device);
int check_csr(const uint64_t* d_off, const int64_t* d_adj, int64_t n, int refused);   // 0, or `refused` when the CSR is not one bvg_store would take
int finish(std::unique_ptr<bvg_text>& t, bvg_text** out);                            // the device drained, then *out

// ---- bvg_index_host.hip
void skip_granularity(const Shared* sh, uint32_t& smin, uint32_t& shift);
int build_skip(bvg_graph* g, const std::shared_ptr<Plan>& plp, uint32_t blo, uint32_t bhi, bool retry_failed = false, bvg_scan_result* first_scan = nullptr, int64_t sfrom = 0, int64_t sto = 0, bool* first_scan_done = nullptr);
int save_index_impl(bvg_graph* g, const char* path);
int load_index_impl(bvg_graph* g, const char* path);

}  // namespace bvghost
