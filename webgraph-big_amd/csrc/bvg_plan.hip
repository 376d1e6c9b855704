// bvg_plan.hip — host side: parameters and handles, the block plan, the packed offsets index, opening a graph (split off csrc/bvg_api.hip in round 6; see bvg_host.h).
//
// Mirrors the load path of the reference (ImmutableGraph.load -> BVGraph.loadInternal, BVGraph.java:1479-1574): bring .graph into memory (here: HBM), turn the
// .offsets gaps into an index (here: a packed device array instead of an Elias-Fano list), cut the node range into blocks of one wavefront each.
#include "bvg_host.h"

namespace bvghost {


Codings codings_of(const bvg_params& p) {
    Codings c; c.outdegree = p.outdegree_coding; c.block = p.block_coding; c.residual = p.residual_coding;
    c.reference = p.reference_coding; c.block_count = p.block_count_coding; c.zeta_k = p.zeta_k;
    return c;
}

int check_params(const bvg_params& p) {
    auto in = [](int v, std::initializer_list<int> s) { for (int x : s) if (x == v) return true; return false; };
    if (p.nodes < 0) return BVG_E_ARG;
    if (!in(p.outdegree_coding, {BVG_GAMMA, BVG_DELTA})) return BVG_E_UNSUPPORTED;                       // BVG:655-659
    if (!in(p.reference_coding, {BVG_UNARY, BVG_GAMMA, BVG_DELTA})) return BVG_E_UNSUPPORTED;            // BVG:695-700
    if (!in(p.block_count_coding, {BVG_UNARY, BVG_GAMMA, BVG_DELTA})) return BVG_E_UNSUPPORTED;          // BVG:729-734
    if (!in(p.block_coding, {BVG_UNARY, BVG_GAMMA, BVG_DELTA})) return BVG_E_UNSUPPORTED;                // BVG:759-764
    if (!in(p.residual_coding, {BVG_GAMMA, BVG_ZETA, BVG_DELTA, BVG_GOLOMB, BVG_NIBBLE})) return BVG_E_UNSUPPORTED;  // BVG:788-795
    if (!in(p.offset_coding, {BVG_GAMMA, BVG_DELTA})) return BVG_E_UNSUPPORTED;                          // BVG:628-632
    if (p.window_size < 0 || p.window_size > kMaxWindowBig) return BVG_E_UNSUPPORTED;
    if (p.min_interval_length < 0) return BVG_E_ARG;
    if (p.residual_coding == BVG_ZETA && (p.zeta_k < 1 || p.zeta_k > 32)) return BVG_E_ARG;
    return 0;
}

// Host-side MSB-first reader for the .offsets file only (one-off at load).

int read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return BVG_E_IO;
    fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize((size_t)sz);
    if (sz && fread(out.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return BVG_E_IO; }
    fclose(f);
    return 0;
}

int make_handle(Shared* sh, bvg_graph** out) {
    std::unique_ptr<bvg_graph> g(new bvg_graph());          // (a handle that fails half-way is deleted: its streams, events and arrays with it)
    g->sh = sh;
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        for (int i = 0; i < bvg_graph::kSide; i++) {
            HIPCHK(hipStreamCreateWithPriority(&g->side[i], hipStreamNonBlocking, knob("BVG_PRIO") ? (atoi(knob("BVG_PRIO")) > 0 ? greatest : atoi(knob("BVG_PRIO")) < 0 ? least : 0) : greatest));
            HIPCHK(hipEventCreateWithFlags(&g->side_ev[i], hipEventDisableTiming));
        }
    }
    HIPCHK(hipEventCreate(&g->ev0));
    HIPCHK(hipEventCreate(&g->ev1));
    g->fail_cap = 1u << 16;
    if (g->d_acc.alloc((size_t)kAccStripes * kAccStride) || g->d_fail.alloc(2 * (size_t)g->fail_cap + 1)) return BVG_E_NOMEM;   // stripe 0 of d_acc also holds the debug counters [4..19]
    *out = g.release();
    return 0;
}

void release_shared(Shared* sh) {
    if (sh->refs.fetch_sub(1) == 1) delete sh;
}

int ensure_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return BVG_E_HIP;
    HIPCHK(hipSetDevice(device));
    return 0;
}

uint64_t next_plan_version() { static std::atomic<uint64_t> v{1}; return v.fetch_add(1); }

// Builds the block plan: boundaries at ~equal compressed bits + per-block halo masks.
int build_plan(bvg_graph* g, uint32_t block_bits, std::shared_ptr<Plan>& out) {
    Shared* sh = g->sh;
    std::lock_guard<std::mutex> lk(sh->mu);
    {
        auto it = sh->plans.find(block_bits);
        if (it != sh->plans.end()) { out = it->second; return 0; }
    }
    struct WallClock { std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); ~WallClock() { if (dbg_on()) fprintf(stderr, "[bvg] block plan built in %.3f s (wall clock)\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); } } wall_clock;
    std::shared_ptr<Plan> np = std::make_shared<Plan>();
    Plan& plan = *np;
    plan.device = sh->device;
    plan.block_bits = block_bits;
    auto publish = [&]() { sh->plans.clear(); sh->plans[block_bits] = np; out = np; return 0; };
    const int64_t n = sh->p.nodes;
    if (n == 0) { plan.nblk = 0; plan.h_first.assign(1, 0); return publish(); }
    const uint64_t limit = sh->nbytes;
    uint64_t nb = (sh->total_bits + block_bits - 1) / block_bits;
    if (nb == 0) nb = 1;
    if (nb > 0x7FFFFFF0ull) return BVG_E_UNSUPPORTED;
    std::vector<uint64_t> first(nb + 1);
    {
        DevArray<uint64_t> d_first0;
        if (d_first0.alloc(nb + 1)) return BVG_E_NOMEM;
        launch_plan_boundaries(sh->offs, n, block_bits, nb, d_first0, g->stream);
        HIPCHK(hipMemcpyAsync(first.data(), d_first0, (nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
    }
    // drop empty blocks (a record longer than block_bits spans several targets)
    first[0] = 0;
    std::vector<uint64_t> uniq; uniq.reserve(first.size());
    for (size_t i = 0; i < first.size(); i++) if (uniq.empty() || first[i] != uniq.back()) uniq.push_back(first[i]);
    if (uniq.back() != (uint64_t)n) uniq.push_back((uint64_t)n);
    uint32_t nblk = (uint32_t)(uniq.size() - 1);
    // A record longer than the LDS stream window sends its whole block to the giant kernel, which walks a block node by node with the
    // whole workgroup: the ~50 ordinary nodes that share the block with it cost that kernel more than the long record itself (4.4 G-node
    // run: 157 k such blocks = 2.0 s of a scan whose tier 0 ends after 1.2 s).  Cut the block in front of the long record (it is the
    // block's last node or nearly: the record runs past the block's end), so that the nodes before it stay with the LDS kernels.
    if (!knob("BVG_NO_LONGCUT")) {
        DevArray<uint64_t> d_f, d_node, d_bits;
        if (d_f.alloc((size_t)nblk + 1) || d_node.alloc(nblk) || d_bits.alloc(nblk)) return BVG_E_NOMEM;
        HIPCHK(hipMemcpyAsync(d_f, uniq.data(), (nblk + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
        launch_plan_longest(sh->offs, d_f, nblk, d_node, d_bits, g->stream);
        std::vector<uint64_t> hn(nblk), hb(nblk);
        HIPCHK(hipMemcpyAsync(hn.data(), d_node, (size_t)nblk * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipMemcpyAsync(hb.data(), d_bits, (size_t)nblk * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        d_f.reset(); d_node.reset(); d_bits.reset();
        std::vector<uint64_t> cut; cut.reserve(uniq.size() + 1024);
        for (uint32_t k = 0; k < nblk; k++) {
            cut.push_back(uniq[k]);
            if (hb[k] + 128 > 32768 && hn[k] > uniq[k] && hn[k] < uniq[k + 1]) cut.push_back(hn[k]);
        }
        cut.push_back(uniq[nblk]);
        if (cut.size() - 1 <= 0x7FFFFFF0ull) { uniq.swap(cut); nblk = (uint32_t)(uniq.size() - 1); }
    }
    // halo per boundary; boundaries whose reference chains reach further back than kMaxHalo nodes are removed.
    // Two rounds: the first one's per-block list sizes show which blocks owe their LDS class (or the giant kernel) to ONE large list; those
    // are cut in front of that list and 2 W + 1 nodes behind it, so that only the few nodes around it run at the class's low occupancy and
    // the rest of the block goes back to tier 0 (the classes held 12 % of the blocks of the default workload and took 28 % of a scan).
    const bool refine = !knob("BVG_NO_LISTCUT") && sh->p.window_size <= kMaxWindow;
    for (int round = 0; round < 2; round++) {
      bool done = false;
      for (int pass = 0; pass < 2 && !done; pass++) {
        DevArray<uint64_t> d_first, d_mask; DevArray<uint32_t> d_halo;
        if (d_first.alloc((size_t)nblk + 1) || d_halo.alloc(nblk) || d_mask.alloc(nblk)) return BVG_E_NOMEM;
        HIPCHK(hipMemcpyAsync(d_first, uniq.data(), (nblk + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
        launch_plan_halo(sh->d_graph, limit, sh->offs, n, d_first, nblk, sh->p.window_size, codings_of(sh->p), d_halo, d_mask, g->stream);
        std::vector<uint32_t> halo(nblk);
        HIPCHK(hipMemcpyAsync(halo.data(), d_halo, (size_t)nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        bool any_bad = false;
        for (uint32_t k = 0; k < nblk; k++) if (halo[k] == 0xFFFFFFFFu) { any_bad = true; break; }
        if (!any_bad || pass == 1) {
            if (any_bad) return BVG_E_UNSUPPORTED;
            // per-block largest "list + window" (one wavefront per block), kept on the host to predict tiers; the block's longest list and its node
            const bool want_cuts = refine && round == 0;
            std::vector<uint32_t> maxd(nblk), bigd(want_cuts ? nblk : 0); std::vector<uint64_t> bign(want_cuts ? nblk : 0);
            {
                DevArray<uint32_t> d_maxd, d_bigd; DevArray<uint64_t> d_bign;      // (the last two stay null without cuts)
                if (d_maxd.alloc(nblk) || (want_cuts && (d_bign.alloc(nblk) || d_bigd.alloc(nblk)))) return BVG_E_NOMEM;
                launch_plan_maxd(sh->d_graph, limit, sh->offs, d_first, d_halo, nblk, sh->p.outdegree_coding, sh->p.window_size, d_maxd, d_bign, d_bigd, g->stream);
                hipError_t e2 = hipMemcpyAsync(maxd.data(), d_maxd, (size_t)nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream);
                if (e2 == hipSuccess && want_cuts) e2 = hipMemcpyAsync(bign.data(), d_bign, (size_t)nblk * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream);
                if (e2 == hipSuccess && want_cuts) e2 = hipMemcpyAsync(bigd.data(), d_bigd, (size_t)nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream);
                if (e2 == hipSuccess) e2 = hipStreamSynchronize(g->stream);
                if (e2 != hipSuccess) return BVG_E_HIP;
            }
            if (want_cuts) {
                // a block above the tier-0 capacity (about 2 000 elements of "worst list + window" / 2) with one list that is most of it
                const uint64_t W1 = knob("BVG_LISTCUT_BEHIND") ? (uint64_t)atoi(knob("BVG_LISTCUT_BEHIND")) : 2 * (uint64_t)sh->p.window_size + 1;   // (behind the list: W + 1 would do for the nodes that copy from it, but chains through them reach back as well: 8 / 15 / 22 nodes measured 251 / 255 / 254 G edges/s)
                std::vector<uint64_t> cut; cut.reserve(uniq.size() + 1024); size_t ncut = 0;
                for (uint32_t k = 0; k < nblk; k++) {
                    cut.push_back(uniq[k]);
                    const uint64_t md = maxd[k] & 0x7FFFFFFFu;
                    if (md / 2 + 64 > 1800 && bigd[k] >= (knob("BVG_LISTCUT_D") ? (uint32_t)atoi(knob("BVG_LISTCUT_D")) : 500u) && uniq[k + 1] - uniq[k] > 2 * W1 + 8) {
                        if (bign[k] > uniq[k] + 4) { cut.push_back(bign[k]); ncut++; }
                        if (bign[k] + W1 + 4 < uniq[k + 1]) { cut.push_back(bign[k] + W1); ncut++; }
                    }
                }
                cut.push_back(uniq[nblk]);
                if (ncut && cut.size() - 1 <= 0x7FFFFFF0ull) {
                    if (dbg_on()) fprintf(stderr, "[bvg] plan: %zu cuts around large lists (%u blocks before)\n", ncut, nblk);
                    uniq.swap(cut); nblk = (uint32_t)(uniq.size() - 1);
                    done = true;                                           // next round on the refined boundaries
                    continue;
                }
            }
            if (dbg_on()) {                                                // how many nodes the blocks decode a second time (their halos)
                std::vector<uint64_t> hm(nblk);
                if (hipMemcpy(hm.data(), d_mask, (size_t)nblk * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess) {
                    uint64_t hn = 0; for (uint32_t k = 0; k < nblk; k++) hn += (uint64_t)__builtin_popcountll(halo[k] ? hm[k] & (halo[k] >= 64 ? ~0ull : ((1ull << halo[k]) - 1ull)) : 0ull);
                    fprintf(stderr, "[bvg] plan: %u blocks, %llu halo nodes (%.1f %% of %lld nodes)\n", nblk, (unsigned long long)hn, 100.0 * (double)hn / (double)n, (long long)n);
                }
            }
            plan.d_first = std::move(d_first); plan.d_halo = std::move(d_halo); plan.d_mask = std::move(d_mask);
            plan.nblk = nblk; plan.h_first = uniq; plan.h_maxd.swap(maxd);
            plan.version = next_plan_version();
            return publish();
        }
        // merge blocks: drop un-cuttable boundaries (the halo of a kept boundary does not depend on the others)
        std::vector<uint64_t> kept; kept.reserve(uniq.size());
        for (uint32_t k = 0; k < nblk; k++) if (halo[k] != 0xFFFFFFFFu || k == 0) kept.push_back(uniq[k]);
        kept.push_back((uint64_t)n);
        uniq.swap(kept); nblk = (uint32_t)(uniq.size() - 1);
      }
      if (!done) break;
    }
    return BVG_E_UNSUPPORTED;
}

uint32_t block_bits_of(const bvg_graph* g) { return g->tun.block_bits ? g->tun.block_bits : kDefaultBlockBits; }


// one entry of the index on the host
int read_offset(const Shared* sh, int64_t x, uint64_t* out) {
    if (!sh->offs.lo) { HIPCHK(hipMemcpy(out, sh->offs.wide + x, sizeof(uint64_t), hipMemcpyDeviceToHost)); return 0; }
    uint32_t lo = 0; uint64_t hi = 0;
    HIPCHK(hipMemcpy(&lo, sh->offs.lo + x, sizeof lo, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hi, sh->offs.hi + (x >> kOffShift), sizeof hi, hipMemcpyDeviceToHost));
    *out = hi + lo;
    return 0;
}

// Packs the index (n+1 entries; on the device or on the host) into sh->offs.  1 = a distance does not fit 32 bits: the caller keeps
// the plain array.  A host array is staged through a 128 MiB device buffer, so the plain form never exists in HBM.
int pack_offsets(Shared* sh, const uint64_t* src_dev, const uint64_t* src_host) {
    const int64_t n1 = sh->p.nodes + 1, G = (int64_t)1 << kOffShift;
    DevArray<uint32_t> lo; DevArray<uint64_t> hi, stagebuf; DevArray<unsigned> ovf;
    if (lo.alloc((size_t)n1) || hi.alloc((size_t)((n1 + G - 1) / G + 1)) || ovf.alloc(1)) return BVG_E_NOMEM;
    HIPCHK(hipMemset(ovf, 0, sizeof(unsigned)));
    if (src_dev) launch_pack_offsets(src_dev, 0, n1, lo, hi, ovf, nullptr);
    else {
        const int64_t step = (int64_t)1 << 24;
        if (stagebuf.alloc((size_t)std::min<int64_t>(step, n1))) return BVG_E_NOMEM;
        for (int64_t first = 0; first < n1; first += step) {
            const int64_t cnt = std::min<int64_t>(step, n1 - first);
            HIPCHK(hipMemcpy(stagebuf, src_host + first, (size_t)cnt * sizeof(uint64_t), hipMemcpyHostToDevice));
            launch_pack_offsets(stagebuf, first, cnt, lo, hi, ovf, nullptr);
            HIPCHK(hipStreamSynchronize(nullptr));
        }
    }
    unsigned o = 0;
    HIPCHK(hipMemcpy(&o, ovf, sizeof o, hipMemcpyDeviceToHost));
    if (o) return 1;
    sh->d_off_lo = std::move(lo); sh->d_off_hi = std::move(hi);
    sh->offs = Offsets{sh->d_off_lo, sh->d_off_hi, nullptr};
    return 0;
}


int open_common(const bvg_params* p, const uint8_t* h_graph, const void* d_graph_in, uint64_t nbytes, const uint64_t* h_offsets,
                const void* d_offsets_in, int device, bvg_graph** out, PackedOffsets* packed) {
    if (!p || !out) return BVG_E_ARG;
    int r = check_params(*p); if (r) return r;
    r = ensure_device(device); if (r) return r;
    struct Release { void operator()(Shared* s) const { release_shared(s); } };
    std::unique_ptr<Shared, Release> owner(new Shared());   // released on every return but the last
    Shared* sh = owner.get();
    sh->device = device; sh->p = *p; sh->nbytes = nbytes;
    // 32-bit successor arithmetic holds every node id below 2^32 - 1 (0xFFFFFFFF is the lists' sentinel); the reference's own line between
    // the int and the long library is 2^31 because Java ints are signed -- nothing here is
    sh->wide = p->nodes > (int64_t)0xFFFFFF00ll || (knob("BVG_WIDE_FROM_2_31") != nullptr && p->nodes > (int64_t)0x7FFFFFFF);
    const int64_t n = p->nodes;
    if (d_graph_in) { sh->d_graph = (uint8_t*)d_graph_in; sh->padded = ((nbytes + 15) & ~15ull) + 16; }
    else {
        uint64_t padded = ((nbytes + 15) & ~15ull) + kPad;
        sh->padded = padded;
        r = sh->own_graph.alloc(padded); if (r) return r;
        sh->d_graph = sh->own_graph;
        HIPCHK(hipMemset(sh->d_graph, 0, padded));
        if (nbytes) HIPCHK(hipMemcpy(sh->d_graph, h_graph, nbytes, hipMemcpyHostToDevice));
    }
    // The index is kept packed (bvg_kernels.h: Offsets).  A caller's device array is packed into memory of our own and not referenced
    // afterwards; BVG_WIDE_OFFSETS=1 or a distance that does not fit 32 bits keeps the plain 64-bit form.
    const bool keep_wide = knob("BVG_WIDE_OFFSETS") != nullptr;
    if (packed) { sh->d_off_lo = std::move(packed->lo); sh->d_off_hi = std::move(packed->hi); sh->offs = Offsets{sh->d_off_lo, sh->d_off_hi, nullptr}; }
    else if (d_offsets_in) {
        int pk = keep_wide ? 1 : pack_offsets(sh, (const uint64_t*)d_offsets_in, nullptr);
        if (pk < 0) return pk;
        if (pk) sh->offs = Offsets{nullptr, nullptr, (const uint64_t*)d_offsets_in};
    } else if (h_offsets) {
        int pk = keep_wide ? 1 : pack_offsets(sh, nullptr, h_offsets);
        if (pk < 0) return pk;
        if (pk) {
            r = sh->own_wide.alloc((size_t)n + 1); if (r) return r;
            sh->offs = Offsets{nullptr, nullptr, sh->own_wide};
            HIPCHK(hipMemcpy(sh->own_wide, h_offsets, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
    } else {
        r = sh->own_wide.alloc((size_t)n + 1); if (r) return r;
        uint64_t* const d_wide = sh->own_wide;
        sh->offs = Offsets{nullptr, nullptr, d_wide};
        {
            // no .offsets (loadSequential / loadOffline, BVG:1345-1464; BVGraph -O, BVG:2595-2609): derive the index from
            // the stream itself with one sequential pass on the device
            DevArray<unsigned> d_err;
            r = d_err.alloc(1); if (r) return r;
            HIPCHK(hipMemset(d_err, 0, sizeof(unsigned)));
            // Default: the chunk-parallel walk of bvg_derive.hip (round 3: one code per lane and step, only changed chunks re-walked).
            // Fall-back -- windows > 127, any oddity in the stream, BVG_DERIVE_SEQ=1 -- is the one-wavefront sequential walk, whose error
            // bits are the documented ones.
            int rounds = 0;
            int pr = knob("BVG_DERIVE_SEQ") ? -1 : derive_offsets_parallel(sh->d_graph, nbytes, n, p->window_size, p->min_interval_length, codings_of(*p), d_wide, d_err, nullptr, &rounds);
            if (pr == 0) {
                unsigned e0 = 0;
                if (hipMemcpy(&e0, d_err, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return BVG_E_HIP;
                if (e0) { pr = -4; (void)hipMemset(d_err, 0, sizeof(unsigned)); }
            }
            if (dbg_on()) fprintf(stderr, "[bvg] derive offsets: parallel walk %s (%d rounds)\n", pr == 0 ? "ok" : "not used / failed", rounds);
            if (pr != 0) launch_derive_offsets(sh->d_graph, sh->padded, nbytes, n, p->window_size, p->min_interval_length, codings_of(*p), d_wide, d_err, nullptr);
            unsigned herr = 0;
            if (hipMemcpy(&herr, d_err, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return BVG_E_HIP;
            if (dbg_on()) { uint64_t last = 0; (void)hipMemcpy(&last, d_wide + n, 8, hipMemcpyDeviceToHost); fprintf(stderr, "[bvg] derive offsets: err=%u end=%llu of %llu bits\n", herr, (unsigned long long)last, (unsigned long long)nbytes * 8); }
            if (herr) return (herr & ERR_REF_RANGE) ? BVG_E_STATE : BVG_E_EOF;
        }
        int pk = keep_wide ? 1 : pack_offsets(sh, d_wide, nullptr);
        if (pk < 0) return pk;
        if (pk == 0) sh->own_wide.reset();
    }
    r = read_offset(sh, n, &sh->total_bits); if (r) return r;
    if (sh->total_bits > nbytes * 8) return BVG_E_EOF;
    r = make_handle(sh, out); if (r) return r;
    (void)owner.release();
    return 0;
}


// ---- arc-bounded batches: what bvg_components, the visits of bvg_bfs and the iterations of bvg_hyperball feed their kernels with

// per batch bound j: the prefix sum at the bound and at the node before it (the arcs of a segment without its last list)
__global__ void gather_bounds_kernel(const uint64_t* cum, const uint64_t* first, uint64_t nb, uint64_t* at, uint64_t* before) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nb + 1; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = first[j];
        at[j] = cum[b];
        before[j] = b ? cum[b - 1] : 0;
    }
}

// outdegrees of [from, to) into out[0, to - from): launch_outdegrees runs one work-item per node, so longer ranges go in pieces
void outdegrees_of(bvg_graph* g, int64_t from, int64_t to, int32_t* out) {
    Shared* sh = g->sh;
    for (int64_t a = from; a < to; a += kMaxBatchNodes)
        launch_outdegrees(sh->d_graph, sh->nbytes, sh->offs, a, std::min(to, a + kMaxBatchNodes), sh->p.outdegree_coding, out + (a - from), nullptr, g->stream);
}

// n lists whose prefix sums d_cum[0 .. n] (arcs = d_cum[n]) are on the device, cut into ranges [lo, hi) of at most `per` arcs each, except
// that a list longer than that forms a batch on its own.  The cut points are the lower bounds of j * per in the prefix sums
// (launch_plan_boundaries), so a segment holds < per arcs before its last list and is split before that list when the whole exceeds per.
int cut_batches(bvg_graph* g, const uint64_t* d_cum, int64_t n, uint64_t arcs, uint64_t per, std::vector<Batch>& out, uint64_t* longest_out) {
    *longest_out = 0;
    out.clear();
    if (arcs == 0) return 0;
    if (per == 0) per = 1;
    const uint64_t nb = (arcs + per - 1) / per;
    DevArray<uint64_t> first, at, before;
    if (first.alloc(nb + 1) || at.alloc(nb + 1) || before.alloc(nb + 1)) return BVG_E_NOMEM;
    uint64_t* const d_first = first; uint64_t* const d_at = at; uint64_t* const d_before = before;
    launch_plan_boundaries(Offsets{nullptr, nullptr, d_cum}, n, per, nb, d_first, g->stream);
    hipLaunchKernelGGL(gather_bounds_kernel, dim3(grid((int64_t)nb + 1, 256)), dim3(256), 0, g->stream, d_cum, (const uint64_t*)d_first, nb, d_at, d_before);
    std::vector<uint64_t> hf(nb + 1), ha(nb + 1), hb(nb + 1);
    HIPCHK(hipMemcpyAsync(hf.data(), d_first, (nb + 1) * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(ha.data(), d_at, (nb + 1) * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(hb.data(), d_before, (nb + 1) * 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    for (uint64_t j = 0; j < nb; j++) {
        const uint64_t b0 = hf[j], b1 = hf[j + 1];
        if (b1 <= b0) continue;
        const uint64_t all = ha[j + 1] - ha[j], last = ha[j + 1] - hb[j + 1];     // arcs of the segment, of its last list
        if (all <= per || b1 - b0 == 1) out.push_back(Batch{(int64_t)b0, (int64_t)b1, all});
        else { out.push_back(Batch{(int64_t)b0, (int64_t)b1 - 1, all - last}); out.push_back(Batch{(int64_t)b1 - 1, (int64_t)b1, last}); }
    }
    std::vector<Batch> cut;                                                  // (and at most kMaxBatchNodes nodes each: runs of empty lists)
    for (const Batch& b : out) {
        if (b.hi - b.lo <= kMaxBatchNodes) { cut.push_back(b); continue; }
        for (int64_t a = b.lo; a < b.hi; a += kMaxBatchNodes) cut.push_back(Batch{a, std::min(b.hi, a + kMaxBatchNodes), b.arcs});   // (arcs: a bound)
    }
    out.swap(cut);
    for (const Batch& b : out) if (b.arcs > *longest_out) *longest_out = b.arcs;
    return 0;
}

// [0, nodes) cut into node ranges that way: the whole graph's outdegrees and their prefix sums are computed on the device
int plan_batches(bvg_graph* g, uint64_t per, std::vector<Batch>& out, uint64_t* arcs_out, uint64_t* longest_out) {
    Shared* sh = g->sh; const int64_t n = sh->p.nodes;
    DevArray<int32_t> deg; DevArray<uint64_t> cum, tmp;
    if (deg.alloc((size_t)n) || cum.alloc((size_t)n + 1) || tmp.alloc(scan_tmp_elems(n))) return BVG_E_NOMEM;
    outdegrees_of(g, 0, n, deg);
    launch_exclusive_scan(deg, cum, n, tmp, g->stream);
    uint64_t arcs = 0;
    HIPCHK(hipMemcpyAsync(&arcs, cum + n, 8, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    *arcs_out = arcs;
    return cut_batches(g, cum, n, arcs, per, out, longest_out);
}

// ---- the sweep: the whole graph decoded in arc-bounded node ranges, each consumed at once by the caller's kernel

// The residual skip index first, for the whole graph (a no-op when it exists): batches below a quarter of the graph would not build it and
// would all run on the checking kernels.  A build that fails leaves the batches index-less, nothing worse.
void index_first(bvg_graph* g) {
    const int64_t n = g->sh->p.nodes;
    if (g->tun.no_index != 1 && n >= 4096) (void)bvg_build_index(g, 0, n, nullptr, nullptr);
}

// The arcs of a batch: half of what is free NOW (the caller's own arrays are allocated, the index is built), less headroom for the decode's own
// workspaces (256 MiB + 1/16), the node-side arrays of a batch and the planning pass (12 bytes per node); at most `cap`, at least 1.  The test knob
// `knob_name` (null: none) overrides it when > 0.
int arc_budget(int64_t n, uint64_t cap, const char* knob_name, uint64_t* per) {
    if (const char* k = knob_name ? knob(knob_name) : nullptr) { const long long v = atoll(k); if (v > 0) { *per = (uint64_t)v; return 0; } }
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const uint64_t head = (256ull << 20) + fr / 16 + (uint64_t)n * 12;
    *per = std::max<uint64_t>(1, std::min<uint64_t>(cap, fr > head ? (fr - head) / 2 / 8 : 1));
    return 0;
}

// plan_batches over the graph.  every_node: every node is in some batch -- the node ranges the plan leaves out (they hold no arcs) become
// batches of their own with arcs == 0 and at most kMaxBatchNodes nodes, which decode() does not decode (bvg_hyperball: every node has a
// counter to carry over and to count, its list empty or not).
int SweepPlan::build(bvg_graph* g, uint64_t per, bool all_nodes) {
    every_node = all_nodes;
    const int rc = plan_batches(g, per, batches, &arcs, &longest); if (rc) return rc;
    if (every_node) {
        std::vector<Batch> all;
        int64_t at = 0;
        auto gap = [&](int64_t to) { for (; at < to; at = std::min(to, at + kMaxBatchNodes)) all.push_back(Batch{at, std::min(to, at + kMaxBatchNodes), 0}); };
        for (const Batch& b : batches) { gap(b.lo); all.push_back(b); at = b.hi; }
        gap(g->sh->p.nodes);
        batches.swap(all);
    }
    maxn = 0; for (const Batch& b : batches) maxn = std::max(maxn, b.hi - b.lo);
    layout(0);
    return 0;
}

// the workspace of one batch, 256-byte aligned pieces: maxn + 1 prefix sums, the scan's scratch, maxn outdegrees, `extra_bytes` of the caller's
// (known once maxn is: bvg_hyperball's per-wavefront partials), then the successors of the largest batch
void SweepPlan::layout(size_t extra_bytes) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    o_tmp = al(((size_t)maxn + 1) * 8); o_deg = o_tmp + al(scan_tmp_elems(maxn) * 8); o_extra = o_deg + al((size_t)maxn * 4); o_succ = o_extra + al(extra_bytes);
    bytes = o_succ + (size_t)std::max<uint64_t>(longest, 1) * 8;
}

// the lists of batch b into the bound workspace, on g->stream: list i of node b.lo + i is succ()[cum()[i] .. cum()[i + 1])
int SweepPlan::decode(bvg_graph* g, const Batch& b) const {
    const int64_t cnt = b.hi - b.lo;
    if (every_node && b.arcs == 0) { HIPCHK(hipMemsetAsync(cum(), 0, ((size_t)cnt + 1) * 8, g->stream)); return 0; }   // (a range the plan left out: empty lists)
    int32_t* const deg = (int32_t*)(base + o_deg);
    outdegrees_of(g, b.lo, b.hi, deg);
    launch_exclusive_scan(deg, cum(), cnt, (uint64_t*)(base + o_tmp), g->stream);
    return run_decode(g, b.lo, b.hi, true, cum(), succ(), nullptr, nullptr);
}

// decode(b), unless b is the plan's only batch and is in the bound workspace already (nothing else is ever decoded into it: the batch stays
// resident until the next bind).  *decodes += 1 when a decode ran
int SweepPlan::load(bvg_graph* g, const Batch& b, uint64_t* decodes) {
    if (single() && resident) return 0;
    const int rc = decode(g, b); if (rc) return rc;
    ++*decodes; resident = single();
    return 0;
}


}  // namespace bvghost
