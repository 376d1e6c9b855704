// bvg_sched.hip — run_decode: the tier scheduler of a scan / decode of a node range (split off csrc/bvg_api.hip in round 6; see bvg_host.h).
//
// The blocks of the plan are predicted into {tier 0, four LDS size classes, giants} by the largest list they hold and launched side by side; what a tier refuses goes to
// the next (learned per block, so later scans launch it there); validated blocks run the lean scan kernel (bvg_scan.hip), the others the checking row kernel.
#include "bvg_host.h"

namespace bvghost {

using Pred = bvg_graph::Pred;

// LDS size classes, in elements: the row kernel's tier 1 (elements of the graph's width: 127 KB of LDS for the largest class of the 64-bit row kernel -- it is what
// VALIDATES such a block for the scan kernel) and the lean scan kernel's classes (32-bit elements on every graph: block-relative ids beyond 2^32 nodes).
constexpr uint32_t kMaxPool = 12288;
constexpr uint32_t kClasses[4] = {kMaxPool / 6, kMaxPool / 3, (kMaxPool * 2) / 3, kMaxPool};
// LDS geometry of the lean classes (round 4): windows of 256 / 384 / 512 / 768 dwords and scratch areas of 384 / 512 / 1 024 / 2 048 elements instead of
// 1 024 dwords and >= 1 024 elements throughout -- resident wavefronts per CU 9 -> 14 / 6 -> 8 / 3 -> 4 in the three populated classes; alone on the chip
// they take 53.3 instead of 63.3 ms, in the concurrent schedule the scan gains 1.9 % (profiles/r04_serial_classes.txt, r04_ab_prio.txt); the few
// blocks whose longest record no longer fits the window fail over to the row kernel's classes (1 821 of 774 k)
constexpr uint32_t kLeanStage[4] = {256, 384, 512, 768}, kLeanScr[4] = {384, 512, 1024, 2048};

// The scheduler's switches (tests and experiments: live with BVG_TEST_KNOBS only), read at the start of every call.  0 means unset where the clamp excludes it.
struct Knobs {
    int giant = -1;                         // BVG_GIANT: 0 no giant kernel, 2 every block through it
    bool noskip = false, nostripe = false, nopredict = false, no_w18 = false, mat_lean = false, scank_off = false;   // BVG_NOSKIP ... BVG_SCANK=0
    uint32_t dbg = 0, pass_cost = 10, xcds = 8; uint64_t wide_half = 0x80000000ull;   // BVG_DBG, BVG_PASSCOST, BVG_XCDS, BVG_WIDE_HALF
    int emit = -1;                          // BVG_EMIT: task emission on (1) / off (0)
    uint32_t stage = 0;                     // BVG_STAGE: tier 0's stream window, dwords (64 ... 2048)
    bool pool_set = false; uint64_t pool = 0, waves = 0;   // BVG_POOL: tier 0's list pool; BVG_WAVES: the resident wavefronts per CU it aims at
    int wg = 0, wgc = 0, flow = 0, flat = 0; uint64_t wg_blocks = 0; uint32_t flow_ring = 1536, flat_recs = 0;   // the experiments (select_experiments)
    uint64_t scan_scr = 448, scan_waves = 0, scan_pool = 0; uint32_t scan_stage = 0; double scan_lists = 20.0;   // BVG_SCAN_*: the lean scan kernel's geometry (lists: window lists + a sub-row's stored lists and parked residuals)
    double admit = 0.3;                     // BVG_ADMIT: share of a block's worst "list + window" that tier 0 of the scan kernel must hold
    double cadmit = 0.75;                   // BVG_CADMIT: the same optimism for the lean classes (a block that fails its class is learned upward): +0.8 % on the default workload (profiles/r05_ab_cadmit.txt)
    uint32_t gbatch = 0;                    // BVG_GBATCH: giants in batched launches of this many, one area per block
    bool tier0_first = false, t0wait = false, serial = false, flat_prof = false; int side2 = 0;   // BVG_ORDER=1, BVG_T0WAIT=1, BVG_SERIAL, BVG_FLAT_PROF, BVG_SIDE2
    uint32_t class_stage[4] = {kLeanStage[0], kLeanStage[1], kLeanStage[2], kLeanStage[3]}, class_scr[4] = {kLeanScr[0], kLeanScr[1], kLeanScr[2], kLeanScr[3]};   // BVG_CLASS_STAGE / _SCR
};

static Knobs read_knobs() {
    Knobs k; const char* v;
    k.noskip = knob("BVG_NOSKIP"); k.nostripe = knob("BVG_NOSTRIPE"); k.nopredict = knob("BVG_NOPREDICT"); k.no_w18 = knob("BVG_NO_W18"); k.mat_lean = knob("BVG_MAT_LEAN");
    k.serial = knob("BVG_SERIAL"); k.flat_prof = knob("BVG_FLAT_PROF");
    if ((v = knob("BVG_GIANT"))) { k.giant = atoi(v); } if ((v = knob("BVG_SCANK"))) { k.scank_off = atoi(v) == 0; }
    if ((v = knob("BVG_DBG"))) { k.dbg = (uint32_t)strtoul(v, nullptr, 10); } if ((v = knob("BVG_PASSCOST"))) { k.pass_cost = (uint32_t)strtoul(v, nullptr, 10); }
    if ((v = knob("BVG_XCDS"))) { k.xcds = (uint32_t)std::max(1, atoi(v)); } if ((v = knob("BVG_WIDE_HALF"))) { k.wide_half = strtoull(v, nullptr, 10); }
    if ((v = knob("BVG_EMIT"))) k.emit = (uint32_t)strtoul(v, nullptr, 10) ? 1 : 0;
    if ((v = knob("BVG_STAGE"))) k.stage = std::min<uint32_t>(std::max<uint32_t>((uint32_t)strtoul(v, nullptr, 10) & ~3u, 64u), 2048u);   // (the skip entries hold 16-bit offsets into a record)
    if ((v = knob("BVG_POOL"))) { k.pool_set = true; k.pool = strtoull(v, nullptr, 10); } if ((v = knob("BVG_WAVES"))) { k.waves = std::max<uint64_t>(1, strtoull(v, nullptr, 10)); }
    if ((v = knob("BVG_WG"))) { k.wg = atoi(v); } if ((v = knob("BVG_WGC"))) { k.wgc = atoi(v); } if ((v = knob("BVG_WG_BLOCKS"))) { k.wg_blocks = std::max<uint64_t>(1, strtoull(v, nullptr, 10)); }
    if ((v = knob("BVG_FLOW"))) { k.flow = atoi(v); } if ((v = knob("BVG_FLOW_RING"))) { k.flow_ring = (uint32_t)std::min(8192, std::max(512, atoi(v))); }
    if ((v = knob("BVG_FLAT"))) { k.flat = atoi(v); } if ((v = knob("BVG_FLAT_RECS"))) { k.flat_recs = std::min(256u, std::max(64u, (unsigned)atoi(v) & ~63u)); }
    if ((v = knob("BVG_SCAN_SCR"))) { k.scan_scr = strtoull(v, nullptr, 10); } if ((v = knob("BVG_SCAN_LISTS"))) { k.scan_lists = atof(v); } if ((v = knob("BVG_SCAN_POOL"))) { k.scan_pool = std::min<uint64_t>(std::max<uint64_t>(strtoull(v, nullptr, 10), 512), 12288); }
    if ((v = knob("BVG_SCAN_WAVES"))) { k.scan_waves = strtoull(v, nullptr, 10); } if ((v = knob("BVG_SCAN_STAGE"))) { k.scan_stage = (uint32_t)std::min(2048, std::max(128, atoi(v) & ~3)); }
    if ((v = knob("BVG_CADMIT"))) { k.cadmit = atof(v); } if ((v = knob("BVG_ADMIT"))) { k.admit = atof(v); } if ((v = knob("BVG_GBATCH"))) { k.gbatch = (uint32_t)std::max(1, atoi(v)); }
    if ((v = knob("BVG_ORDER"))) { k.tier0_first = atoi(v) == 1; } if ((v = knob("BVG_T0WAIT"))) { k.t0wait = atoi(v) == 1; } if ((v = knob("BVG_SIDE2"))) { k.side2 = atoi(v); }
    unsigned cs[4] = {1024, 1024, 1024, 1024}, cr[4] = {1024, 1024, 2048, 3072};
    if ((v = knob("BVG_CLASS_STAGE"))) { sscanf(v, "%u,%u,%u,%u", &cs[0], &cs[1], &cs[2], &cs[3]); for (int c = 0; c < 4; c++) k.class_stage[c] = std::min(2048u, std::max(128u, cs[c] & ~3u)); }
    if ((v = knob("BVG_CLASS_SCR"))) { sscanf(v, "%u,%u,%u,%u", &cr[0], &cr[1], &cr[2], &cr[3]); for (int c = 0; c < 4; c++) k.class_scr[c] = std::min(8192u, std::max(128u, cr[c])); }
    return k;
}

// The experimental kernels (experimental/, built by `make experimental` only) a call runs in place of the product's: chosen in select_experiments alone.
struct Experiments {
    enum { kRowKernel, kStream, kLegacy } tier0 = kRowKernel;   // bvg_tuning.reserved 2: the streaming data-flow kernel as tier 0; 1: the generic row kernel (BitCursor) in LDS as tiers 0 / 1
    int wg_nw = 0, wg_class = 0;            // wavefronts per pool of the workgroup row kernel as tier 0 / in the LDS classes (0: the row kernel)
    bool flow = false; uint32_t flow_ring = 0;   // the flow scan kernel as predicted tier 0
    bool flat = false; uint32_t flat_recs = 0;   // the flat scan kernel in place of the lean one
};

// what one run_decode call works with
struct Decode {
    bvg_graph* g; Shared* sh; std::shared_ptr<Plan> plp; const Plan& pl;   // the plan is held for the whole call (see Shared::plans)
    int64_t from, to; bool materialise; const BatchPlan* batch; bvg_scan_result* res;
    Knobs k; Experiments x;
    bool force_slow, rows_default, force_giant, wide; size_t esz; double avg;
    uint32_t lo = 0, nblocks = 0;
    std::shared_ptr<SkipIndex> skx;         // held for the whole call
    DecodeArgs a{}, af{};                   // the row kernels' arguments, the lean scan kernel's
    bool giant_ok = false, predict = false, fast_ok = false; uint32_t lean_waves = 0;
    uint32_t launches = 0, slow_blocks = 0, lean_blocks = 0; double kernel_ms = 0; bool predicted_run = false;   // (cascade outcomes of a predicted run are remembered in g->pred2)
    std::vector<uint32_t> work; DevArray<uint32_t> d_work;   // the blocks the next tier runs
    Decode(bvg_graph* g_, std::shared_ptr<Plan> p, int64_t f, int64_t t, bool m, const BatchPlan* b, bvg_scan_result* r)
        : g(g_), sh(g_->sh), plp(std::move(p)), pl(*plp), from(f), to(t), materialise(m), batch(b), res(r), k(read_knobs()) {
        force_slow = g->tun.force_slow || sh->p.window_size > kMaxWindow;   // wide windows: the generic global-memory kernel only
        rows_default = (g->tun.reserved & 0xFF) == 0 && !force_slow;
        force_giant = !force_slow && k.giant == 2;                          // tests: every block through the giant kernel
        wide = sh->wide || g->tun.force_wide; esz = wide ? 8 : 4;
        avg = sh->p.arcs > 0 && sh->p.nodes > 0 ? (double)sh->p.arcs / (double)sh->p.nodes : 16.0;
        if (batch) { nblocks = batch->requests; return; }
        const std::vector<uint64_t>& hf = pl.h_first;
        lo = (uint32_t)(std::upper_bound(hf.begin(), hf.end(), (uint64_t)from) - hf.begin());
        lo = lo ? lo - 1 : 0;
        const uint32_t hi = std::min<uint32_t>((uint32_t)(std::lower_bound(hf.begin(), hf.end(), (uint64_t)to) - hf.begin()), pl.nblk);
        nblocks = hi > lo ? hi - lo : 0;
    }
    Pred& pred() { return g->pred2[materialise ? 1 : 0]; }
    bool tier0_runs() const { return nblocks && !force_slow && !force_giant; }
    int fetch_failures(std::vector<uint32_t>& out) {        // the blocks the last launches failed
        uint32_t nfail = 0;
        HIPCHK(hipMemcpy(&nfail, g->d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (nfail > g->fail_cap) return BVG_E_NOMEM;
        out.resize(nfail);
        if (nfail) HIPCHK(hipMemcpy(out.data(), g->d_fail + 1, nfail * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return 0;
    }
    int fetch_needs(std::vector<uint32_t>& need) { need.resize(work.size()); HIPCHK(hipMemcpy(need.data(), g->d_fail + 1 + g->fail_cap, work.size() * sizeof(uint32_t), hipMemcpyDeviceToHost)); return 0; }   // ... and their fail_need (`work` holds them)
    template <typename F> int timed(const char* what, size_t nb, F&& launch) {
        HIPCHK(hipEventRecord(g->ev0, g->stream));
        launch();
        HIPCHK(hipEventRecord(g->ev1, g->stream)); HIPCHK(hipStreamSynchronize(g->stream));
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
        kernel_ms += ms;
        if (dbg_on()) fprintf(stderr, "[bvg] %s: %zu blocks, %.3f ms\n", what, nb, ms);
        return 0;
    }
    int upload_work() {
        if (d_work.alloc(work.size())) return BVG_E_NOMEM;
        HIPCHK(hipMemcpy(d_work, work.data(), work.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(g->d_fail, 0, sizeof(uint32_t), g->stream));
        a.work_list = d_work;
        return 0;
    }
    // the LDS tiers' kernel (tier 0 and, is_class, the size classes): the row kernel, or the experiment selected in its place
    void launch_lds(const DecodeArgs& aa, uint32_t nb, hipStream_t st, bool is_class = false) {
        if (x.tier0 == Experiments::kStream && !is_class) launch_stream_decode(aa, nb, wide, materialise, st);
        else if (x.tier0 == Experiments::kLegacy) launch_decode(aa, nb, wide, materialise, false, st);
        else if (x.flow && !is_class && aa.work_list == pred().d_lists) launch_flow_scan(aa, nb, g->flow_waves, g->flow_ws.get(), x.flow_ring, st);
        else if (const int nw = is_class && x.wg_class ? x.wg_class : x.wg_nw) launch_rows_wg_decode(aa, nb, nw, st);
        else launch_rows_decode(aa, nb, wide, materialise, st);
    }
    void launch_lean(DecodeArgs& al, uint32_t nb, int occ, hipStream_t st) {   // occ: wavefronts per SIMD the instantiation leaves registers for (4: 128 VGPRs, 5: 96, 6: 80)
        if (x.flat) { al.flat_recs = x.flat_recs; launch_flat_decode(al, nb, occ == 6, st); }
        else launch_scan_decode(al, nb, wide, occ, materialise, st);
    }
    void learn(const std::vector<uint32_t>& ids, uint8_t slot) {   // where these blocks finally ran: later predicted runs send them there
        Pred& pd = pred();
        if (predicted_run) for (uint32_t id : ids) if (id < pd.learned.size()) { pd.learned[id] = slot; pd.dirty = true; }
    }
};

// The residual skip index is built the first time it would pay: a SCAN of >= 4096 nodes indexes the blocks it covers (a shard
// of a multi-GPU scan builds its own part only; a later scan outside them indexes the whole graph), a materialising call
// the whole graph once it covers a quarter of it.  bvg_build_index() does the same explicitly.  `done`: the build's validating pass was this scan.
static int ensure_skip(Decode& d, bool& done) {
    bvg_graph* g = d.g; const int64_t span = d.to - d.from;
    if (!d.batch && d.rows_default && g->skip_mode == 0 && !d.k.noskip && g->tun.no_index != 1 && span >= 4096 && d.nblocks) {
        const uint32_t lo = d.lo, hi = d.lo + d.nblocks;
        std::shared_ptr<SkipIndex> cur = std::atomic_load(&d.plp->skip);
        bool covered = cur && cur->covers(lo, hi), retry = false;
        // a build that failed for want of memory is tried again every kRetryEvery-th scan of its blocks; so is the whole-graph rebuild behind a good partial index
        // (the countdown is shared by every handle of the graph: a compare-exchange, so that two threads at 1 cannot wrap it)
        auto tick = [](const SkipIndex& ix) { uint32_t b = ix.backoff.load(); while (b > 0 && !ix.backoff.compare_exchange_weak(b, b - 1)) {} return b; };   // the value before the tick
        // (round 6: the cause is the covering RANGE's own, and only a call that could rebuild -- a scan, or a materialising call of a quarter of the graph -- counts down)
        const bool can_build = !d.materialise || span >= d.sh->p.nodes / 4;
        if (cur && covered && cur->failed && cur->cause_of(lo, hi) == SkipIndex::kResources) { if (can_build && tick(*cur) <= 1) { covered = false; retry = true; } }
        else if (cur && !covered && !cur->failed && cur->wide != d.wide) covered = true;        // a good index of the other width is not replaced (build_skip): this handle scans without it
        else if (cur && !covered && !cur->failed && can_build && tick(*cur) > 0) covered = true;
        if (!covered && can_build) {                        // (the validating pass of the build may BE this scan: same nodes, the checking kernels, bit-exact by construction)
            const int r = d.materialise ? build_skip(g, d.plp, 0, d.pl.nblk, retry) : build_skip(g, d.plp, lo, hi, retry, d.res, d.from, d.to, &done);
            if (r || done) return r;
        }
    }
    d.skx = g->skip_mode >= 2 ? g->skip_building : (g->skip_mode == 1 ? std::shared_ptr<SkipIndex>() : std::atomic_load(&d.plp->skip));
    if (d.skx && g->skip_mode == 0 && (d.skx->failed || g->tun.no_index == 1)) d.skx.reset();      // a failed build left no arrays; bvg_tuning.no_index: this handle scans without it
    return 0;
}

static int base_args(Decode& d, const uint64_t* d_cum, int64_t* d_succ, int32_t* d_outdeg) {
    bvg_graph* g = d.g; Shared* sh = d.sh; DecodeArgs& a = d.a;
    if (d.nblocks > g->fail_cap) {                          // every block may fail over to the slow path
        g->fail_cap = 0;
        if (g->d_fail.alloc(2 * (size_t)d.nblocks + 1)) return BVG_E_NOMEM;
        g->fail_cap = d.nblocks;
    }
    HIPCHK(hipMemsetAsync(g->d_acc, 0, (size_t)kAccStripes * kAccStride * sizeof(unsigned long long), g->stream));
    HIPCHK(hipMemsetAsync(g->d_fail, 0, sizeof(uint32_t), g->stream));
    const BatchPlan* batch = d.batch;
    a.graph = sh->d_graph; a.limit_byte = sh->nbytes; a.padded_bytes = sh->padded; a.offsets = sh->offs; a.n = sh->p.nodes; a.from = d.from; a.to = d.to;
    a.blk_first = batch ? batch->d_first : d.pl.d_first; a.blk_halo = batch ? batch->d_halo : d.pl.d_halo; a.blk_mask = batch ? batch->d_mask : d.pl.d_mask;
    a.work_list = nullptr; a.blk_lo = d.lo; a.batch = batch ? 1u : 0u;
    a.window = sh->p.window_size; a.min_interval = sh->p.min_interval_length; a.cod = codings_of(sh->p);
    a.node_base = g->node_base; a.acc = g->d_acc; a.acc_mask = d.k.nostripe ? 0u : kAccStripes - 1; a.cum = d_cum; a.succ = d_succ; a.outdeg = d_outdeg;
    a.fail_list = g->d_fail + 1; a.fail_count = g->d_fail; a.fail_cap = g->fail_cap; a.fail_need = g->d_fail + 1 + g->fail_cap;
    a.dbg = d.k.dbg;
#ifndef BVG_PROF
    a.dbg &= (16u | 32u | 64u | 4096u | 8192u | 0xFFFF0000u);             // forcing an emission form (16, 32; 4096 / 8192: scan_kernel's opt-in list builds) and the work counters leave the results alone; the
                                                            // phase-skipping bits (1, 2, 4, 128) exist in the profiling build only
#endif
    // The COUNTING pass of the index build needs the record headers only (a node's entry count follows from its residual count): the
    // row kernels skip the residual decode and the emission there (the same switches the profiling build skips phases with), which
    // turns the first of the two index passes into a header walk.  Pool sizing and every fail-over stay as in the filling pass, so a
    // block is counted in the tier that will fill it.
    if (g->skip_mode == 1) a.dbg |= 3u;
    // Row-kernel variant: splitting lists into tasks pays on dense or reference-free graphs; sparse graphs with reference
    // chains (several short levels per row) are served better by the pipelined node-per-lane loop alone.
    a.emit_tasks = (sh->p.window_size == 0 || d.avg >= 8.0) ? 1u : 0u;     // (sparse web shape, 11 arcs a node: the scan kernel still gains 3 %, profiles/r03_web_lean.txt)
    if (d.k.emit >= 0) a.emit_tasks = (uint32_t)d.k.emit;
    a.pass_cost = d.k.pass_cost;                            // measured: 11-14 merge steps per level pass; the optimum of the estimate is flat over 8-14
    a.skip_mode = (uint32_t)g->skip_mode; a.skip_cnt = g->skip_cnt;
    {   // the granularity of the index in use -- or of the one being built: the counting pass has no arrays yet
        const SkipIndex* gi = g->skip_mode == 1 ? g->skip_building.get() : d.skx.get();
        a.skip_min = gi ? gi->skip_min : kSkipMin; a.skip_shift = 0; if (gi) a.skip_shift = gi->skip_shift; else while ((1u << a.skip_shift) < kSkipEvery) a.skip_shift++;
    }
    a.xcds = d.k.xcds; a.wide_half = d.k.wide_half;
    if (!batch && d.rows_default && d.skx && d.skx->wide == d.wide) {
        a.skip_first = d.skx->d_first; a.skip_bit = d.skx->d_bit; a.skip_val = d.skx->d_val; a.skip_fmt = d.skx->d_fmt;
        // the recorded positions of the snapshot (scan mode of the lean scan kernel only); a marks-only handle has no entries at all, BVG_NO_POS=1 keeps the searches
        if (!d.materialise && g->skip_mode == 0 && !d.skx->h_pos_first.empty() && g->tun.no_index != 2 && !(knob("BVG_NO_POS") && atoi(knob("BVG_NO_POS")))) {
            a.pos_refd = d.skx->pos_refd; a.pos_first = d.skx->pos_first; a.pos_ent = d.skx->pos_ent; a.pos_ready = d.skx->pos_ready; a.pos_stat = dbg_on() ? 1u : 0u;
        }
    }
    a.grab_threshold = (g->tun.reserved >> 8) ? (g->tun.reserved >> 8) : 40;
    // tier 2a (bvg_giant.hip): lists / records too large for LDS, decoded by a whole workgroup each; default codings and windows <= 64
    // (anything else, and whatever it refuses, takes the generic kernel).  BVG_GIANT=0 switches it off.
    d.giant_ok = is_default_codings(a.cod) && d.rows_default && sh->p.window_size <= kMaxWindow && d.k.giant != 0;
    return 0;
}

// Every experiment is an opt-in of the experimental build, for full scans with default codings and 32-bit successors (the flat kernel: any
// scan with 32-bit ids); the product build selects none of them.
static void select_experiments(Decode& d) {
    bvg_graph* g = d.g; const Knobs& k = d.k; Experiments& x = d.x;
    if (kExperimental) x.tier0 = (g->tun.reserved & 0xFF) == 2 ? Experiments::kStream : (g->tun.reserved & 0xFF) == 1 ? Experiments::kLegacy : Experiments::kRowKernel;
    const bool scan = !d.materialise && !d.wide && !d.batch && is_default_codings(d.a.cod) && g->skip_mode == 0 && d.rows_default;
    // the workgroup row kernel, several wavefronts sharing one pool: as tier 0 (BVG_WG=2|4; measured: +4 % at 2 wavefronts on the eu shape, slower on sparse
    // graphs and at 4); in the big-LDS classes, which hold few workgroups per CU (BVG_WGC=2|4|8; round 1 (8 GiB eu): 258.6 ms (0), 254.9 (2), 254.6 (4); end of
    // round 2, after the single-wavefront kernel got the window overlay and the leaf pass (2 GiB eu15 / eu): 53.2 / 53.4 ms (0), 53.3 / 53.8 (2), 54.2 / 54.6 (4),
    // 56.5 / 57.7 (8) -- the workgroup kernel is opt-in again)
    if (kExperimental && scan && d.a.emit_tasks && (k.wg == 2 || k.wg == 4)) x.wg_nw = k.wg;
    if (kExperimental && scan && d.a.emit_tasks && (k.wgc == 2 || k.wgc == 4 || k.wgc == 8)) x.wg_class = k.wgc;
    // The flow scan kernel as tier 0 (bvg_flow.hip): windows up to 64.  Its LDS holds only the lists of the window that are really copied
    // from, so it keeps more wavefronts resident than the row kernel.
    if (kExperimental && k.flow && scan && d.sh->p.window_size <= kMaxWindow) {
        x.flow = true; x.flow_ring = k.flow_ring;
        const size_t per = flow_scratch_bytes_per_wave(d.sh->p.window_size);
        const uint32_t per_cu = (uint32_t)std::min<size_t>(20, (160 * 1024) / (flow_lds_bytes(x.flow_ring) + 1536 + 64));
        const uint32_t waves = 256u * std::max(1u, per_cu);
        if (g->flow_waves != waves) g->flow_ws.reset();                    // (another geometry: a block of its own size)
        if (g->flow_ws.reserve(per * waves)) x.flow = false; else g->flow_waves = waves;
    }
    // The flat scan kernel (experimental/bvg_flat.hip, round 5: bit-exact, slower -- DESIGN.md) takes what the lean scan kernel takes, for scans (not materialising
    // calls) of graphs whose ids fit 32 bits, with BVG_FLAT=1; BVG_FLAT_RECS = records per super-row (64 ... 256).
    x.flat = kExperimental && !d.materialise && !d.wide && k.flat == 1;
    x.flat_recs = k.flat_recs ? k.flat_recs : (d.avg <= 16.0 ? 128u : 64u);
}

// tier 0: every block, LDS sized for occupancy (the list pool holds one row of 64 lists + the window)
static void tier0_pool(Decode& d) {
    DecodeArgs& a = d.a; const Knobs& k = d.k; const bool wide = d.wide; const size_t esz = d.esz; const double avg = d.avg;
    if (d.x.tier0 == Experiments::kStream) {                // list ring: power of two
        uint64_t want = (uint64_t)(avg * 72.0), cap = 2048;
        while (cap * 2 <= want && cap < (wide ? 8192u : 16384u)) cap *= 2;
        a.lds_pool_elems = (uint32_t)(k.pool_set ? k.pool : cap); a.lds_scr_elems = 0;
        return;
    }
    const bool task = a.emit_tasks != 0;                    // task emission parks the row's residuals beside the lists
    uint64_t pool = ((uint64_t)(avg * (task ? 52.0 : 48.0)) + 255) & ~255ull;   // ~a row of lists (rows shrink when they do not fit)
    pool = std::min<uint64_t>(std::max<uint64_t>(pool, 1024), wide ? 4096 : 8192);
    if (d.x.wg_nw) {
        // workgroups per CU are bounded by registers (wavefronts per SIMD): give each the LDS share of that count
        uint64_t wgs = d.x.wg_nw == 4 ? 5 : 8;
        if (k.wg_blocks) wgs = k.wg_blocks;
        const uint64_t share = ((160 * 1024) / wgs) & ~255ull, fixed = (uint64_t)a.lds_stage_words * 4 + rows_wg_static_lds(d.x.wg_nw) + 256;
        const uint64_t fit = share > fixed ? ((share - fixed) / esz) * 8 / 9 : 1024;      // pool + pool/8 of scratch
        pool = std::min<uint64_t>(std::max<uint64_t>(pool, fit & ~63ull), 12288);
        pool = std::max<uint64_t>(pool, 1024);
    } else if (task) {
        // resident waves per CU step down with the LDS footprint: take every byte of the step the pool lands on
        const uint64_t lds_cu = 160 * 1024, fixed = 1536 + 64;   // static arrays (+ slack); the task variant keeps the stream window INSIDE the pool
        auto foot = [&](uint64_t pe) { return ((pe + std::max<uint64_t>(256, pe / 8)) * esz + fixed + 127) & ~127ull; };
        uint64_t waves = std::max<uint64_t>(1, lds_cu / foot(pool));
        // Two wavefronts per SIMD (8 per CU) is the step that pays on dense graphs: below it the CU's SIMDs sit idle behind
        // LDS latency, and a row that shrinks to ~40 lists costs less than the lost wavefronts (eu15 shape, 4 GiB: 90.0 G
        // edges/s at 6 per CU with 54 lists per row, 98.7 G at 8 per CU with 43; profiles/r02/occ_sweep15.sh).
        // Resident wavefronts per CU are what this kernel's throughput follows (linear from 1 to 8, profiles/r02/ldspad.sh), as
        // long as a row still holds enough lists to fill its lock-step passes: take the largest EVEN count (odd ones load
        // the four SIMDs unevenly: 9 and 11 measured below 8 and 10) whose pool holds ~48 average lists; dense graphs end at
        // 8-10, sparse ones at the 16 the registers allow (profiles/r02: eu 10 per CU 118.8 G edges/s vs 8: 117.3, 9: 113.8;
        // eu15 8: 121.6, 9: 111.0, 10: 111.3).
        if (!k.stage) {
            for (uint64_t w : {20ull, 16ull, 12ull, 10ull, 8ull, 6ull, 4ull}) {
                uint64_t pw = wide ? 4096 : 8192;
                while (pw > 1024 && lds_cu / foot(pw) < w) pw -= 32;
                if (lds_cu / foot(pw) >= w && ((double)pw >= 48.0 * avg || w == 4)) { pool = pw; waves = lds_cu / foot(pw); a.lds_stage_words = std::min<uint32_t>(a.lds_stage_words, 512); break; }
            }
        }
        if (k.waves) {                                      // experiments: aim at this many resident wavefronts per CU
            uint64_t pw = wide ? 4096 : 8192;
            while (pw > 1024 && lds_cu / foot(pw) < k.waves) pw -= 64;
            pool = pw; waves = lds_cu / foot(pw);
        }
        while (pool + 32 <= (wide ? 4096u : 8192u) && lds_cu / foot(pool + 32) == waves) pool += 32;
    }
    if (k.pool_set) pool = std::min<uint64_t>(std::max<uint64_t>(k.pool, 256), wide ? 6144 : 12288);
    a.lds_pool_elems = (uint32_t)pool; a.lds_scr_elems = (uint32_t)std::max<uint64_t>(256, pool / 8);
}

// The lean scan kernel (bvg_scan.hip) takes the blocks that the index-building pass has validated: scans with 32-bit
// successors and the default codings, index present.  BVG_SCANK=0 keeps every block on the row kernel (tests, A/B runs).
static void lean_geometry(Decode& d) {
    const DecodeArgs& a = d.a; const Knobs& k = d.k; const double avg = d.avg;
    // (a materialising call takes it on dense graphs only: below ~16 arcs per node the row kernel's pipelined loop is the faster way to
    //  build every list -- web shape 71.9 vs 60.5 G edges/s, eu shape 93.6 vs 165.9: profiles/r04_mat_first.txt)
    d.fast_ok = d.predict && !(d.materialise && avg < 16.0 && !k.mat_lean) && is_default_codings(a.cod) && a.emit_tasks && d.g->skip_mode == 0 && d.rows_default && a.skip_first &&
                a.skip_fmt && d.skx && d.skx->h_fmt.size() == d.pl.nblk && !d.x.wg_nw && !d.x.flow && !k.scank_off;
    d.af = a;
    if (!d.fast_ok) return;
    // LDS per wavefront: pool (stored lists + their parked residuals + the window) + scratch (copy blocks, intervals, run
    // queue) + static arrays.  Resident wavefronts per CU step down with it; take the largest even count whose pool
    // still holds a row's worth of lists (leaves take no pool: about half the row kernel's need).
    // The window: 512 dwords at up to 14 wavefronts, 384 at 16 (profiles/r03_ab_uni.txt; a super-row = the records that fit it, up to 64).
    // Lists, parked residuals and the super-row's copy blocks / intervals share pool + scratch (bvg_scan.hip): about half the
    // scratch is free for lists on average, and counts as such here.
    const size_t lean_static = d.x.flat ? flat_table_bytes(d.x.flat_recs, d.sh->p.window_size) : scan_static_lds();
    const uint64_t scrw = k.scan_scr, lds_cu = 160 * 1024, wforce = k.scan_waves;
    auto stage_of = [&](uint64_t w) -> uint32_t { return k.scan_stage ? k.scan_stage : std::min<uint32_t>(a.lds_stage_words, w >= 16 ? 384 : 512); };
    auto foot = [&](uint64_t pe, uint64_t w) { return (pe * 4 + lean_static + 64 + (uint64_t)stage_of(w) * 4 + scrw * 4 + 127) & ~127ull; };
    const bool refs = d.sh->p.window_size > 0 && !wforce && !d.materialise;
    uint64_t pool = 1024, waves = 4;
    for (uint64_t w : {24ull, 20ull, 18ull, 16ull, 14ull, 12ull, 10ull, 8ull, 6ull, 4ull}) {
        // (round 6: 18 wavefronts -- the 96-VGPR instantiation, 4.5 per SIMD -- for graphs of 16 ... 48 arcs per node: uk +5.8 %, profiles/r06_ab_w18_*.txt; eu15, 86 arcs per node: -3 %)
        if (w > 16 && wforce != w && !(w == 24 && avg <= 16.0 && refs)
            && !(w == 18 && avg > 16.0 && avg <= 48.0 && refs && !k.no_w18)) continue;   // more than 16: the 85-VGPR instantiation, sparse graphs with references only (web shape: +7 %; eu15: -11 % at 20; w0, all residuals: -6 %)
        if (wforce && w != wforce && w != 4) continue;
        uint64_t pw = 8192;
        while (pw > 512 && lds_cu / foot(pw, w) < w) pw -= 32;
        if (lds_cu / foot(pw, w) >= w && ((double)(pw + scrw / 2) >= k.scan_lists * avg || w == 4 || wforce)) { pool = pw; waves = w; break; }
    }
    const uint32_t stagew = stage_of(waves); d.lean_waves = (uint32_t)waves;
    while (pool + 32 <= 8192 && lds_cu / foot(pool + 32, waves) >= waves) pool += 32;
    if (k.scan_pool) pool = k.scan_pool;
    d.af.lds_pool_elems = (uint32_t)pool; d.af.lds_scr_elems = (uint32_t)scrw; d.af.lds_stage_words = stagew;
    if (dbg_on()) fprintf(stderr, "[bvg] %s: pool %u + scratch %u elements, window %u dwords, %llu wavefronts per CU\n", d.x.flat ? "flat kernel" : "scan kernel", d.af.lds_pool_elems, d.af.lds_scr_elems, d.af.lds_stage_words, (unsigned long long)waves);
}

static void geometry(Decode& d) {
    // stream window: ~1.5 rows of records, 1..4 KiB (LDS bytes bound occupancy, and occupancy bounds throughput)
    const double bits_per_node = d.sh->p.nodes > 0 ? (double)d.sh->total_bits / (double)d.sh->p.nodes : 64.0;
    uint32_t words = 256;
    while (words < 1024 && (double)words * 32.0 < bits_per_node * 64.0 * 1.5) words *= 2;
    d.a.lds_stage_words = d.k.stage ? d.k.stage : words;
    if (!d.tier0_runs()) return;
    tier0_pool(d);
    d.predict = !d.batch && d.x.tier0 == Experiments::kRowKernel && d.pl.h_maxd.size() == d.pl.nblk && !d.k.nopredict;
    lean_geometry(d);
}

// Blocks sorted into the work lists of Pred by the largest list they hold (and what earlier cascades taught about them); kept on the device until the plan, the
// index snapshot, the range or the geometry changes.
static int classify_blocks(Decode& d) {
    const Plan& pl = d.pl; const uint32_t lo = d.lo, nblocks = d.nblocks; const DecodeArgs& a = d.a; const DecodeArgs& af = d.af; Pred& pd = d.pred();
    const uint32_t pool0 = a.lds_pool_elems;
    const uint32_t pmode = (d.materialise ? 1u : 0u) | (a.emit_tasks ? 2u : 0u) | (a.skip_first ? 4u : 0u) | (d.wide ? 8u : 0u) | (d.x.flow ? 16u : 0u) | (d.fast_ok ? 32u : 0u) | (d.fast_ok && d.x.flat ? 64u : 0u) | (d.fast_ok ? (af.lds_pool_elems << 8) : 0u);
    const uint64_t cap0 = d.x.flow ? 6144 : pool0;          // the flow kernel keeps long lists in its scratch area
    const uint64_t sgen = (a.skip_first && d.skx) ? d.skx->gen : 0;   // the snapshot the marks / entry layouts come from: another one, another split
    const bool rekey = pd.plan_version != pl.version || pd.skip_gen != sgen || pd.lo != lo || pd.n != nblocks || pd.pool0 != pool0 || pd.mode != pmode || !pd.d_lists;
    // what the cascade taught about a block is kept per block of the PLAN, so a scan of another node range (a shard, an
    // iterator batch, the bench's verification of single tiles) does not throw it away
    if (pd.learned.size() != pl.nblk || pd.learned_version != pl.version || pd.learned_gen != sgen || pd.learned_pool0 != pool0 || pd.learned_mode != pmode) {
        pd.learned.assign(pl.nblk, 0); pd.leanfail.assign(pl.nblk, 0); pd.learned_version = pl.version; pd.learned_gen = sgen; pd.learned_pool0 = pool0; pd.learned_mode = pmode;
    }
    if (rekey) pd.dirty = false;
    if (!rekey && !pd.dirty) return 0;
    std::vector<uint32_t> L[Pred::kSlots];
    uint64_t gneed = 0, gnodes = 0, glong = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        const uint64_t md = pl.h_maxd[lo + i] & 0x7FFFFFFFu;    // worst "list + window" of the block
        const bool long_record = (pl.h_maxd[lo + i] >> 31) != 0;
        const uint64_t need = md + md / 8 + 64;
        const bool fastb = d.fast_ok && d.skx->h_fmt[lo + i] == 1 && pd.leanfail[lo + i] < 2;   // (a block the lean kernel failed twice -- first for its pool, then in the class it was sent to -- stays on the row kernel)
        int c;
        if (long_record) c = Pred::kGiant;
        else if (fastb ? ((uint64_t)((double)md * d.k.admit) + 64 <= af.lds_pool_elems + af.lds_scr_elems / 2) : need <= cap0) c = Pred::kRow0;   // (the lean kernel stores only the lists that are copied from: optimistic, the cascade teaches the rest)
        else { c = Pred::kRowC1; const uint64_t cneed = fastb ? (uint64_t)((double)need * d.k.cadmit) : need; while (c < Pred::kGiant && kClasses[c - 1] < cneed) c++; }
        const int lrn = pd.learned[lo + i];                 // learned from an earlier scan's cascade
        if (lrn > c) { c = lrn; if (c >= Pred::kGiant && gneed < 65536) gneed = 65536; }
        if (c == Pred::kGiant && !d.giant_ok) c = Pred::kGeneric;
        if (c >= Pred::kGiant && need > gneed) gneed = need;
        if (c >= Pred::kGiant) { gnodes += pl.h_first[lo + i + 1] - pl.h_first[lo + i]; if (long_record) glong++; }
        L[(fastb && c <= Pred::kRowC4) ? Pred::kLean0 + c : c].push_back(lo + i);
    }
    const size_t ngiant = L[Pred::kGiant].size() + L[Pred::kGeneric].size();
    if (dbg_on() && ngiant) fprintf(stderr, "[bvg] giant blocks: %zu (%llu of them for a record longer than the window), %llu nodes in them\n", ngiant, (unsigned long long)glong, (unsigned long long)gnodes);
    pd.dirty = false; pd.mode = pmode;
    if (pd.d_lists.alloc(nblocks)) return BVG_E_NOMEM;
    size_t off = 0;
    for (int c = 0; c < Pred::kSlots; c++) {
        pd.count[c] = (uint32_t)L[c].size();
        if (!L[c].empty()) HIPCHK(hipMemcpy(pd.d_lists + off, L[c].data(), L[c].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        off += L[c].size();
    }
    pd.plan_version = pl.version; pd.skip_gen = sgen; pd.lo = lo; pd.n = nblocks; pd.pool0 = pool0; pd.giant_need = gneed;
    return 0;
}

struct GiantWs { uint64_t pool_elems = 0, scr_elems = 0; uint32_t batch = 0; bool slots = false; };   // batch 0: no workspace, the cascade takes the giants
// giants: global-memory pools sized to the largest list, allocated before anything is launched
static int giant_workspace(Decode& d, GiantWs& gw) {
    bvg_graph* g = d.g; const Pred& pd = d.pred();
    const uint32_t ngiant = pd.count[Pred::kGiant] + pd.count[Pred::kGeneric];
    if (!ngiant) return 0;
    // (the giant kernel parks the residuals of the list it decodes in the same area: twice the worst list + window)
    gw.pool_elems = 1ull << 16; while (gw.pool_elems < 2 * pd.giant_need + pd.giant_need / 4) gw.pool_elems <<= 1;
    // Work areas: as many SLOTS as giant workgroups can be resident at once (2 per CU: bvg_giant.hip) and half as many again, whatever the
    // number of giant blocks -- the kernel takes a free slot when a workgroup starts (DecodeArgs::gslots).  Round 3 sized one area per block of
    // a batch of 8 192 (up to 1/8 of the free memory: 26-31 GB on the default workload, per handle).  All giants go in ONE launch.
    gw.scr_elems = gw.pool_elems / 2; gw.batch = std::min<uint32_t>(giant_slots(), ngiant);
    if (d.k.gbatch) gw.batch = d.k.gbatch;                  // (experiments: batched launches, one area per block of a batch)
    gw.slots = !d.k.gbatch;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const uint64_t per = (gw.pool_elems + gw.scr_elems) * d.esz, room = ((uint64_t)free_b + g->giant_ws.bytes()) / 4;
        const uint64_t fit = room / std::max<uint64_t>(per, 1);
        if (fit < gw.batch) { gw.batch = (uint32_t)std::max<uint64_t>(fit, 1); if (gw.batch < std::min<uint32_t>(kGiantResident, ngiant)) gw.slots = false; }   // too few slots for every resident workgroup: batches again
    }
    const uint64_t bytes = (uint64_t)gw.batch * (gw.pool_elems + gw.scr_elems) * d.esz;
    if (g->giant_ws.reserve(bytes)) gw.batch = 0;           // fall back to the cascade
    if (gw.slots && gw.batch) {
        if (!g->d_gslots && g->d_gslots.alloc(8192)) { gw.slots = false; gw.batch = std::min<uint32_t>(gw.batch, 256u); }
        if (gw.slots) HIPCHK(hipMemsetAsync(g->d_gslots, 0, 8192 * sizeof(uint32_t), g->stream));   // (ordered before the side streams by ev0 below)
    }
    return 0;
}

// every work list of the prediction at once: tier 0 on the main stream, giants and LDS classes on the side streams
static int launch_concurrent(Decode& d, const GiantWs& gw) {
    bvg_graph* g = d.g; const Pred& pd = d.pred(); const Knobs& k = d.k; const bool wide = d.wide, materialise = d.materialise;
    HIPCHK(hipEventRecord(g->ev0, g->stream));
    for (int i = 0; i < bvg_graph::kSide; i++) HIPCHK(hipStreamWaitEvent(g->side[i], g->ev0, 0));
    bool t0_waits = false;
    // side streams: [0] the giants and, behind them, the smallest class (short); [1..3] one per larger LDS class, so that every
    // class starts with the main launch and overlaps it.  (One stream per class and one for the giants made six streams: the
    // largest class then started only when the last giant batch had finished -- streams share hardware queues -- and ended 11 ms
    // after everything else at full size; three side streams were 11 % slower, profiles/r03_ab_smap.txt.)
    auto side_of = [&](int c) {
        if (k.side2 == 1) return g->side[c >= 4 ? 1 : c == 3 ? 0 : 2];
        if (k.side2 == 2) return g->side[c];
        return g->side[c == 1 ? 0 : c - 1];
    };
    auto alone = [&](hipStream_t st) { if (k.serial) (void)hipStreamSynchronize(st); };   // experiments: every launch alone on the chip (its own duration in a kernel trace)
    auto row0 = [&] { if (pd.count[Pred::kRow0]) { DecodeArgs a0 = d.a; a0.work_list = pd.d_lists; d.launch_lds(a0, pd.count[Pred::kRow0], g->stream); d.launches++; } };
    auto lean0 = [&] {
        if (!pd.count[Pred::kLean0]) return;
        DecodeArgs a7 = d.af; a7.work_list = pd.d_lists + pd.offset(Pred::kLean0);
        d.launch_lean(a7, pd.count[Pred::kLean0], d.lean_waves > 20 ? 6 : (d.lean_waves > 16 ? 5 : 4), g->stream); d.launches++; alone(g->stream);
    };
    if (k.tier0_first) { row0(); lean0(); }
    if (gw.batch && pd.count[Pred::kGiant] + pd.count[Pred::kGeneric]) {   // giants first: they are the critical path
        DecodeArgs ag = d.a; ag.gpool = g->giant_ws.get(); ag.gpool_elems = gw.pool_elems;
        if (ag.skip_mode == 3) ag.skip_mode = 2;            // (the giant kernel fills its own entries, in its own format, while it validates)
        ag.gscr = g->giant_ws.at((size_t)gw.batch * gw.pool_elems * d.esz); ag.gscr_elems = gw.scr_elems; ag.lds_stage_words = 1024;
        for (int c = Pred::kGiant; c <= Pred::kGeneric; c++) {
            const bool slots = gw.slots && c == Pred::kGiant;   // (the generic kernel keeps one area per block of a batch)
            ag.gslots = slots ? g->d_gslots.get() : nullptr; ag.gnslots = slots ? gw.batch : 0u;
            const uint32_t step = slots ? std::max<uint32_t>(pd.count[c], 1u) : gw.batch;
            for (uint32_t o2 = 0; o2 < pd.count[c]; o2 += step) {
                ag.work_list = pd.d_lists + pd.offset(c) + o2;
                const uint32_t nb = std::min<uint32_t>(step, pd.count[c] - o2);
                if (c == Pred::kGiant) launch_giant_decode(ag, nb, wide, materialise, g->side[0]);
                else launch_decode(ag, nb, wide, materialise, true, g->side[0]);
                d.launches++; alone(g->side[0]);
            }
        }
        // (experiment, BVG_T0WAIT=1: tier 0 starts when the giants are done.  With all giants in one launch they trickle through the whole scan beside tier 0 -- a giant
        // workgroup needs 16 wave slots of ONE CU at once -- and end ~30 ms after it, profiles/r04_eu15_scan_timeline.txt; holding tier 0 back by the giants' ~30 ms
        // ends the scan on tier 0 instead and takes exactly as long: 366.0 vs 366.5 ms, profiles/r04_ab_t0wait.txt.  The launches are work-conserving.)
        if (k.t0wait && !k.tier0_first) { HIPCHK(hipEventRecord(g->side_ev[0], g->side[0])); t0_waits = true; }
    }
    for (int c = 4; c >= 1; c--) {                          // LDS size classes, largest first
        if (!pd.count[Pred::kRow0 + c]) continue;
        DecodeArgs ac = d.a; ac.work_list = pd.d_lists + pd.offset(Pred::kRow0 + c);
        ac.lds_pool_elems = kClasses[c - 1]; ac.lds_scr_elems = std::max<uint32_t>(1024, kClasses[c - 1] / 4); ac.lds_stage_words = 1024;
        d.launch_lds(ac, pd.count[Pred::kRow0 + c], side_of(c), true); alone(side_of(c)); d.launches++;
    }
    for (int c = 4; c >= 1; c--) {                          // the same classes of the lean scan kernel
        if (!pd.count[Pred::kLean0 + c]) continue;
        DecodeArgs ac = d.af; ac.work_list = pd.d_lists + pd.offset(Pred::kLean0 + c);
        ac.lds_pool_elems = kClasses[c - 1]; ac.lds_scr_elems = k.class_scr[c - 1]; ac.lds_stage_words = k.class_stage[c - 1];
        d.launch_lean(ac, pd.count[Pred::kLean0 + c], 4, side_of(c)); alone(side_of(c)); d.launches++;
    }
    if (t0_waits) HIPCHK(hipStreamWaitEvent(g->stream, g->side_ev[0], 0));
    if (!k.tier0_first) { lean0(); row0(); }
    for (int i = 0; i < bvg_graph::kSide; i++) { HIPCHK(hipEventRecord(g->side_ev[i], g->side[i])); HIPCHK(hipStreamWaitEvent(g->stream, g->side_ev[i], 0)); }
    HIPCHK(hipEventRecord(g->ev1, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    d.kernel_ms += ms;
    const uint32_t* n = pd.count;
    if (dbg_on()) {
        unsigned long long ps[2] = {0, 0};                  // scan-kernel blocks that read their extras' positions back / that searched for them and wrote them down (a debug
                                                            // figure: fetched with a synchronous copy, and printed for the concurrent launch of the tiers only -- the cascade's launches print none)
        if (d.af.pos_stat) HIPCHK(hipMemcpy(ps, g->d_acc + 2 * kAccStride + 4, sizeof ps, hipMemcpyDeviceToHost));
        fprintf(stderr, "[bvg] tiers concurrent: scan kernel %u + %u/%u/%u/%u LDS-class, row kernel %u + %u/%u/%u/%u LDS-class, %u giant + %u generic blocks, %.3f ms; positions: %llu blocks recorded, %llu recording\n",
                n[Pred::kLean0], n[Pred::kLeanC1], n[Pred::kLeanC2], n[Pred::kLeanC3], n[Pred::kLeanC4], n[Pred::kRow0], n[Pred::kRowC1], n[Pred::kRowC2], n[Pred::kRowC3], n[Pred::kRowC4], n[Pred::kGiant], n[Pred::kGeneric], ms, ps[0], ps[1]);
    }
    return 0;
}

static int run_predicted(Decode& d) {
    GiantWs gw; int r = classify_blocks(d); if (r) return r;
    r = giant_workspace(d, gw); if (r) return r;
    r = launch_concurrent(d, gw); if (r) return r;
    Pred& pd = d.pred();
    d.slow_blocks = d.nblocks - pd.count[Pred::kRow0] - pd.count[Pred::kLean0];
    d.lean_blocks = pd.count[Pred::kLean0] + pd.count[Pred::kLeanC1] + pd.count[Pred::kLeanC2] + pd.count[Pred::kLeanC3] + pd.count[Pred::kLeanC4];
    d.predicted_run = true;
    const uint32_t ngiant = pd.count[Pred::kGiant] + pd.count[Pred::kGeneric];
    std::vector<uint32_t> gl(gw.batch ? 0 : ngiant);        // could not get the giant workspace: leave them to the cascade
    if (!gl.empty()) HIPCHK(hipMemcpy(gl.data(), pd.d_lists + pd.offset(Pred::kGiant), gl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    r = d.fetch_failures(d.work); if (r) return r;
    d.work.insert(d.work.end(), gl.begin(), gl.end());
    if (d.fast_ok) for (uint32_t id : d.work) if (id < pd.leanfail.size() && d.skx->h_fmt[id] == 1 && pd.leanfail[id] < 2) { pd.leanfail[id]++; pd.dirty = true; }
    d.slow_blocks += (uint32_t)d.work.size();               // blocks the prediction missed: re-run by the cascade below
    return 0;
}

static int run_unpredicted(Decode& d) {
    if (d.batch) {                                          // one block per request: the even entries of the per-call plan
        d.work.resize(d.nblocks); for (uint32_t i = 0; i < d.nblocks; i++) d.work[i] = 2 * i;
        const int r = d.upload_work(); if (r) return r;
        d.work.clear();
    }
    int r = d.timed("tier0 (LDS)", d.nblocks, [&] { d.launch_lds(d.a, d.nblocks, d.g->stream); }); if (r) return r;
    d.launches++;
    r = d.fetch_failures(d.work); if (r) return r;
    d.slow_blocks = (uint32_t)d.work.size();
    return 0;
}

// tier 1: the few blocks holding a list that overflowed the small pool, re-run with a pool sized to
// what each block reported it needs (size classes keep as many waves resident as possible)
static int tier1_classes(Decode& d) {
    DecodeArgs& a = d.a;
    std::vector<uint32_t> need, bins[4], rest;
    int r = d.fetch_needs(need); if (r) return r;
    if (dbg_on()) { size_t h[8] = {0}; for (uint32_t nd : need) h[nd >= kFailReason ? (nd - kFailReason) & 7 : 0]++; fprintf(stderr, "[bvg] failures: pool %zu, window %zu, huge %zu, blocks-scratch %zu, intervals-scratch %zu, code %zu, other %zu\n", h[0], h[1], h[2], h[3], h[4], h[5], h[7]); }
    for (size_t i = 0; i < d.work.size(); i++) {
        int c = 3;
        if (d.x.tier0 == Experiments::kRowKernel && need[i] < kFailReason) { c = 0; while (c < 3 && kClasses[c] < need[i]) c++; if (kClasses[c] < need[i]) c = -1; }
        if (c < 0) rest.push_back(d.work[i]); else bins[c].push_back(d.work[i]);
    }
    for (int c = 0; c < 4; c++) {
        if (bins[c].empty()) continue;
        d.work.swap(bins[c]);
        r = d.upload_work(); if (r) return r;
        a.lds_pool_elems = kClasses[c]; a.lds_scr_elems = std::max<uint32_t>(1024, kClasses[c] / 4); a.lds_stage_words = 1024;
        const uint32_t nb = (uint32_t)d.work.size();
        r = d.timed("tier1 (big LDS)", nb, [&] { d.launch_lds(a, nb, d.g->stream, true); });
        if (r) return r;
        d.launches++;
        std::vector<uint32_t> again;
        r = d.fetch_failures(again); if (r) return r;
        // what a class fails is tried in the next larger one (the need a block reported may come from another kernel's footprint)
        if (c < 3) bins[c + 1].insert(bins[c + 1].end(), again.begin(), again.end()); else rest.insert(rest.end(), again.begin(), again.end());
        if (d.predicted_run) {                              // remember where the survivors of this class fit
            Pred& pd = d.pred();
            std::sort(again.begin(), again.end());
            for (uint32_t id : d.work)
                if (id < pd.learned.size() && !std::binary_search(again.begin(), again.end(), id)) { pd.learned[id] = (uint8_t)(Pred::kRowC1 + c); pd.dirty = true; }
        }
    }
    d.work.swap(rest);
    d.learn(d.work, Pred::kGiant);
    return 0;
}

// tier 2a / 2: per-workgroup areas in global memory (kept in the handle), grown until every remaining block fits.  First the
// giant kernel (a workgroup per list); what it refuses (overlapping streams, contradictory counts) goes to the generic kernel.
static int run_global_tier(Decode& d, bool giant, std::vector<uint32_t>& refused) {
    bvg_graph* g = d.g; DecodeArgs& a = d.a; std::vector<uint32_t>& work = d.work;
    uint64_t pool_elems = 1ull << 20;
    while (!work.empty()) {
        uint64_t scr_elems = pool_elems / 2;
        uint64_t per_wg = (pool_elems + scr_elems) * d.esz;
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        uint32_t batch = (uint32_t)std::min<uint64_t>({(uint64_t)work.size(), std::max<uint64_t>(1, ((free_b + g->slow_ws.bytes()) / 2) / per_wg), 1024});
        if (g->slow_ws.reserve((size_t)batch * per_wg)) return BVG_E_NOMEM;
        int r = d.upload_work(); if (r) return r;
        a.gpool = g->slow_ws.get(); a.gpool_elems = pool_elems;
        a.gscr = g->slow_ws.at((size_t)batch * pool_elems * d.esz); a.gscr_elems = scr_elems;
        a.lds_stage_words = 1024;
        const size_t nwork = work.size();
        r = d.timed(giant ? "tier2a (giant)" : "tier2 (generic)", nwork, [&] {
            for (size_t off = 0; off < nwork; off += batch) {
                uint32_t nb = (uint32_t)std::min<size_t>(batch, nwork - off);
                a.work_list = d.d_work + off;
                if (giant) { DecodeArgs ag2 = a; if (ag2.skip_mode == 3) ag2.skip_mode = 2; launch_giant_decode(ag2, nb, d.wide, d.materialise, g->stream); } else launch_decode(a, nb, d.wide, d.materialise, true, g->stream);
                d.launches++;
            }
        });
        if (r) return r;
        r = d.fetch_failures(work); if (r) return r;
        if (giant && !work.empty()) {                       // only "the area is too small" is worth another round
            std::vector<uint32_t> need, again;
            r = d.fetch_needs(need); if (r) return r;
            for (size_t i = 0; i < work.size(); i++) (need[i] == kFailHuge ? again : refused).push_back(work[i]);
            work.swap(again);
        }
        if (!work.empty()) {
            if (pool_elems >= (1ull << 34)) { if (giant) { refused.insert(refused.end(), work.begin(), work.end()); work.clear(); break; } return BVG_E_NOMEM; }
            pool_elems *= 8;
        }
    }
    return 0;
}

static int cascade(Decode& d) {
    if (!d.work.empty() && !d.force_slow && !d.force_giant) { const int r = tier1_classes(d); if (r) return r; }
    if (!d.work.empty() && d.giant_ok && !d.force_slow) {
        std::vector<uint32_t> refused;
        const int r = run_global_tier(d, true, refused); if (r) return r;
        d.work.swap(refused);
        d.learn(d.work, Pred::kGeneric);
    }
    std::vector<uint32_t> none;
    return run_global_tier(d, false, none);
}

static int finish(Decode& d) {
    bvg_graph* g = d.g; const DecodeArgs& a = d.a; const uint32_t lean_blocks = d.lean_blocks;
#ifdef BVG_PROF_WORK
    unsigned long long acc[2 * kAccStride];                 // (`make work`: the scan kernel's fill counts stand in the spare words of result stripe 1)
#else
    unsigned long long acc[32];
#endif
    launch_reduce_acc(g->d_acc, kAccStripes, g->stream);
    HIPCHK(hipMemcpyAsync(acc, g->d_acc, sizeof acc, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    if (a.dbg & 64u) fprintf(stderr, "[bvg] counters: position steps %llu, position passes %llu, extras passes %llu, rows %llu, position tasks %llu, leaf steps %llu, leaf passes %llu\n", acc[4], acc[5], acc[8], acc[6], acc[7], acc[22], acc[23]);
    if ((a.dbg & 64u) && lean_blocks) fprintf(stderr, "[bvg] scan kernel rows: %llu super-rows, %llu sub-rows, %llu nodes in them\n", acc[5], acc[6], acc[7]);
    if ((a.dbg & 64u) && lean_blocks && d.k.flat_prof)      // `make flatprof` (-DBVG_FLAT_PROF): the flat kernel's section cycles and work counts (bvg_flat.hip)
        fprintf(stderr, "[bvg] flat kernel wave-cycles (M): super-row set-up %.0f, headers %.0f, peek/marks %.0f, sizing+stages %.0f, residual set-up %.0f, residual steps %.0f, Z1 %.0f, item set-up %.0f, chunks %.0f, compaction %.0f | "
                "super-rows %llu sub-rows %llu records %llu | residual passes %llu steps %llu | Z1 passes %llu | item passes %llu chunk passes %llu chunk steps %llu\n",
                acc[9] / 1e6, acc[10] / 1e6, acc[11] / 1e6, acc[12] / 1e6, acc[13] / 1e6, acc[14] / 1e6, acc[15] / 1e6, acc[16] / 1e6, acc[17] / 1e6, acc[18] / 1e6,
                acc[19], acc[20], acc[21], acc[22], acc[23], acc[24], acc[25], acc[26], acc[27]);
#ifndef BVG_PROF_WORK
    if ((a.dbg & 64u) && acc[14]) {                         // only the -DBVG_PROF build fills these
        fprintf(stderr, "[bvg] wave-cycles (M): phase1 %.0f, row prep %.0f, level prep %.0f, task set-up %.0f, seeks %.0f, merge loop %.0f\n", acc[14] / 1e6, acc[9] / 1e6, acc[10] / 1e6, acc[11] / 1e6, acc[12] / 1e6, acc[13] / 1e6);
        fprintf(stderr, "[bvg] phase 1 split (M): row set-up %.0f, headers %.0f, pool sizing %.0f, residuals %.0f; leaf pass %.0f (loop %.0f)\n", acc[15] / 1e6, acc[16] / 1e6, acc[17] / 1e6, acc[18] / 1e6, acc[20] / 1e6, acc[21] / 1e6);
        fprintf(stderr, "[bvg] scan kernel, more wave-cycles (M): compaction %.0f, window staging %.0f, residual task set-up %.0f, stored-list marking %.0f\n", acc[24] / 1e6, acc[25] / 1e6, acc[26] / 1e6, acc[27] / 1e6);
    }
#else
    if ((a.dbg & 64u) && (acc[24] | acc[25] | acc[26] | acc[27]))   // only the -DBVG_PROF -DBVG_PROF_WORK build (`make work`): the slots above hold counts, not cycles
        fprintf(stderr, "[bvg] scan kernel work: levels %llu | Z1 passes %llu | Z2 passes %llu tasks %llu steps %llu positions %llu | residual task passes %llu steps %llu residuals %llu | "
                "leaf item passes %llu chunk passes %llu steps(x4) %llu | stored lists %llu: with reference and extras %llu, d2 roots %llu, direct roots %llu | "
                "wave-wide interval fills: lists %llu intervals %llu elements %llu trips %llu\n",
                acc[9], acc[12], acc[10], acc[11], acc[13], acc[14], acc[15], acc[16], acc[17], acc[27], acc[20], acc[21], acc[24], acc[18], acc[25], acc[26],
                acc[kAccStride + 4], acc[kAccStride + 5], acc[kAccStride + 6], acc[kAccStride + 7]);
    if ((a.dbg & 64u) && (acc[28] | acc[29]))
        fprintf(stderr, "[bvg] scan kernel work, headers: copy-block loop steps (pairs) %llu for %llu blocks | interval loop steps %llu for %llu intervals\n", acc[28], acc[30], acc[29], acc[31]);
#endif
    if (bvg_scan_result* res = d.res) {
        const int64_t from = d.from, to = d.to; const uint32_t lo = d.lo, nblocks = d.nblocks;
        res->arcs = acc[0]; res->chk = acc[1]; res->nodes = acc[2];
        res->kernel_ms = d.kernel_ms; res->launches = d.launches; res->slow_blocks = d.slow_blocks; res->lean_blocks = lean_blocks;
        res->index_bytes = (uint64_t)(to - from + 1) * (d.sh->offs.lo ? 4 : 8) + (d.sh->offs.lo ? ((uint64_t)(to - from) >> kOffShift) * 8 : 0) + (uint64_t)nblocks * 20;
        res->index_entries = a.skip_first && d.skx->h_first.size() > (size_t)lo + nblocks ? d.skx->h_first[lo + nblocks] - d.skx->h_first[lo] : 0;
        if (a.skip_first) res->index_bytes += res->index_entries * (2 + d.esz) + (uint64_t)nblocks * 9;
        if (a.pos_first && d.skx->h_pos_first.size() > (size_t)lo + nblocks)       // recorded positions: the entries, a base and a flag per block, a bit per node
            res->index_bytes += (d.skx->h_pos_first[lo + nblocks] - d.skx->h_pos_first[lo]) * 2 + (uint64_t)nblocks * 9 + ((uint64_t)(to - from) >> 3);
        res->graph_bytes = 0;
    }
    if (acc[3] && dbg_on()) fprintf(stderr, "[bvg] error bits 0x%llx\n", acc[3]);
    if (acc[3] & ERR_REF_RANGE) return BVG_E_STATE;
    if (acc[3] & (ERR_OVERRUN | ERR_MALFORMED)) return BVG_E_EOF;
    return 0;
}

int run_decode(bvg_graph* g, int64_t from, int64_t to, bool materialise, const uint64_t* d_cum, int64_t* d_succ, int32_t* d_outdeg,
               bvg_scan_result* res, const BatchPlan* batch, const std::shared_ptr<Plan>* use_plan) {
    static const std::shared_ptr<Plan> no_plan = std::make_shared<Plan>();         // batch calls bring their own per-call plan
    std::shared_ptr<Plan> plp = use_plan ? *use_plan : no_plan;
    if (!batch && !use_plan) { const int r = build_plan(g, block_bits_of(g), plp); if (r) return r; }
    Decode d(g, std::move(plp), from, to, materialise, batch, res);
    bool done = false;                                      // (the skip index's build may have been this scan)
    int r = ensure_skip(d, done); if (r || done) return r;
    r = base_args(d, d_cum, d_succ, d_outdeg); if (r) return r;
    select_experiments(d);
    geometry(d);
    if (d.tier0_runs()) r = d.predict ? run_predicted(d) : run_unpredicted(d);
    else if (d.force_slow || d.force_giant) {
        d.work.resize(d.nblocks); for (uint32_t i = 0; i < d.nblocks; i++) d.work[i] = batch ? 2 * i : d.lo + i;
        d.slow_blocks = d.nblocks;
    }
    if (r) return r;
    r = cascade(d); if (r) return r;
    return finish(d);
}


}  // namespace bvghost
