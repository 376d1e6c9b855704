// C++ twin of the labelled transforms over the host mirror (webgraph-big_amd/host/bvgraph.hpp: LabelledGraph, transposeLabelled, unionLabelled,
// symmetrizeLabelled, filterLabelledArcs -> bvg_lgraph_* -> HIP kernels): loads a BVGraph, labels arc (x, y) with (31 x + y) mod 2^13, and prints
// what the pytest wrapper (tests/test_gpu_labelled_cpp.py) compares with the model and the CPU label writer: sizes and checksums; then refusals.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

// the sum of (v[i] + 1) * (2 i + 1) modulo 2^64: depends on every position, and numpy computes it exactly
template <typename T> static uint64_t chk(const std::vector<T>& v) {
    uint64_t h = 0;
    for (size_t i = 0; i < v.size(); i++) h += ((uint64_t)v[i] + 1) * (2 * (uint64_t)i + 1);
    return h;
}

struct Arrays { std::vector<uint64_t> off; std::vector<int64_t> adj; std::vector<int32_t> lab; };
static Arrays arrays(const LabelledGraph& g) { Arrays a; g.csr(a.off, a.adj, a.lab); return a; }
static void print(const char* name, const LabelledGraph& g) {
    const Arrays a = arrays(g);
    printf("%s nodes %lld arcs %lld kind %d width %d off_chk %016llx adj_chk %016llx lab_chk %016llx\n", name, (long long)g.numNodes(), (long long)g.numArcs(), g.kind(), g.width(),
           (unsigned long long)chk(a.off), (unsigned long long)chk(a.adj), (unsigned long long)chk(a.lab));
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto bv = BVGraph::load(argv[1]);
        Arrays g;
        identityGraph(*bv)->csr(g.off, g.adj);
        g.lab.resize(g.adj.size());
        for (size_t x = 0; x + 1 < g.off.size(); x++)
            for (uint64_t i = g.off[x]; i < g.off[x + 1]; i++) g.lab[i] = (int32_t)((31 * (uint64_t)x + (uint64_t)g.adj[i]) % 8192);
        auto lg = LabelledGraph::fromCSR(g.off, g.adj, g.lab, BVG_LABEL_FIXED_INT, 13);
        print("source", *lg);
        auto t = transposeLabelled(*lg);
        print("transpose", *t);
        const Arrays back = arrays(*transposeLabelled(*t));
        std::vector<uint64_t> uoff, toff; std::vector<int64_t> uadj, tadj;
        t->underlying()->csr(uoff, uadj);
        transposeGraph(*bv)->csr(toff, tadj);
        printf("twice_equal %d underlying_equal %d\n", (int)(back.off == g.off && back.adj == g.adj && back.lab == g.lab), (int)(uoff == toff && uadj == tadj));
        auto s = symmetrizeLabelled(*lg, BVG_LMERGE_MIN);
        print("symmetrize_min", *s);
        const Arrays u = arrays(*unionLabelled(*lg, *t)), k = arrays(*symmetrizeLabelled(*lg));
        printf("union_is_symmetrize %d\n", (int)(u.off == k.off && u.adj == k.adj && u.lab == k.lab));
        print("lower_bound_4096", *filterLabelledArcs(*lg, BVG_LFILTER_LOWER_BOUND, std::vector<int64_t>(), 4096));
        print("no_loops", *filterLabelledArcs(*lg, BVG_LFILTER_NO_LOOPS));
        std::vector<uint8_t> stream; std::vector<uint64_t> loff;
        lg->storeLabels(stream, loff);
        printf("labels bytes %llu stream_chk %016llx offsets_chk %016llx\n", (unsigned long long)stream.size(), (unsigned long long)chk(stream), (unsigned long long)chk(loff));
        std::vector<int32_t> bad = g.lab; bad[bad.size() / 2] = 8192;              // 2^width: outside the class
        try { LabelledGraph::fromCSR(g.off, g.adj, bad, BVG_LABEL_FIXED_INT, 13); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { LabelledGraph::fromCSR(g.off, g.adj, g.lab, BVG_LABEL_FIXED_INT_LIST, 13); printf("refusal none\n"); }
        catch (const UnsupportedOperation&) { printf("refusal unsupported\n"); }
        auto gamma = LabelledGraph::fromCSR(g.off, g.adj, g.lab, BVG_LABEL_GAMMA_INT);
        try { unionLabelled(*lg, *gamma); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { symmetrizeLabelled(*lg, 7); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
