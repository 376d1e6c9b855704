// C++ twin of the labelled graph product over the host mirror (webgraph-big_amd/host/bvgraph.hpp: composeLabelled -> bvg_lcompose -> HIP kernels):
// the reference's own case (TransformTest.testLabelledCompose) under the five semirings, then one row of `lists` lists of the single successor 5
// with different labels (argv[1]; the caller forces a tier through the environment), and the refusals.  It prints what the pytest wrapper
// (tests/test_gpu_lcompose_cpp.py) compares with the model.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

struct Arrays { std::vector<uint64_t> off; std::vector<int64_t> adj; std::vector<int32_t> lab; };
static void print(const char* name, const LabelledGraph& g, const LabelledComposeReport& rep) {
    Arrays a; g.csr(a.off, a.adj, a.lab);
    printf("%s nodes %lld arcs %lld kind %d width %d rows %llu %llu %llu :", name, (long long)g.numNodes(), (long long)g.numArcs(), g.kind(), g.width(),
           (unsigned long long)rep.rows[0], (unsigned long long)rep.rows[1], (unsigned long long)rep.rows[2]);
    for (size_t x = 0; x + 1 < a.off.size(); x++)
        for (uint64_t i = a.off[x]; i < a.off[x + 1]; i++) printf(" %zu>%lld:%d", x, (long long)a.adj[i], a.lab[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s lists\n", argv[0]); return 2; }
    try {
        // 0 -> 1:2, 0 -> 2:10, 0 -> 3:1, 1 -> 2:4, 3 -> 2:1
        auto ref = LabelledGraph::fromCSR({0, 3, 4, 4, 5}, {1, 2, 3, 2, 2}, {2, 10, 1, 4, 1}, BVG_LABEL_GAMMA_INT);
        const Semiring all[5] = {SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS, SEMIRING_MAX_MIN, SEMIRING_MIN_MAX, SEMIRING_PLUS_TIMES};
        for (int s = 0; s < 5; s++) {
            LabelledComposeReport rep;
            auto r = composeLabelled(*ref, *ref, all[s], -1, &rep);
            print(("reference_" + std::to_string(s)).c_str(), *r, rep);
        }
        // node 0 -> nodes 6 .. 6 + lists - 1 (labels 1, 2, 3, 1, ...); node 6 + i -> 5 with label i + 1
        const int64_t lists = atoll(argv[1]), n = 6 + lists;
        Arrays g0, g1;
        g0.off.assign((size_t)n + 1, (uint64_t)lists); g0.off[0] = 0;
        g1.off.assign((size_t)n + 1, 0);
        for (int64_t i = 0; i < lists; i++) {
            g0.adj.push_back(6 + i); g0.lab.push_back((int32_t)(i % 3 + 1));
            g1.adj.push_back(5); g1.lab.push_back((int32_t)(i + 1));
        }
        for (int64_t x = 0; x <= n; x++) g1.off[(size_t)x] = (uint64_t)(x <= 6 ? 0 : x - 6);
        auto a = LabelledGraph::fromCSR(g0.off, g0.adj, g0.lab, BVG_LABEL_FIXED_INT, 20), b = LabelledGraph::fromCSR(g1.off, g1.adj, g1.lab, BVG_LABEL_FIXED_INT, 20);
        for (int s = 0; s < 5; s++) {
            LabelledComposeReport rep;
            auto r = composeLabelled(*a, *b, all[s], 31, &rep);
            print(("same_key_" + std::to_string(s)).c_str(), *r, rep);
        }
        LabelledComposeReport rep;
        composeLabelled(*ref, *ref, SEMIRING_MIN_PLUS, -1, &rep);
        printf("limits %llu %llu\n", (unsigned long long)rep.limit[0], (unsigned long long)rep.limit[1]);
        try { composeLabelled(*a, *b, SEMIRING_PLUS_TIMES, 3, &rep); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument out_of_range %llu first %lld %lld\n", (unsigned long long)rep.out_of_range, (long long)rep.first_row, (long long)rep.first_successor); }
        try { composeLabelled(*ref, *a, SEMIRING_MIN_PLUS); printf("refusal none\n"); }                 // different label classes
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { composeLabelled(*ref, *ref, (Semiring)9); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { composeLabelled(*ref, *ref, SEMIRING_MIN_PLUS, 8); printf("refusal none\n"); }            // a GammaCodedIntLabel has no width
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
