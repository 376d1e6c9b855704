// C++ twin of the graph product over the host mirror (webgraph-big_amd/host/bvgraph.hpp: composeGraphs -> bvg_compose -> HIP kernels): loads
// a BVGraph, composes it with itself, and prints what the pytest wrapper (tests/test_gpu_compose_cpp.py) compares with the model: sizes,
// the report and checksums of the result's two arrays; then two refusals.
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

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto bv = BVGraph::load(argv[1]);
        ComposeReport rep{};
        auto sq = composeGraphs(*bv, *bv, &rep);
        std::vector<uint64_t> off; std::vector<int64_t> adj;
        sq->csr(off, adj);
        printf("nodes %lld arcs %lld products %llu report_arcs %llu rows %llu\n", (long long)sq->numNodes(), (long long)sq->numArcs(), (unsigned long long)rep.products,
               (unsigned long long)rep.arcs, (unsigned long long)(rep.rows[0] + rep.rows[1] + rep.rows[2]));
        printf("off_chk %016llx adj_chk %016llx\n", (unsigned long long)chk(off), (unsigned long long)chk(adj));
        auto id = identityGraph(*bv);
        auto mixed = composeGraphs(*id, *bv);                                  // a ParsedGraph and a BVGraph source
        std::vector<uint64_t> off2; std::vector<int64_t> adj2;
        mixed->csr(off2, adj2);
        printf("mixed_equal %d\n", (int)(off2 == off && adj2 == adj));
        bvg_transform_src none; none.graph = nullptr; none.csr = nullptr;
        bvg_transform_src one = transformSource(*id);
        bvg_text* t = nullptr;
        try { check(bvg_compose(&none, &one, nullptr, &t), "compose"); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { check(bvg_compose(&one, &one, nullptr, nullptr), "compose"); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
