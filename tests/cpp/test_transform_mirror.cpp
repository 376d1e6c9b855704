// C++ twin of the transforms over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels): loads a BVGraph, holds
// identity / transpose / symmetrise against what the mirror already returns (decodeRange, transposeCSR, symmetrizeCSR), checks the simplified
// graph, computes the three permutations, maps by the lexicographic one and back, stores the mapped graph, and prints what the pytest
// wrapper (tests/test_gpu_transform_cpp.py) compares with the model: sizes and checksums.
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

static bool holds(const ParsedGraph& g, const std::vector<uint64_t>& off, const std::vector<int64_t>& adj) {
    std::vector<uint64_t> o; std::vector<int64_t> a;
    g.csr(o, a);
    return o == off && a == adj;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto bv = BVGraph::load(argv[1]);
        const int64_t n = bv->numNodes();
        std::vector<int32_t> deg; std::vector<int64_t> succ;
        bv->decodeRange(0, n, deg, succ);
        std::vector<uint64_t> off((size_t)n + 1, 0);
        for (int64_t x = 0; x < n; x++) off[(size_t)x + 1] = off[(size_t)x] + (uint64_t)deg[(size_t)x];
        auto id = identityGraph(*bv);
        auto fromCsr = graphFromCSR(off, succ);
        printf("nodes %lld arcs %lld identity %d from_csr %d\n", (long long)id->numNodes(), (long long)id->numArcs(), (int)holds(*id, off, succ), (int)holds(*fromCsr, off, succ));

        std::vector<uint64_t> toff, soff; std::vector<int64_t> tsucc, ssucc;
        bv->transposeCSR(toff, tsucc); bv->symmetrizeCSR(soff, ssucc);
        auto tr = transposeGraph(*bv); auto sy = symmetrizeGraph(*id); auto un = unionGraphs(*bv, *tr);
        auto simple = simplifyGraph(*bv); auto simpleT = transposeGraph(*simple); auto noLoops = filterArcs(*sy, BVG_TRANSFORM_NO_LOOPS);
        std::vector<uint64_t> so; std::vector<int64_t> sa;
        simple->csr(so, sa);
        int64_t loops = 0;
        for (int64_t x = 0; x < n; x++) for (uint64_t i = so[(size_t)x]; i < so[(size_t)x + 1]; i++) loops += sa[(size_t)i] == x;
        printf("transpose_equal %d symmetrize_equal %d union_equal %d simplify_loops %lld simplify_symmetric %d simplify_is_filter %d\n", (int)holds(*tr, toff, tsucc),
               (int)holds(*sy, soff, ssucc), (int)holds(*un, soff, ssucc), (long long)loops, (int)holds(*simpleT, so, sa), (int)holds(*noLoops, so, sa));

        const std::vector<int64_t> lex = lexicographicalPermutation(*bv), gray = grayCodePermutation(*id), rnd = randomPermutation(*bv, 42);
        printf("lex_chk %016llx gray_chk %016llx random_chk %016llx\n", (unsigned long long)chk(lex), (unsigned long long)chk(gray), (unsigned long long)chk(rnd));
        auto mapped = mapGraph(*bv, lex);
        std::vector<int64_t> inv((size_t)n);
        for (int64_t x = 0; x < n; x++) inv[(size_t)lex[(size_t)x]] = x;
        auto back = mapGraph(*mapped, inv);
        std::vector<uint64_t> mo; std::vector<int64_t> ma;
        mapped->csr(mo, ma);
        bvg_params p; bvg_default_params(&p);
        std::vector<uint8_t> g1, g2; std::vector<uint64_t> o1, o2;
        mapped->store(p, g1, o1);
        BVGraph::store(p, mo, ma, g2, o2);
        printf("mapped nodes %lld arcs %lld off_chk %016llx adj_chk %016llx map_back %d store_equal %d graph_bytes %zu\n", (long long)mapped->numNodes(),
               (long long)mapped->numArcs(), (unsigned long long)chk(mo), (unsigned long long)chk(ma), (int)holds(*back, off, succ), (int)(g1 == g2 && o1 == o2), g1.size());
        try { mapGraph(*bv, std::vector<int64_t>(3, 0)); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        try { filterArcs(*bv, BVG_TRANSFORM_SAME_CLASS); printf("refusal none\n"); }
        catch (const std::invalid_argument&) { printf("refusal invalid_argument\n"); }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
