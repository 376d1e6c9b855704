// C++ twin of an EFGraph round trip over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels): loads a BVGraph,
// stores it as an EFGraph on the device (EFGraph::store), opens the result and prints what the pytest wrapper
// (tests/test_gpu_efgraph_cpp.py) compares with the golden lists: sizes, a checksum of every successor, the scans of both graphs and
// skipTo answers for a fixed set of (node, bound) pairs.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto bv = BVGraph::load(argv[1]);
        const int64_t n = bv->numNodes();
        std::vector<int32_t> deg; std::vector<int64_t> succ;
        bv->decodeRange(0, n, deg, succ);
        std::vector<uint64_t> adjOff((size_t)n + 1, 0);
        for (int64_t x = 0; x < n; x++) adjOff[(size_t)x + 1] = adjOff[(size_t)x] + (uint64_t)deg[(size_t)x];
        std::vector<uint8_t> graph; std::vector<uint64_t> offsets;
        EFGraph::store(adjOff, succ, n, 8, false, graph, offsets);
        bvg_ef_params p{}; p.nodes = n; p.arcs = (int64_t)succ.size(); p.upper_bound = n; p.log2_quantum = 8; p.big_endian = 0;
        auto ef = EFGraph::fromMemory(p, graph.data(), graph.size(), offsets.data());
        auto fly = ef->copy();
        std::vector<int32_t> edeg; std::vector<int64_t> esucc;
        fly->decodeRange(0, n, edeg, esucc);
        if (edeg != deg || esucc != succ) { printf("FAIL lists differ\n"); return 1; }
        uint64_t mix = 0;
        for (size_t i = 0; i < esucc.size(); i++) mix += (uint64_t)esucc[i] * (uint64_t)(i + 1);
        const bvg_scan_result a = ef->scan();
        std::vector<int64_t> nodes, bounds;
        for (int64_t x = 0; x < n; x += 997) for (int64_t b = 0; b <= n; b += n / 7) { nodes.push_back(x); bounds.push_back(b); }
        const std::vector<int64_t> got = ef->skipTo(nodes, bounds);
        uint64_t skipmix = 0; size_t agree = 0;
        for (size_t i = 0; i < got.size(); i++) {
            skipmix += (uint64_t)got[i] * (uint64_t)(i + 1);
            auto it = ef->successors(nodes[i]);                                                // the same answer from the host iterator
            const int64_t v = it.skipTo(bounds[i]);
            agree += (v == LazyLongSkippableIterator::END_OF_LIST ? -1 : v) == got[i];
        }
        printf("OK nodes=%lld arcs=%zu bytes=%zu bits=%llu mix=%llu\n", (long long)ef->numNodes(), esucc.size(), graph.size(), (unsigned long long)offsets[(size_t)n],
               (unsigned long long)mix);
        printf("SCAN nodes=%llu arcs=%llu chk=%llu outdegree0=%lld\n", (unsigned long long)a.nodes, (unsigned long long)a.arcs, (unsigned long long)a.chk, (long long)ef->outdegree(0));
        printf("SKIP queries=%zu agree=%zu mix=%llu\n", got.size(), agree, (unsigned long long)skipmix);
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
