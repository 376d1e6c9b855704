// C++ twin of ConnectedComponents.compute / computeSizes / sortBySize over the host mirror (webgraph-big_amd/host/bvgraph.hpp ->
// C ABI -> HIP kernels).  Prints the component count and checksums of the labels and sizes, plain and renumbered by size; the pytest
// wrapper (tests/test_gpu_components_cpp.py) compares them with a CPU union-find.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

static uint64_t label_chk(const std::vector<int64_t>& v) {
    uint64_t c = 0;
    for (size_t i = 0; i < v.size(); i++) c += bvg_arc_mix((uint64_t)i, (uint64_t)v[i]);
    return c;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto g = BVGraph::load(argv[1]);
        std::vector<int64_t> comp, sizes, comp2, sizes2;
        const int64_t k = g->connectedComponents(comp, &sizes);
        const int64_t k2 = g->connectedComponents(comp2, &sizes2, true);
        int64_t total = 0;
        for (int64_t s : sizes) total += s;
        if (k != k2 || (int64_t)sizes.size() != k || total != g->numNodes()) { printf("FAIL counts %lld %lld %zu %lld\n", (long long)k, (long long)k2, sizes.size(), (long long)total); return 1; }
        for (size_t i = 1; i < sizes2.size(); i++) if (sizes2[i] > sizes2[i - 1]) { printf("FAIL sizes not sorted at %zu\n", i); return 1; }
        printf("OK nodes=%lld count=%lld chk=%016llx sizes_chk=%016llx sorted_chk=%016llx sorted_sizes_chk=%016llx\n", (long long)g->numNodes(), (long long)k,
               (unsigned long long)label_chk(comp), (unsigned long long)label_chk(sizes), (unsigned long long)label_chk(comp2), (unsigned long long)label_chk(sizes2));
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
