// C++ twin of StronglyConnectedComponents.compute(g, computeBuckets = true) / computeSizes / sortBySize over the host mirror
// (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels).  Prints the component count, the largest size and the bucket counts; the
// pytest wrapper (tests/test_gpu_scc_cpp.py) compares them with the known answers for cnr-2000.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto g = BVGraph::load(argv[1]);
        auto scc = g->stronglyConnectedComponents(true);
        const int64_t k = scc.numberOfComponents;
        const std::vector<int64_t> plain = scc.computeSizes();
        int64_t total = 0, singletons = 0;
        for (int64_t s : plain) { total += s; singletons += s == 1; }
        int64_t bucket_nodes = 0;
        std::vector<uint8_t> is_bucket((size_t)k, 0);
        for (size_t x = 0; x < scc.buckets.size(); x++) if (scc.buckets[x]) { bucket_nodes++; is_bucket[(size_t)scc.component[x]] = 1; }
        int64_t bucket_comps = 0;
        for (uint8_t b : is_bucket) bucket_comps += b;
        const std::vector<int64_t> sizes = scc.sortBySize();
        if (scc.numberOfComponents != k || (int64_t)sizes.size() != k || total != g->numNodes()) { printf("FAIL counts %lld %lld %zu %lld\n", (long long)k, (long long)scc.numberOfComponents, sizes.size(), (long long)total); return 1; }
        for (size_t i = 1; i < sizes.size(); i++) if (sizes[i] > sizes[i - 1]) { printf("FAIL sizes not sorted at %zu\n", i); return 1; }
        if (scc.computeSizes() != sizes) { printf("FAIL sizes of the renumbered labels differ\n"); return 1; }
        printf("OK nodes=%lld count=%lld largest=%lld singletons=%lld bucket_components=%lld bucket_nodes=%lld\n", (long long)g->numNodes(), (long long)k,
               (long long)(sizes.empty() ? 0 : sizes[0]), (long long)singletons, (long long)bucket_comps, (long long)bucket_nodes);
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
