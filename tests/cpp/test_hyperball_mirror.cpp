// C++ twin of HyperBall.run over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels).  Runs log2m / seed / upper
// bound from the command line with both centralities, and prints the iteration reached, modified(), the neighbourhood function as the bits
// of its doubles, and checksums (the sum of (index + 1) * value, modulo 2^64) of the registers and of the bits of the two float arrays.  The pytest wrapper
// (tests/test_gpu_hyperball_cpp.py) compares them with the Python mirror and the numpy model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

static uint64_t chk_floats(const std::vector<float>& v) {
    uint64_t c = 0;
    for (size_t i = 0; i < v.size(); i++) { uint32_t b; memcpy(&b, &v[i], 4); c += ((uint64_t)i + 1) * (uint64_t)b; }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s basename log2m seed upper_bound\n", argv[0]); return 2; }
    try {
        auto g = BVGraph::load(argv[1]);
        const int log2m = atoi(argv[2]);
        HyperBall hb = g->hyperBall(log2m, (uint64_t)atoll(argv[3]), true, true);
        hb.run(atoll(argv[4]), -1);
        printf("RUN iteration=%lld modified=%lld\n", (long long)hb.iteration(), (long long)hb.modified());
        printf("NF");
        for (double x : hb.neighbourhoodFunction()) { uint64_t b; memcpy(&b, &x, 8); printf(" %016llx", (unsigned long long)b); }
        printf("\n");
        uint64_t c = 0;
        const int64_t n = g->numNodes(), step = 1 << 14;
        for (int64_t a = 0; a < n; a += step) {
            const int64_t b = a + step < n ? a + step : n;
            const std::vector<uint8_t> r = hb.registers(a, b);
            for (size_t i = 0; i < r.size(); i++) c += ((((uint64_t)a << log2m) + i) + 1) * (uint64_t)r[i];
        }
        double c0 = hb.count(0);
        uint64_t c0b; memcpy(&c0b, &c0, 8);
        printf("STATE registers=%016llx sod=%016llx sid=%016llx count0=%016llx\n", (unsigned long long)c, (unsigned long long)chk_floats(hb.sumOfDistances()),
               (unsigned long long)chk_floats(hb.sumOfInverseDistances()), (unsigned long long)c0b);
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
