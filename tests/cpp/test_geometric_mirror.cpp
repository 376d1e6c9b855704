// C++ twin of LinearGeometricCentrality.compute() over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels).
// Arguments: basename coefficients [from to], coefficients = harmonic | power:x | exp:x | table:a,b,... ; without a range every node is
// a source (compute()), and the object comes from the graph's factory.  Prints the centralities as the bits of their floats, the
// reachable counts, the histogram and the words per node; the pytest wrapper (tests/test_gpu_geometric_cpp.py) compares them with the model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

static void print(const LinearGeometricCentrality& c) {
    printf("C");
    for (float x : c.centrality) { uint32_t b; memcpy(&b, &x, 4); printf(" %08x", b); }
    printf("\nR");
    for (int64_t r : c.reachable) printf(" %lld", (long long)r);
    printf("\nH");
    for (uint64_t h : c.histogram) printf(" %llu", (unsigned long long)h);
    printf("\nOK sources=%zu words=%llu passes=%llu\n", c.centrality.size(), (unsigned long long)c.counters[3], (unsigned long long)c.counters[0]);
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: %s basename harmonic|power:x|exp:x|table:a,b,... [from to]\n", argv[0]); return 2; }
    try {
        auto g = BVGraph::load(argv[1]);
        const std::string spec = argv[2];
        const bool all = argc == 3;
        const int64_t from = all ? 0 : atoll(argv[3]), to = all ? g->numNodes() : atoll(argv[4]);
        auto run = [&](LinearGeometricCentrality c) { if (all) c.compute(); else c.compute(from, to); print(c); };
        if (spec == "harmonic") run(g->linearGeometricCentrality(HarmonicCoefficients()));
        else if (spec.rfind("power:", 0) == 0) run(g->linearGeometricCentrality(PowerLawCoefficients(atof(spec.c_str() + 6))));
        else if (spec.rfind("exp:", 0) == 0) run(LinearGeometricCentrality(g, ExponentialCoefficients(atof(spec.c_str() + 4))));
        else if (spec.rfind("table:", 0) == 0) {
            std::vector<double> t;
            for (const char* p = spec.c_str() + 6; *p;) { char* e; t.push_back(strtod(p, &e)); if (*e != ',') break; p = e + 1; }
            run(g->linearGeometricCentrality(t));
        } else { printf("FAIL unknown coefficients %s\n", spec.c_str()); return 1; }
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
