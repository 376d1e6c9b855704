// C++ twin of ParallelBreadthFirstVisit.visit / visitAll over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels).
// Prints, for a visit from each start given on the command line, the visited count, the maximum distance, the node at maximum distance and
// checksums of the queue, the cut points, the distances and the parents; then the round count and a checksum of the round markers of
// visitAll.  The pytest wrapper (tests/test_gpu_bfs_cpp.py) compares them with a CPU breadth-first search.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

template <typename V> static uint64_t chk(const V& v) {
    uint64_t c = 0;
    for (size_t i = 0; i < v.size(); i++) c += bvg_arc_mix((uint64_t)i, (uint64_t)(int64_t)v[i]);
    return c;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s basename start...\n", argv[0]); return 2; }
    try {
        auto g = BVGraph::load(argv[1]);
        for (int a = 2; a < argc; a++) {
            const int64_t start = atoll(argv[a]);
            ParallelBreadthFirstVisit v = g->breadthFirstVisit(false), p = g->breadthFirstVisit(true);
            const int64_t k = v.visit(start), kp = p.visit(start);
            if (k != kp || v.visit(start) != 0 || v.round() != 0) { printf("FAIL visit %lld: %lld %lld round %lld\n", (long long)start, (long long)k, (long long)kp, (long long)v.round()); return 1; }
            if (chk(v.queue()) != chk(p.queue()) || chk(v.dist()) != chk(p.dist())) { printf("FAIL parent and round visits differ from %lld\n", (long long)start); return 1; }
            printf("VISIT start=%lld visited=%lld maxdist=%lld far=%lld queue=%016llx cuts=%016llx dist=%016llx parents=%016llx\n", (long long)start, (long long)k,
                   (long long)v.maxDistance(), (long long)v.nodeAtMaxDistance(), (unsigned long long)chk(v.queue()), (unsigned long long)chk(v.cutPoints()),
                   (unsigned long long)chk(v.dist()), (unsigned long long)chk(p.marker()));
        }
        ParallelBreadthFirstVisit all = g->breadthFirstVisit();
        all.visitAll();
        printf("ALL rounds=%lld marker=%016llx\n", (long long)all.round() + 1, (unsigned long long)chk(all.marker()));
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
