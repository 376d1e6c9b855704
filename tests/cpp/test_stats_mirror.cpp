// C++ twin of Stats.run over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels).  Prints the summary, the
// lengths and heads of both distributions and a checksum of the per-node indegrees; the pytest wrapper (tests/test_gpu_stats_cpp.py)
// compares them with the model's answers for cnr-2000.
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
        GraphStats st = g->stats(true);
        const bvg_stats_summary& s = st.summary;
        const std::vector<uint64_t> od = st.outdegreeDistribution(), id = st.indegreeDistribution();
        const std::vector<int64_t> in = st.indegrees();
        const std::vector<int64_t> tail = st.indegrees((int64_t)s.nodes - 3, -1);
        if (in.size() != (size_t)s.nodes || tail.size() != 3 || tail[0] != in[in.size() - 3] || tail[2] != in.back()) { printf("FAIL indegrees %zu %zu\n", in.size(), tail.size()); return 1; }
        uint64_t insum = 0, inmix = 0;
        for (size_t x = 0; x < in.size(); x++) { insum += (uint64_t)in[x]; inmix += (uint64_t)in[x] * (uint64_t)(x + 1); }
        printf("OK nodes=%llu arcs=%llu loops=%llu dangling=%llu terminal=%llu num_gaps=%llu tot_gap=%llu:%llu tot_loc=%llu:%llu\n", (unsigned long long)s.nodes,
               (unsigned long long)s.arcs, (unsigned long long)s.loops, (unsigned long long)s.dangling, (unsigned long long)s.terminal, (unsigned long long)s.num_gaps,
               (unsigned long long)s.tot_gap_hi, (unsigned long long)s.tot_gap_lo, (unsigned long long)s.tot_loc_hi, (unsigned long long)s.tot_loc_lo);
        printf("OUT min=%lld@%lld max=%lld@%lld len=%zu head=%llu,%llu,%llu\n", (long long)s.min_outdegree, (long long)s.min_outdegree_node, (long long)s.max_outdegree,
               (long long)s.max_outdegree_node, od.size(), (unsigned long long)od[0], (unsigned long long)od[1], (unsigned long long)od[2]);
        printf("IN min=%lld@%lld max=%lld@%lld len=%zu head=%llu,%llu,%llu sum=%llu mix=%llu\n", (long long)s.min_indegree, (long long)s.min_indegree_node, (long long)s.max_indegree,
               (long long)s.max_indegree_node, id.size(), (unsigned long long)id[0], (unsigned long long)id[1], (unsigned long long)id[2], (unsigned long long)insum,
               (unsigned long long)inmix);
        printf("BINS");
        for (int b = 0; b < 64; b++) printf("%c%llu", b ? ',' : ' ', (unsigned long long)s.log_delta[b]);
        printf("\n");
    } catch (const std::exception& e) {
        printf("FAIL exception %s\n", e.what());
        return 1;
    }
    return 0;
}
