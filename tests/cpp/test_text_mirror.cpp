// C++ twin of a text graph round trip over the host mirror (webgraph-big_amd/host/bvgraph.hpp -> C ABI -> HIP kernels): loads a BVGraph,
// writes it as an ASCIIGraph text and as an arc list (storeASCIIGraph / storeArcList), reads both back (loadASCIIGraph / loadArcList),
// compresses the parsed graph where it lies and prints what the pytest wrapper (tests/test_gpu_text_cpp.py) compares with the golden
// files: sizes, checksums of the texts, whether the round trips and the stored bytes agree, and the record of one refusal.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

static uint64_t fnv(const std::string& s) { uint64_t h = 1469598103934665603ull; for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; } return h; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s basename\n", argv[0]); return 2; }
    try {
        auto bv = BVGraph::load(argv[1]);
        const int64_t n = bv->numNodes();
        std::vector<int32_t> deg; std::vector<int64_t> succ;
        bv->decodeRange(0, n, deg, succ);
        const std::string ascii = storeASCIIGraph(*bv);
        std::string pieces = std::to_string(n) + "\n";
        for (int64_t lo = 0; lo < n; lo += 100003) pieces += formatASCIIGraph(*bv, lo, lo + 100003 < n ? lo + 100003 : n);
        const std::string arcs = storeArcList(*bv, 5);
        std::string arcPieces;
        for (int64_t lo = 0; lo < n; lo += 77777) arcPieces += formatArcList(*bv, lo, lo + 77777 < n ? lo + 77777 : n, 5);
        auto pa = loadASCIIGraph(ascii);
        auto pl = loadArcList(arcs, -5, false, false, n);
        std::vector<uint64_t> off, off2; std::vector<int64_t> adj, adj2;
        pa->csr(off, adj); pl->csr(off2, adj2);
        bool same = adj == succ && off.size() == (size_t)n + 1 && off == off2 && adj == adj2;
        for (int64_t x = 0; same && x < n; x++) same = off[(size_t)x + 1] - off[(size_t)x] == (uint64_t)deg[(size_t)x];
        bvg_params p; bvg_default_params(&p);
        bvg_params q = bv->params();
        p.window_size = q.window_size; p.max_ref_count = q.max_ref_count; p.min_interval_length = q.min_interval_length; p.zeta_k = q.zeta_k;
        std::vector<uint8_t> g1, g2; std::vector<uint64_t> o1, o2;
        pa->store(p, g1, o1);
        BVGraph::store(p, off, adj, g2, o2);
        printf("nodes %lld arcs %lld\n", (long long)pa->numNodes(), (long long)pa->numArcs());
        printf("ascii_bytes %zu ascii_fnv %016llx pieces_equal %d\n", ascii.size(), (unsigned long long)fnv(ascii), (int)(pieces == ascii && arcPieces == arcs));
        printf("arcs_bytes %zu arcs_fnv %016llx\n", arcs.size(), (unsigned long long)fnv(arcs));
        printf("round_trips %d store_equal %d graph_bytes %zu graph_fnv %016llx\n", (int)same, (int)(g1 == g2 && o1 == o2), g1.size(),
               (unsigned long long)fnv(std::string(g1.begin(), g1.end())));
        try { loadASCIIGraph("3\n0 1\n2 2\n\n"); printf("refusal none\n"); }
        catch (const TextRefusal& e) { printf("refusal %d %d %lld %llu\n", e.status, e.error.reason, (long long)e.error.line, (unsigned long long)e.error.byte); }
        try { loadArcList("0 1\n2\n"); printf("refusal none\n"); }
        catch (const TextRefusal& e) { printf("refusal %d %d %lld %llu\n", e.status, e.error.reason, (long long)e.error.line, (unsigned long long)e.error.byte); }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
