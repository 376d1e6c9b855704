// C++ twin of the scattered arc list parser over the host mirror (webgraph-big_amd/host/bvgraph.hpp: parseScatteredArcs -> C ABI -> HIP
// kernels).  Every argument is one case, "<flags>:<text>" with flags out of S (symmetrize), L (no loops), K (the numbering 2, -1, 7 given in
// advance), X (strict) and the text with \n written as '|'.  Prints per case what the pytest wrapper (tests/test_gpu_scattered_cpp.py)
// compares with the model: the ids, the adjacency, the report -- or the record of the refusal.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../webgraph-big_amd/host/bvgraph.hpp"

using namespace webgraph;

int main(int argc, char** argv) {
    try {
        for (int c = 1; c < argc; c++) {
            const char* colon = strchr(argv[c], ':');
            if (!colon) { fprintf(stderr, "usage: %s flags:text...\n", argv[0]); return 2; }
            const std::string flags(argv[c], (size_t)(colon - argv[c]));
            std::string text(colon + 1);
            for (char& ch : text) if (ch == '|') ch = '\n';
            const std::vector<int64_t> known = {2, -1, 7};
            const bool given = flags.find('K') != std::string::npos;
            try {
                auto g = parseScatteredArcs(text, flags.find('S') != std::string::npos, flags.find('L') != std::string::npos, given ? &known : nullptr,
                                            flags.find('X') != std::string::npos);
                std::vector<uint64_t> off; std::vector<int64_t> adj;
                g->csr(off, adj);
                printf("nodes %lld arcs %lld ids", (long long)g->numNodes(), (long long)g->numArcs());
                for (int64_t v : g->ids()) printf(" %lld", (long long)v);
                printf("\noff");
                for (uint64_t v : off) printf(" %llu", (unsigned long long)v);
                printf("\nadj");
                for (int64_t v : adj) printf(" %lld", (long long)v);
                const bvg_scattered_report& r = g->report();
                printf("\nreport %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %lld %d\n", (unsigned long long)r.lines, (unsigned long long)r.arcs,
                       (unsigned long long)r.bad_source, (unsigned long long)r.bad_target, (unsigned long long)r.no_target, (unsigned long long)r.too_large,
                       (unsigned long long)r.trailing, (unsigned long long)r.unknown_source, (unsigned long long)r.unknown_target, (unsigned long long)r.dropped_loops,
                       (unsigned long long)r.first_byte, (long long)r.first_line, (int)r.first_reason);
            } catch (const TextRefusal& e) {
                printf("refusal %d %d %lld %llu\n", e.status, e.error.reason, (long long)e.error.line, (unsigned long long)e.error.byte);
            }
        }
        printf("OK\n");
        return 0;
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 1;
    }
}
