// TEST INFRASTRUCTURE: a stand-alone program that replays bvg_successors_batch calls on ONE fresh handle of the emulated library, so that
// the sanitizer build (make replay_asan) checks the calls as an ordinary program, with nothing preloaded.
//   batch_replay <dir> <call> [<call> ...]
// <dir>/params.bin (a bvg_params), graph.bin, offsets.bin (uint64, nodes + 1 bit positions): the graph, opened with bvg_open_mem;
// <dir>/<call>.nodes (int64), .deg (int32), .succ (int64): the requests of a call and the answer it must give.  The calls run in the order given:
// every call asks with a buffer of exactly the expected size and compares outdegrees and successors element for element.
// tests/test_emu.py writes the files (the calls of test_workspace_growth_between_the_two_preparations of tests/test_gpu_batch.py) and runs this.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "bvgraph_hip.h"

template <class T>
static std::vector<T> read_all(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "batch_replay: cannot read %s\n", path.c_str()); exit(2); }
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> out(raw.size() / sizeof(T));
    if (!out.empty()) memcpy(out.data(), raw.data(), out.size() * sizeof(T));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: batch_replay <dir> <call> [<call> ...]\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<bvg_params> p = read_all<bvg_params>(dir + "params.bin");
    const std::vector<uint8_t> graph = read_all<uint8_t>(dir + "graph.bin");
    const std::vector<uint64_t> offsets = read_all<uint64_t>(dir + "offsets.bin");
    if (p.size() != 1 || (int64_t)offsets.size() != p[0].nodes + 1) { fprintf(stderr, "batch_replay: the files do not fit each other\n"); return 2; }
    bvg_graph* g = nullptr;
    int rc = bvg_open_mem(&p[0], graph.data(), graph.size(), offsets.data(), 0, &g);
    if (rc) { fprintf(stderr, "batch_replay: bvg_open_mem: %d\n", rc); return 1; }
    for (int a = 2; a < argc; a++) {
        const std::vector<int64_t> nodes = read_all<int64_t>(dir + argv[a] + ".nodes"), esucc = read_all<int64_t>(dir + argv[a] + ".succ");
        const std::vector<int32_t> edeg = read_all<int32_t>(dir + argv[a] + ".deg");
        std::vector<int32_t> deg(nodes.size());                              // (exactly as long as they may be written: a byte behind them is a report)
        std::vector<int64_t> succ(esucc.size());
        uint64_t n_succ = 0;
        rc = bvg_successors_batch(g, nodes.data(), (int64_t)nodes.size(), deg.data(), succ.empty() ? nullptr : succ.data(), succ.size(), &n_succ);
        if (rc || n_succ != esucc.size() || deg != edeg || succ != esucc) {
            fprintf(stderr, "batch_replay: call %s: status %d, %llu successors (expected %zu), outdegrees %s, successors %s\n", argv[a], rc, (unsigned long long)n_succ,
                    esucc.size(), deg == edeg ? "equal" : "DIFFER", succ == esucc ? "equal" : "DIFFER");
            return 1;
        }
        printf("call %s: %zu requests, %zu successors\n", argv[a], nodes.size(), esucc.size());
    }
    bvg_close(g);
    printf("replay ok\n");
    return 0;
}
