// bvgraph.hpp — C++ host-side mirror of the reference's graph API for the decode path, over the C ABI
// of libbvgraph_hip.so (include/bvgraph_hip.h).  Header-only; link with -lbvgraph_hip.
//
// The reference is Java; there is no JVM in this image, so the host side above the C ABI is written in
// C++ with the reference's names, argument meaning and error behaviour (paths relative to
// /root/reference/src/it/unimi/dsi/big/webgraph):
//   LazyLongIterator.java:28-44          nextLong() -> next successor or -1; skip(n)
//   NodeIterator.java:34-133             hasNext / nextLong / outdegree / successors / successorBigArray / copy(upperBound) / skip
//   ImmutableGraph.java:245-447          numNodes / numArcs / randomAccess / outdegree / successors / successorBigArray /
//                                        nodeIterator(from) / splitNodeIterators(k) / copy()
//   BVGraph.java:1345-1464               load / loadMapped / loadOffline / loadSequential
// Error mapping: BVG_E_ARG -> std::invalid_argument (IllegalArgumentException),
// BVG_E_STATE -> std::logic_error (IllegalStateException), BVG_E_UNSUPPORTED -> UnsupportedOperation,
// BVG_E_IO/EOF -> std::ios_base::failure (IOException), nextLong() past the end -> std::out_of_range
// (NoSuchElementException).  A JNI shim is the same calls with jlong/jlongArray marshalling.
#pragma once
#include <cstdint>
#include <ios>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bvgraph_hip.h"

namespace webgraph {

struct UnsupportedOperation : std::runtime_error { using std::runtime_error::runtime_error; };
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

inline void check(int st, const char* what) {
    if (st == BVG_OK) return;
    std::string msg = std::string(what) + ": " + bvg_strerror(st);
    switch (st) {
        case BVG_E_ARG: throw std::invalid_argument(msg);
        case BVG_E_STATE: throw std::logic_error(msg);
        case BVG_E_UNSUPPORTED: throw UnsupportedOperation(msg);
        case BVG_E_IO: case BVG_E_EOF: throw std::ios_base::failure(msg);
        case BVG_E_NOMEM: throw std::bad_alloc();
        default: throw DeviceError(msg);
    }
}

// LazyLongIterators.wrap(array, n), LazyLongIterators.java:220-255
class LazyLongIterator {
    const int64_t* a_; int64_t n_, i_ = 0;
public:
    LazyLongIterator(const int64_t* a, int64_t n) : a_(a), n_(n) {}
    int64_t nextLong() { return i_ < n_ ? a_[i_++] : -1; }
    int64_t skip(int64_t n) { int64_t k = n < n_ - i_ ? n : n_ - i_; i_ += k; return k; }
};

class BVGraph;

// BVGraph.BVGraphNodeIterator (BVGraph.java:1100-1245): sequential scan served by batched GPU decodes.
class NodeIterator {
    std::shared_ptr<BVGraph> g_;
    int64_t from_, curr_, limit_, b0_ = 0, b1_ = 0, batch_;
    std::vector<int32_t> deg_; std::vector<int64_t> succ_; std::vector<uint64_t> cum_;
    void fill(int64_t x);
public:
    NodeIterator(std::shared_ptr<BVGraph> g, int64_t from, int64_t upperBound, int64_t batchNodes = 1 << 16);
    bool hasNext() const { return curr_ < limit_; }                                        // BVGraph.java:1179-1181
    int64_t nextLong() {                                                                   // BVGraph.java:1164-1176
        if (!hasNext()) throw std::out_of_range("NoSuchElementException");
        ++curr_;
        if (curr_ < b0_ || curr_ >= b1_) fill(curr_);
        return curr_;
    }
    int64_t outdegree() const { started(); return deg_[(size_t)(curr_ - b0_)]; }          // BVGraph.java:1206-1209
    // successorBigArray(): valid until the next nextLong() (NodeIterator.java:80-96)
    const int64_t* successorBigArray() const { started(); return succ_.data() + cum_[(size_t)(curr_ - b0_)]; }
    LazyLongIterator successors() const { return LazyLongIterator(successorBigArray(), outdegree()); }
    NodeIterator copy(int64_t upperBound) const;                                           // BVGraph.java:1223-1229
    int64_t skip(int64_t n) { int64_t k = 0; while (k < n && hasNext()) { nextLong(); k++; } return k; }
private:
    void started() const { if (curr_ == from_ - 1) throw std::logic_error("IllegalStateException"); }   // BVGraph.java:1185
};

class BVGraph : public std::enable_shared_from_this<BVGraph> {
    bvg_graph* h_ = nullptr; bvg_params p_{}; std::string basename_;
    explicit BVGraph(bvg_graph* h) : h_(h) { check(bvg_info(h_, &p_), "info"); }
public:
    ~BVGraph() { bvg_close(h_); }
    BVGraph(const BVGraph&) = delete;
    static std::shared_ptr<BVGraph> load(const std::string& basename, int device = 0, int mode = BVG_LOAD_STANDARD) {   // BVGraph.java:1345
        bvg_graph* h = nullptr; check(bvg_open(basename.c_str(), mode, device, &h), "load");
        auto g = std::shared_ptr<BVGraph>(new BVGraph(h)); g->basename_ = basename; return g;
    }
    static std::shared_ptr<BVGraph> loadMapped(const std::string& b, int device = 0) { return load(b, device, BVG_LOAD_MAPPED); }
    static std::shared_ptr<BVGraph> loadOffline(const std::string& b, int device = 0) { return load(b, device, BVG_LOAD_OFFLINE); }
    static std::shared_ptr<BVGraph> loadSequential(const std::string& b, int device = 0) { return load(b, device, BVG_LOAD_SEQUENTIAL); }
    static std::shared_ptr<BVGraph> fromMemory(const bvg_params& p, const uint8_t* graph, uint64_t nbytes, const uint64_t* offsets, int device = 0) {
        bvg_graph* h = nullptr; check(bvg_open_mem(&p, graph, nbytes, offsets, device, &h), "open_mem");
        return std::shared_ptr<BVGraph>(new BVGraph(h));
    }
    bvg_graph* handle() const { return h_; }
    int64_t numNodes() const { return p_.nodes; }
    int64_t numArcs() const { if (p_.arcs < 0) throw UnsupportedOperation("numArcs"); return p_.arcs; }     // ImmutableGraph.java:253-258
    bool randomAccess() const { return true; }
    bool hasCopiableIterators() const { return true; }
    const std::string& basename() const { return basename_; }
    int windowSize() const { return p_.window_size; }
    int maxRefCount() const { return p_.max_ref_count; }
    int minIntervalLength() const { return p_.min_interval_length; }
    std::shared_ptr<BVGraph> copy() const {                                                // BVGraph.java:553-578
        bvg_graph* h = nullptr; check(bvg_copy(h_, &h), "copy");
        auto g = std::shared_ptr<BVGraph>(new BVGraph(h)); g->basename_ = basename_; return g;
    }
    int64_t outdegree(int64_t x) {                                                         // BVGraph.java:821-842
        if (x < 0 || x >= p_.nodes) throw std::invalid_argument("Node index out of range");
        int32_t d; check(bvg_outdegrees(h_, x, x + 1, &d), "outdegree"); return d;
    }
    const bvg_params& params() const { return p_; }
    // how much index the scans of this handle build and use (bvg_tuning.no_index): 0 = the full residual skip index, 1 = none, 2 = marks only (validation marks + entries for
    // lists of >= 4 096 residuals: ~0.03 % of the stream instead of ~50 %)
    void setIndexMode(int mode) { bvg_tuning t{}; t.no_index = (uint32_t)mode; check(bvg_set_tuning(h_, &t), "set_tuning"); }
    // BVGraph.store on the device (bvg_store; BVG:2404-2457 with chunkNodes > 0, the single-threaded store with 0): the bytes of
    // basename.graph and the bit offsets (basename.offsets holds their gamma-coded gaps)
    static void store(const bvg_params& p, const std::vector<uint64_t>& adjOff, const std::vector<int64_t>& adj, std::vector<uint8_t>& graph,
                      std::vector<uint64_t>& offsets, int64_t chunkNodes = 0, int device = 0) {
        uint8_t* g = nullptr; uint64_t nb = 0; uint64_t* o = nullptr;
        const int64_t n = (int64_t)adjOff.size() - 1;
        static const int64_t none = 0;
        check(bvg_store(&p, n, adjOff.data(), adj.empty() ? &none : adj.data(), chunkNodes, device, &g, &nb, &o), "store");
        graph.assign(g, g + nb); offsets.assign(o, o + n + 1);
        bvg_free(g); bvg_free(o);
    }
    // decode of [from,to): outdegrees + concatenated successor lists
    void decodeRange(int64_t from, int64_t to, std::vector<int32_t>& deg, std::vector<int64_t>& succ) {
        deg.resize((size_t)(to > from ? to - from : 0));
        uint64_t need = 0;
        int st = bvg_decode_range(h_, from, to, deg.data(), nullptr, 0, &need);
        if (st != BVG_E_CAPACITY) check(st, "decode_range");
        succ.resize((size_t)need);
        if (need) check(bvg_decode_range(h_, from, to, deg.data(), succ.data(), need, &need), "decode_range");
    }
    std::vector<int64_t> successorBigArray(int64_t x) {                                    // BVGraph.java:860-867
        if (x < 0 || x >= p_.nodes) throw std::invalid_argument("Node index out of range");
        std::vector<int32_t> d; std::vector<int64_t> s; decodeRange(x, x + 1, d, s); return s;
    }
    // successors(x) for a whole frontier (bvg_successors_batch): outdegrees + concatenated lists in request order
    void successorsBatch(const std::vector<int64_t>& nodes, std::vector<int32_t>& deg, std::vector<int64_t>& succ) {
        deg.resize(nodes.size());
        uint64_t need = 0;
        int st = bvg_successors_batch(h_, nodes.data(), (int64_t)nodes.size(), deg.data(), nullptr, 0, &need);
        if (st != BVG_E_CAPACITY) check(st, "successors_batch");
        succ.resize((size_t)need);
        if (need) check(bvg_successors_batch(h_, nodes.data(), (int64_t)nodes.size(), deg.data(), succ.data(), need, &need), "successors_batch");
    }
    // the transpose in CSR form (decode + device sort; Transform.transposeOffline, Transform.java:1058-1160)
    void transposeCSR(std::vector<uint64_t>& toffsets, std::vector<int64_t>& tsucc) {
        toffsets.resize((size_t)p_.nodes + 1);
        uint64_t need = 0;
        int st = bvg_transpose(h_, toffsets.data(), nullptr, 0, &need);
        if (st != BVG_E_CAPACITY) check(st, "transpose");
        tsucc.resize((size_t)need);
        if (need) check(bvg_transpose(h_, toffsets.data(), tsucc.data(), need, &need), "transpose");
    }
    // the symmetrised graph in CSR form (Transform.symmetrizeOffline, Transform.java:546-575: union with the transpose)
    void symmetrizeCSR(std::vector<uint64_t>& soffsets, std::vector<int64_t>& ssucc) {
        soffsets.resize((size_t)p_.nodes + 1);
        uint64_t need = 0;
        int st = bvg_symmetrize(h_, soffsets.data(), nullptr, 0, &need);
        if (st != BVG_E_CAPACITY) check(st, "symmetrize");
        ssucc.resize((size_t)need);
        if (need) check(bvg_symmetrize(h_, soffsets.data(), ssucc.data(), need, &need), "symmetrize");
    }
    // weakly connected components (ConnectedComponents.compute + computeSizes / sortBySize, algo/ConnectedComponents.java) by a
    // union-find on the device: comp[x] for every node, sizes per component when asked for; returns the number of components
    int64_t connectedComponents(std::vector<int64_t>& comp, std::vector<int64_t>* sizes = nullptr, bool sortBySize = false) {
        const size_t n = (size_t)p_.nodes;
        comp.resize(n);
        if (sizes) sizes->resize(n ? n : 1);                                                // (there are at most n components)
        uint64_t count = 0;
        check(bvg_components(h_, sortBySize ? BVG_CC_SORT_BY_SIZE : 0u, n ? comp.data() : nullptr, sizes ? sizes->data() : nullptr, sizes ? (uint64_t)sizes->size() : 0,
                             &count), "components");
        if (sizes) sizes->resize((size_t)count);
        return (int64_t)count;
    }
    // strongly connected components (algo/StronglyConnectedComponents.java) on the device: the class is below
    inline class StronglyConnectedComponents stronglyConnectedComponents(bool computeBuckets = false);
    // graph statistics on the device (Stats.java): the class is below
    inline class GraphStats stats(bool keepIndegrees = false);
    // exact geometric centralities on the device (algo/LinearGeometricCentrality.java): the class and the coefficient objects are below
    template <typename Coeffs> inline class LinearGeometricCentrality linearGeometricCentrality(const Coeffs& coeffs);
    // breadth-first visits on the device (algo/ParallelBreadthFirstVisit.java): the class is below
    inline class ParallelBreadthFirstVisit breadthFirstVisit(bool parent = false);
    // HyperBall on the device (algo/HyperBall.java, standard iterations): the class is below
    inline class HyperBall hyperBall(int log2m, uint64_t seed = 0, bool sumOfDistances = false, bool harmonic = false);
    NodeIterator nodeIterator(int64_t from = 0) { return NodeIterator(shared_from_this(), from, INT64_MAX); }   // BVGraph.java:1257
    std::vector<NodeIterator> splitNodeIterators(int howMany) {                            // ImmutableGraph.java:405-436
        std::vector<NodeIterator> v; const int64_t n = p_.nodes, m = (n + howMany - 1) / howMany;
        for (int i = 0; i < howMany; i++) {
            int64_t lo = (int64_t)i * m < n ? (int64_t)i * m : n, hi = lo + m < n ? lo + m : n;
            v.emplace_back(lo < n ? copy() : shared_from_this(), lo, hi);
        }
        return v;
    }
    bvg_scan_result scan(int64_t from = 0, int64_t to = -1) {                               // the SpeedTest loop, test/SpeedTest.java:127-141
        bvg_scan_result r; check(bvg_scan(h_, from, to < 0 ? p_.nodes : to, &r), "scan"); return r;
    }
};

// StronglyConnectedComponents (algo/StronglyConnectedComponents.java) over bvg_scc: what compute() leaves -- numberOfComponents, component[]
// and, with computeBuckets, buckets[] (one byte per node, 0 / 1) -- plus computeSizes() and sortBySize().  The partition, the count, the
// sizes and the buckets are the reference's; the numbering is by smallest node, not Tarjan's emission order (include/bvgraph_hip.h).
class StronglyConnectedComponents {
    std::shared_ptr<BVGraph> g_;
    void run(uint32_t flags, std::vector<int64_t>* sizes) {
        const size_t n = (size_t)g_->numNodes();
        component.resize(n);
        if (sizes) sizes->resize(n ? n : 1);                                                // (there are at most n components)
        if (hasBuckets) buckets.resize(n ? n : 1);
        uint64_t count = 0;
        check(bvg_scc(g_->handle(), flags | (hasBuckets ? BVG_SCC_BUCKETS : 0u), n ? component.data() : nullptr, sizes ? sizes->data() : nullptr,
                      sizes ? (uint64_t)sizes->size() : 0, &count, hasBuckets ? buckets.data() : nullptr, counters), "scc");
        if (sizes) sizes->resize((size_t)count);
        if (hasBuckets) buckets.resize(n);
        numberOfComponents = (int64_t)count;
    }
public:
    int64_t numberOfComponents = 0;
    std::vector<int64_t> component;
    std::vector<uint8_t> buckets; bool hasBuckets = false;
    uint64_t counters[BVG_SCC_COUNTERS] = {};
    StronglyConnectedComponents(std::shared_ptr<BVGraph> g, bool computeBuckets) : g_(std::move(g)), hasBuckets(computeBuckets) { run(0u, nullptr); }
    // the size of every component, in the numbering component[] has now
    std::vector<int64_t> computeSizes() {
        std::vector<int64_t> sizes((size_t)numberOfComponents, 0);
        for (int64_t c : component) sizes[(size_t)c]++;
        return sizes;
    }
    // renumbers component[] by decreasing size (ties: smallest node first) and returns the sizes in the new order
    std::vector<int64_t> sortBySize() {
        std::vector<int64_t> sizes;
        run(BVG_SCC_SORT_BY_SIZE, &sizes);
        return sizes;
    }
};
inline StronglyConnectedComponents BVGraph::stronglyConnectedComponents(bool computeBuckets) { return StronglyConnectedComponents(shared_from_this(), computeBuckets); }

// GraphStats (Stats.java) over bvg_stats_*: what one pass of Stats.run counts -- the summary (arcs, loops, dangling and terminal nodes, the
// degree extremes with the reference's tie rules, the gap and locality sums as 128-bit values in two words, the binned gap histogram),
// both degree distributions and, with keepIndegrees, the indegree of every node (kept on the device, copied on request).
class GraphStats {
    bvg_stats* s_ = nullptr;
    std::vector<uint64_t> distribution(int which) const {
        uint64_t len = 0;
        int st = bvg_stats_distribution(s_, which, nullptr, 0, &len);
        if (st != BVG_E_CAPACITY) check(st, "stats_distribution");
        std::vector<uint64_t> out((size_t)len);
        check(bvg_stats_distribution(s_, which, out.data(), len, &len), "stats_distribution");
        return out;
    }
public:
    bvg_stats_summary summary{};
    GraphStats(BVGraph& g, bool keepIndegrees);
    ~GraphStats() { if (s_) bvg_stats_close(s_); }
    GraphStats(const GraphStats&) = delete; GraphStats& operator=(const GraphStats&) = delete;
    GraphStats(GraphStats&& o) noexcept : s_(o.s_), summary(o.summary) { o.s_ = nullptr; }
    std::vector<uint64_t> outdegreeDistribution() const { return distribution(BVG_STATS_OUT); }
    std::vector<uint64_t> indegreeDistribution() const { return distribution(BVG_STATS_IN); }
    // the indegrees of [from, to) (to < 0: up to the last node); needs keepIndegrees
    std::vector<int64_t> indegrees(int64_t from = 0, int64_t to = -1) {
        if (to < 0) to = (int64_t)summary.nodes;
        std::vector<int64_t> out(to > from ? (size_t)(to - from) : 0);
        check(bvg_stats_indegrees(s_, from, to, out.empty() ? nullptr : out.data()), "stats_indegrees");
        return out;
    }
};
inline GraphStats::GraphStats(BVGraph& g, bool keepIndegrees) {
    check(bvg_stats_compute(g.handle(), keepIndegrees ? BVG_STATS_KEEP_INDEGREES : 0u, &s_), "stats_compute");
    check(bvg_stats_get(s_, &summary), "stats_get");
}
inline GraphStats BVGraph::stats(bool keepIndegrees) { return GraphStats(*this, keepIndegrees); }

// The coefficient objects of LinearGeometricCentrality (LinearGeometricCentrality.java:82-124): get(d) is what the library evaluates.
struct HarmonicCoefficients { double get(int64_t d) const { return d == 0 ? 0.0 : 1.0 / (double)d; } };
struct PowerLawCoefficients { double exponent; explicit PowerLawCoefficients(double e) : exponent(e) {} };
struct ExponentialCoefficients { double base; explicit ExponentialCoefficients(double b) : base(b) {} };

// LinearGeometricCentrality (algo/LinearGeometricCentrality.java) over bvg_geometric: compute() fills centrality[] (float) and reachable[]
// for every node, or for the sources [from, to) given to it.  Coefficients: one of the three objects above or a std::vector<double> (coeff(d)
// = v[d], 0 beyond its end).  The sum is formed in double and rounded to float once; the reference rounds once per reached node.
class LinearGeometricCentrality {
    std::shared_ptr<BVGraph> g_;
    int kind_; double param_ = 0; std::vector<double> table_;
public:
    std::vector<float> centrality;
    std::vector<int64_t> reachable;
    std::vector<uint64_t> histogram;                                                        // pairs (source, node) by distance, over the sources of the last compute()
    uint64_t counters[BVG_GEO_COUNTERS] = {};
    LinearGeometricCentrality(std::shared_ptr<BVGraph> g, const HarmonicCoefficients&) : g_(std::move(g)), kind_(BVG_GEO_HARMONIC) {}
    LinearGeometricCentrality(std::shared_ptr<BVGraph> g, const PowerLawCoefficients& c) : g_(std::move(g)), kind_(BVG_GEO_POWER_LAW), param_(c.exponent) {}
    LinearGeometricCentrality(std::shared_ptr<BVGraph> g, const ExponentialCoefficients& c) : g_(std::move(g)), kind_(BVG_GEO_EXPONENTIAL), param_(c.base) {}
    LinearGeometricCentrality(std::shared_ptr<BVGraph> g, const std::vector<double>& table) : g_(std::move(g)), kind_(BVG_GEO_TABLE), table_(table) {}
    void compute() { compute(0, g_->numNodes()); }
    void compute(int64_t from, int64_t to) {
        const size_t count = to > from ? (size_t)(to - from) : 0;
        centrality.assign(count, 0.0f); reachable.assign(count, 0);
        histogram.assign((size_t)g_->numNodes() + 1, 0);                                    // (distances are below the number of nodes)
        uint64_t len = 0;
        check(bvg_geometric(g_->handle(), kind_, param_, table_.empty() ? nullptr : table_.data(), (uint64_t)table_.size(), from, to, count ? centrality.data() : nullptr,
                            count ? reachable.data() : nullptr, histogram.data(), (uint64_t)histogram.size(), &len, counters), "linearGeometricCentrality");
        histogram.resize((size_t)len);
    }
};
template <typename Coeffs> inline LinearGeometricCentrality BVGraph::linearGeometricCentrality(const Coeffs& coeffs) { return LinearGeometricCentrality(shared_from_this(), coeffs); }

// ParallelBreadthFirstVisit (algo/ParallelBreadthFirstVisit.java) over bvg_bfs_*: marker / round / queue / cutPoints live on the device
// between visits; inside a level the queue is in increasing id, and with parent = true a node's parent is the smallest node of the
// previous level that has it as a successor.  dist() is the level of every node of the last visit (-1: not reached).
class ParallelBreadthFirstVisit {
    bvg_bfs* v_ = nullptr; int64_t n_ = 0;
public:
    ParallelBreadthFirstVisit(BVGraph& g, bool parent) : n_(g.numNodes()) { check(bvg_bfs_create(g.handle(), parent ? BVG_BFS_PARENT : 0u, &v_), "bfs_create"); }
    ParallelBreadthFirstVisit(ParallelBreadthFirstVisit&& o) noexcept : v_(o.v_), n_(o.n_) { o.v_ = nullptr; }
    ParallelBreadthFirstVisit(const ParallelBreadthFirstVisit&) = delete;
    ParallelBreadthFirstVisit& operator=(const ParallelBreadthFirstVisit&) = delete;
    ~ParallelBreadthFirstVisit() { bvg_bfs_close(v_); }
    void clear() { check(bvg_bfs_clear(v_), "bfs_clear"); }
    int64_t visit(int64_t start) { uint64_t k = 0; check(bvg_bfs_visit(v_, start, &k), "bfs_visit"); return (int64_t)k; }
    void visitAll() { check(bvg_bfs_visit_all(v_), "bfs_visit_all"); }
    int64_t round() const { int64_t r = 0; check(bvg_bfs_info(v_, &r, nullptr, nullptr), "bfs_info"); return r; }
    int64_t maxDistance() const { uint64_t c = 0; check(bvg_bfs_info(v_, nullptr, nullptr, &c), "bfs_info"); return (int64_t)c - 2; }
    std::vector<int64_t> queue() const {
        uint64_t q = 0; check(bvg_bfs_info(v_, nullptr, &q, nullptr), "bfs_info");
        std::vector<int64_t> out((size_t)q);
        if (q) check(bvg_bfs_get(v_, nullptr, out.data(), q, nullptr, 0, nullptr), "bfs_get");
        return out;
    }
    std::vector<uint64_t> cutPoints() const {
        uint64_t c = 0; check(bvg_bfs_info(v_, nullptr, nullptr, &c), "bfs_info");
        std::vector<uint64_t> out((size_t)c);
        if (c) check(bvg_bfs_get(v_, nullptr, nullptr, 0, out.data(), c, nullptr), "bfs_get");
        return out;
    }
    std::vector<int64_t> marker() const { std::vector<int64_t> out((size_t)n_); if (n_) check(bvg_bfs_get(v_, out.data(), nullptr, 0, nullptr, 0, nullptr), "bfs_get"); return out; }
    std::vector<int32_t> dist() const { std::vector<int32_t> out((size_t)n_); if (n_) check(bvg_bfs_get(v_, nullptr, nullptr, 0, nullptr, 0, out.data()), "bfs_get"); return out; }
    int64_t nodeAtMaxDistance() const { const std::vector<int64_t> q = queue(); if (q.empty()) throw std::out_of_range("nodeAtMaxDistance: empty queue"); return q.back(); }
};
inline ParallelBreadthFirstVisit BVGraph::breadthFirstVisit(bool parent) { return ParallelBreadthFirstVisit(*this, parent); }

// HyperBall (algo/HyperBall.java, non-systolic in-memory iterations) over bvg_hyperball_*: the counters live on the device between
// iterations.  The hash behind the counters is this library's (include/bvgraph_hip.h); the algorithm and the estimator are the reference's.
class HyperBall {
    bvg_hyperball* h_ = nullptr; int64_t n_ = 0; int log2m_ = 0;
    std::vector<float> centrality(int which, const char* what) const { std::vector<float> out((size_t)n_); check(bvg_hyperball_centrality(h_, which, n_ ? out.data() : nullptr), what); return out; }
public:
    HyperBall(BVGraph& g, int log2m, uint64_t seed, bool sumOfDistances, bool harmonic) : n_(g.numNodes()), log2m_(log2m) {
        check(bvg_hyperball_create(g.handle(), log2m, (sumOfDistances ? BVG_HB_SUM_OF_DISTANCES : 0u) | (harmonic ? BVG_HB_HARMONIC : 0u), seed, &h_), "hyperball_create");
    }
    HyperBall(HyperBall&& o) noexcept : h_(o.h_), n_(o.n_), log2m_(o.log2m_) { o.h_ = nullptr; }
    HyperBall(const HyperBall&) = delete;
    HyperBall& operator=(const HyperBall&) = delete;
    ~HyperBall() { bvg_hyperball_close(h_); }
    void init(uint64_t seed = 0) { check(bvg_hyperball_init(h_, seed), "hyperball_init"); }
    void iterate() { check(bvg_hyperball_iterate(h_), "hyperball_iterate"); }
    void run(int64_t upperBound = -1, double threshold = -1) { check(bvg_hyperball_run(h_, upperBound, threshold), "hyperball_run"); }
    int64_t iteration() const { int64_t i = 0; check(bvg_hyperball_info(h_, &i, nullptr, nullptr, nullptr), "hyperball_info"); return i; }
    int64_t modified() const { uint64_t m = 0; check(bvg_hyperball_info(h_, nullptr, &m, nullptr, nullptr), "hyperball_info"); return (int64_t)m; }
    double relativeIncrement() const { double r = 0; check(bvg_hyperball_info(h_, nullptr, nullptr, &r, nullptr), "hyperball_info"); return r; }
    std::vector<double> neighbourhoodFunction() const {
        uint64_t k = 0; check(bvg_hyperball_info(h_, nullptr, nullptr, nullptr, &k), "hyperball_info");
        std::vector<double> out((size_t)k);
        if (k) check(bvg_hyperball_neighbourhood_function(h_, out.data(), k), "hyperball_neighbourhood_function");
        return out;
    }
    std::vector<uint8_t> registers(int64_t from, int64_t to) const {
        std::vector<uint8_t> out((size_t)(to - from) << log2m_);
        check(bvg_hyperball_registers(h_, from, to, out.empty() ? nullptr : out.data()), "hyperball_registers");
        return out;
    }
    std::vector<double> counts(int64_t from, int64_t to) const {
        std::vector<double> out((size_t)(to - from));
        check(bvg_hyperball_counts(h_, from, to, out.empty() ? nullptr : out.data()), "hyperball_counts");
        return out;
    }
    double count(int64_t x) const { return counts(x, x + 1)[0]; }
    std::vector<float> sumOfDistances() const { return centrality(BVG_HB_WHICH_SUM_OF_DISTANCES, "sumOfDistances"); }
    std::vector<float> sumOfInverseDistances() const { return centrality(BVG_HB_WHICH_HARMONIC, "sumOfInverseDistances"); }
    std::vector<float> closeness() const { return centrality(BVG_HB_WHICH_CLOSENESS, "closeness"); }
    std::vector<float> lin() const { return centrality(BVG_HB_WHICH_LIN, "lin"); }
    std::vector<float> nieminen() const { return centrality(BVG_HB_WHICH_NIEMINEN, "nieminen"); }
    std::vector<float> reachable() const { return centrality(BVG_HB_WHICH_REACHABLE, "reachable"); }
    static double relativeStandardDeviation(int log2m) { return bvg_hyperball_relative_standard_deviation(log2m); }
};
inline HyperBall BVGraph::hyperBall(int log2m, uint64_t seed, bool sumOfDistances, bool harmonic) { return HyperBall(*this, log2m, seed, sumOfDistances, harmonic); }

inline NodeIterator::NodeIterator(std::shared_ptr<BVGraph> g, int64_t from, int64_t upperBound, int64_t batchNodes)
    : g_(std::move(g)), from_(from), curr_(from - 1), batch_(batchNodes) {
    const int64_t n = g_->numNodes();
    if (from < 0 || from > n) throw std::invalid_argument("Node index out of range");     // BVGraph.java:1128
    limit_ = (upperBound < n ? upperBound : n) - 1;                                        // BVGraph.java:1148
    b0_ = b1_ = from;
}
inline void NodeIterator::fill(int64_t x) {
    int64_t hi = x + batch_ < limit_ + 1 ? x + batch_ : limit_ + 1;
    g_->decodeRange(x, hi, deg_, succ_);
    cum_.assign(deg_.size() + 1, 0);
    for (size_t i = 0; i < deg_.size(); i++) cum_[i + 1] = cum_[i] + (uint64_t)deg_[i];
    b0_ = x; b1_ = hi;
}
inline NodeIterator NodeIterator::copy(int64_t upperBound) const { return NodeIterator(g_->copy(), curr_ + 1, upperBound, batch_); }

// labelling/BitStreamArcLabelledImmutableGraph.java: an underlying BVGraph plus one int label per arc (GammaCodedIntLabel /
// FixedWidthIntLabel) and the list labels (FixedWidthIntListLabel, FixedWidthLongListLabel), all decoded on the device.  decodeRange is one batch of the labelled node iterator (:565-582);
// successors(x) positions at the node's label offset (:208-229).
class BitStreamArcLabelledImmutableGraph {
    std::shared_ptr<BVGraph> g_; bvg_labels* l_ = nullptr;
    BitStreamArcLabelledImmutableGraph(std::shared_ptr<BVGraph> g, bvg_labels* l) : g_(std::move(g)), l_(l) {}
public:
    ~BitStreamArcLabelledImmutableGraph() { bvg_labels_close(l_); }
    BitStreamArcLabelledImmutableGraph(const BitStreamArcLabelledImmutableGraph&) = delete;
    static std::shared_ptr<BitStreamArcLabelledImmutableGraph> load(const std::string& basename, int device = 0) {     // :378-484
        char under[4096];                                                                      // the property file names the underlying graph
        check(bvg_labels_read_properties(basename.c_str(), nullptr, nullptr, under, sizeof under), "labels properties");
        auto g = BVGraph::load(under, device);
        bvg_labels* l = nullptr; check(bvg_labels_open(basename.c_str(), g->numNodes(), device, &l, nullptr, 0), "labels");
        return std::shared_ptr<BitStreamArcLabelledImmutableGraph>(new BitStreamArcLabelledImmutableGraph(g, l));
    }
    std::shared_ptr<BVGraph> underlying() const { return g_; }
    bvg_labels* handle() const { return l_; }
    int64_t numNodes() const { return g_->numNodes(); }
    void decodeRange(int64_t from, int64_t to, std::vector<int32_t>& deg, std::vector<int64_t>& succ, std::vector<int32_t>& lab) {
        g_->decodeRange(from, to, deg, succ);
        lab.resize(succ.size());
        uint64_t n = 0;
        check(bvg_labels_decode_range(l_, from, to, deg.data(), lab.data(), lab.size(), &n), "labels_decode_range");
    }
    // list labels (FixedWidthIntListLabel.java:73-78, FixedWidthLongListLabel.java:81-87): listOff[arcs + 1] = where each arc's list
    // starts in `values`
    void decodeRangeLists(int64_t from, int64_t to, std::vector<int32_t>& deg, std::vector<int64_t>& succ, std::vector<uint64_t>& listOff, std::vector<int64_t>& values) {
        g_->decodeRange(from, to, deg, succ);
        listOff.assign(succ.size() + 1, 0);
        int kind = 0, width = 0; int64_t nodes = 0; uint64_t sb = 0;
        check(bvg_labels_info(l_, &kind, &width, &nodes, &sb), "labels_info");
        uint64_t n = 0;
        if (kind == BVG_LABEL_FIXED_LONG_LIST) {
            int st = bvg_labels_decode_range_lists64(l_, from, to, deg.data(), listOff.data(), nullptr, 0, &n);
            if (st != BVG_E_CAPACITY) check(st, "labels_decode_range_lists64");
            values.resize(n);
            if (n) check(bvg_labels_decode_range_lists64(l_, from, to, deg.data(), listOff.data(), values.data(), n, &n), "labels_decode_range_lists64");
        } else {
            int st = bvg_labels_decode_range_lists(l_, from, to, deg.data(), listOff.data(), nullptr, 0, &n);
            if (st != BVG_E_CAPACITY) check(st, "labels_decode_range_lists");
            std::vector<int32_t> v32(n);
            if (n) check(bvg_labels_decode_range_lists(l_, from, to, deg.data(), listOff.data(), v32.data(), n, &n), "labels_decode_range_lists");
            values.assign(v32.begin(), v32.end());
        }
    }
};

// EFGraph.java: the quasi-succinct format, decoded on the device (bvg_ef_*).  successors(x) is a LazyLongSkippableIterator over the
// node's list (skipTo on the host copy); skipTo(nodes, bounds) is the batched device form: for each pair, skipTo(bound) on a fresh
// iterator (EFGraph.java:1098-1160), defined on the real successors only.  store: EFGraph.store (:773-820) on the device.
class LazyLongSkippableIterator {
    std::vector<int64_t> a_; size_t i_ = 0; int64_t last_ = INT64_MIN;
public:
    static constexpr int64_t END_OF_LIST = INT64_MAX;
    explicit LazyLongSkippableIterator(std::vector<int64_t> a) : a_(std::move(a)) {}
    int64_t nextLong() { if (i_ < a_.size()) return last_ = a_[i_++]; last_ = END_OF_LIST; return -1; }
    int64_t skipTo(int64_t lowerBound) {                                                       // LazyLongSkippableIterator.java
        if (lowerBound <= last_) return last_;
        while (i_ < a_.size() && a_[i_] < lowerBound) i_++;
        return last_ = i_ < a_.size() ? a_[i_++] : END_OF_LIST;
    }
};

class EFGraph {
    bvg_efgraph* h_ = nullptr; bvg_ef_params p_{}; std::string basename_;
    explicit EFGraph(bvg_efgraph* h) : h_(h) { check(bvg_ef_info(h_, &p_), "ef_info"); }
public:
    ~EFGraph() { bvg_ef_close(h_); }
    EFGraph(const EFGraph&) = delete;
    static std::shared_ptr<EFGraph> load(const std::string& basename, int device = 0, int mode = BVG_LOAD_STANDARD) {       // EFGraph.java:542-750
        bvg_efgraph* h = nullptr; check(bvg_ef_open(basename.c_str(), mode, device, &h), "EFGraph.load");
        auto g = std::shared_ptr<EFGraph>(new EFGraph(h)); g->basename_ = basename; return g;
    }
    static std::shared_ptr<EFGraph> loadOffline(const std::string& b, int device = 0) { return load(b, device, BVG_LOAD_OFFLINE); }
    static std::shared_ptr<EFGraph> fromMemory(const bvg_ef_params& p, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, int device = 0) {
        bvg_efgraph* h = nullptr; check(bvg_ef_open_mem(&p, bytes, nbytes, offsets, device, &h), "ef_open_mem");
        return std::shared_ptr<EFGraph>(new EFGraph(h));
    }
    bvg_efgraph* handle() const { return h_; }
    int64_t numNodes() const { return p_.nodes; }
    int64_t numArcs() const { if (p_.arcs < 0) throw UnsupportedOperation("numArcs"); return p_.arcs; }
    int64_t upperBound() const { return p_.upper_bound; }
    int log2Quantum() const { return p_.log2_quantum; }
    bool randomAccess() const { return true; }
    const std::string& basename() const { return basename_; }
    std::shared_ptr<EFGraph> copy() const {                                                    // EFGraph.java:1173-1176
        bvg_efgraph* h = nullptr; check(bvg_ef_copy(h_, &h), "ef_copy");
        auto g = std::shared_ptr<EFGraph>(new EFGraph(h)); g->basename_ = basename_; return g;
    }
    int64_t outdegree(int64_t x) {                                                             // EFGraph.java:1008-1014
        if (x < 0 || x >= p_.nodes) throw std::invalid_argument("Node index out of range");
        int32_t d; check(bvg_ef_outdegrees(h_, x, x + 1, &d), "ef_outdegree"); return d;
    }
    void decodeRange(int64_t from, int64_t to, std::vector<int32_t>& deg, std::vector<int64_t>& succ) {
        deg.resize((size_t)(to > from ? to - from : 0));
        uint64_t need = 0;
        int st = bvg_ef_decode_range(h_, from, to, deg.data(), nullptr, 0, &need);
        if (st != BVG_E_CAPACITY) check(st, "ef_decode_range");
        succ.resize((size_t)need);
        if (need) check(bvg_ef_decode_range(h_, from, to, deg.data(), succ.data(), need, &need), "ef_decode_range");
    }
    LazyLongSkippableIterator successors(int64_t x) {                                          // EFGraph.java:1168-1171
        if (x < 0 || x >= p_.nodes) throw std::invalid_argument("Node index out of range");
        std::vector<int32_t> d; std::vector<int64_t> s; decodeRange(x, x + 1, d, s); return LazyLongSkippableIterator(std::move(s));
    }
    std::vector<int64_t> skipTo(const std::vector<int64_t>& nodes, const std::vector<int64_t>& bounds) {
        if (nodes.size() != bounds.size()) throw std::invalid_argument("skipTo: one bound per node");
        std::vector<int64_t> out(nodes.size());
        if (!nodes.empty()) check(bvg_ef_skip_to_batch(h_, nodes.data(), bounds.data(), (int64_t)nodes.size(), out.data()), "ef_skip_to_batch");
        return out;
    }
    bvg_scan_result scan(int64_t from = 0, int64_t to = -1) { bvg_scan_result r; check(bvg_ef_scan(h_, from, to < 0 ? p_.nodes : to, &r), "ef_scan"); return r; }
    static void store(const std::vector<uint64_t>& adjOff, const std::vector<int64_t>& adj, int64_t upperBound, int log2Quantum, bool bigEndian,
                      std::vector<uint8_t>& graph, std::vector<uint64_t>& offsets, int device = 0) {
        uint8_t* g = nullptr; uint64_t nb = 0; uint64_t* o = nullptr;
        const int64_t n = (int64_t)adjOff.size() - 1;
        static const int64_t none = 0;
        check(bvg_ef_store(n, upperBound, log2Quantum, bigEndian ? 1 : 0, adjOff.data(), adj.empty() ? &none : adj.data(), device, &g, &nb, &o), "ef_store");
        graph.assign(g, g + nb); offsets.assign(o, o + n + 1);
        bvg_free(g); bvg_free(o);
    }
};

// ---- text graphs (ASCIIGraph.java, ArcListASCIIGraph.java) over bvg_text_*: a refusal carries the record of the first offending byte
struct TextRefusal : std::runtime_error {
    int status; bvg_text_error error;
    TextRefusal(int st, const bvg_text_error& e, const std::string& what)
        : std::runtime_error(what + ": reason " + std::to_string(e.reason) + " at line " + std::to_string(e.line) + ", byte " + std::to_string(e.byte)), status(st), error(e) {}
};

// a parsed text graph: its adjacency in CSR form, resident on the device
class ParsedGraph {
    bvg_text* t_; int64_t n_ = 0; uint64_t m_ = 0;
public:
    explicit ParsedGraph(bvg_text* t) : t_(t) {                              // owns t from here on: closed if the constructor fails
        const int st = bvg_text_info(t_, &n_, &m_);
        if (st != BVG_OK) { bvg_text_close(t_); check(st, "text_info"); }
    }
    ParsedGraph(const ParsedGraph&) = delete; ParsedGraph& operator=(const ParsedGraph&) = delete;
    ~ParsedGraph() { bvg_text_close(t_); }
    int64_t numNodes() const { return n_; }
    int64_t numArcs() const { return (int64_t)m_; }
    bvg_text* handle() const { return t_; }
    void csr(std::vector<uint64_t>& adjOff, std::vector<int64_t>& adj) const {
        adjOff.resize((size_t)n_ + 1); adj.resize((size_t)m_);
        check(bvg_text_get(t_, adjOff.data(), adjOff.size(), m_ ? adj.data() : nullptr, m_), "text_get");
    }
    // BVGraph.store of the resident CSR: the bytes of BVGraph::store on csr()
    void store(const bvg_params& p, std::vector<uint8_t>& graph, std::vector<uint64_t>& offsets, int64_t chunkNodes = 0) const {
        uint8_t* g = nullptr; uint64_t nb = 0; uint64_t* o = nullptr;
        check(bvg_text_store(t_, &p, chunkNodes, &g, &nb, &o), "text_store");
        graph.assign(g, g + nb); offsets.assign(o, o + n_ + 1);
        bvg_free(g); bvg_free(o);
    }
};

inline std::unique_ptr<ParsedGraph> finishParse(int st, bvg_text* t, const bvg_text_error& e, const char* what) {
    if (st != BVG_OK && e.reason != 0) throw TextRefusal(st, e, what);
    check(st, what);
    return std::unique_ptr<ParsedGraph>(new ParsedGraph(t));
}
// ASCIIGraph.load on a text in memory: the node count, then one line of successors per node
inline std::unique_ptr<ParsedGraph> loadASCIIGraph(const std::string& text, int device = 0) {
    bvg_text* t = nullptr; bvg_text_error e{};
    const int st = bvg_text_parse_ascii(text.data(), text.size(), device, &t, &e);
    return finishParse(st, t, e, "loadASCIIGraph");
}
// ArcListASCIIGraph / ScatteredArcsASCIIGraph on a text in memory: `source TAB target` lines in any order
inline std::unique_ptr<ParsedGraph> loadArcList(const std::string& text, int64_t shift = 0, bool symmetrize = false, bool noLoops = false, int64_t minNodes = 0, int device = 0) {
    bvg_text* t = nullptr; bvg_text_error e{};
    const int st = bvg_text_parse_arcs(text.data(), text.size(), shift, (symmetrize ? BVG_TEXT_SYMMETRIZE : 0u) | (noLoops ? BVG_TEXT_NO_LOOPS : 0u), minNodes, device, &t, &e);
    return finishParse(st, t, e, "loadArcList");
}
// ScatteredArcsASCIIGraph on a text in memory: `source target` lines whose identifiers are any integers of [-2^63, 2^63).  Every newly seen
// identifier gets the next node number (ids()[node] is the identifier), offending lines are counted in report() and skipped -- refused
// (TextRefusal, reason BVG_SCATTERED_*) with strict.  knownIds: a numbering given in advance; lines that mention other identifiers are skipped.
class ScatteredGraph : public ParsedGraph {
    bvg_scattered_report rep_;
public:
    ScatteredGraph(bvg_text* t, const bvg_scattered_report& rep) : ParsedGraph(t), rep_(rep) {}
    const bvg_scattered_report& report() const { return rep_; }
    std::vector<int64_t> ids() const {
        std::vector<int64_t> v((size_t)numNodes());
        check(bvg_scattered_ids(handle(), v.empty() ? nullptr : v.data(), v.size()), "scattered_ids");
        return v;
    }
};
inline std::unique_ptr<ScatteredGraph> parseScatteredArcs(const std::string& text, bool symmetrize = false, bool noLoops = false, const std::vector<int64_t>* knownIds = nullptr,
                                                          bool strict = false, int device = 0) {
    bvg_text* t = nullptr; bvg_text_error e{}; bvg_scattered_report rep{};
    static const int64_t none = 0;
    const int st = bvg_scattered_parse(text.data(), text.size(), (symmetrize ? BVG_TEXT_SYMMETRIZE : 0u) | (noLoops ? BVG_TEXT_NO_LOOPS : 0u) | (strict ? BVG_TEXT_STRICT : 0u),
                                       knownIds ? (knownIds->empty() ? &none : knownIds->data()) : nullptr, knownIds ? (int64_t)knownIds->size() : 0, device, &t, &rep, &e);
    if (st != BVG_OK && e.reason != 0) throw TextRefusal(st, e, "parseScatteredArcs");
    check(st, "parseScatteredArcs");
    return std::unique_ptr<ScatteredGraph>(new ScatteredGraph(t, rep));
}
// the lines of nodes [from, to) as ASCIIGraph.store writes them (never a header line), and their arcs as ArcListASCIIGraph.store writes them
inline std::string formatASCIIGraph(BVGraph& g, int64_t from, int64_t to) {
    uint64_t need = 0;
    int st = bvg_text_format_ascii(g.handle(), from, to, nullptr, 0, &need);
    if (st != BVG_E_CAPACITY) check(st, "formatASCIIGraph");
    std::string body((size_t)need, '\0');
    if (need) check(bvg_text_format_ascii(g.handle(), from, to, &body[0], need, &need), "formatASCIIGraph");
    return body;
}
inline std::string formatArcList(BVGraph& g, int64_t from, int64_t to, int64_t shift = 0) {
    uint64_t need = 0;
    int st = bvg_text_format_arcs(g.handle(), from, to, shift, nullptr, 0, &need);
    if (st != BVG_E_CAPACITY) check(st, "formatArcList");
    std::string body((size_t)need, '\0');
    if (need) check(bvg_text_format_arcs(g.handle(), from, to, shift, &body[0], need, &need), "formatArcList");
    return body;
}
// ASCIIGraph.store / ArcListASCIIGraph.store of the whole graph into a string: the text of basename.graph-txt (the node count on a line of
// its own, then every node's line), the text of the arc list
inline std::string storeASCIIGraph(BVGraph& g) { return std::to_string(g.numNodes()) + "\n" + formatASCIIGraph(g, 0, g.numNodes()); }
inline std::string storeArcList(BVGraph& g, int64_t shift = 0) { return formatArcList(g, 0, g.numNodes(), shift); }

// ---- Transform (Transform.java) over bvg_transform_*: every source is a BVGraph or a ParsedGraph, every graph-valued result a ParsedGraph
// that stays on the device -- the source of the next call, or stored with ParsedGraph::store
inline bvg_transform_src transformSource(BVGraph& g) { bvg_transform_src s; s.graph = g.handle(); s.csr = nullptr; return s; }
inline bvg_transform_src transformSource(const ParsedGraph& g) { bvg_transform_src s; s.graph = nullptr; s.csr = g.handle(); return s; }
inline std::unique_ptr<ParsedGraph> finishTransform(int st, bvg_text* t, const char* what) {
    check(st, what);
    return std::unique_ptr<ParsedGraph>(new ParsedGraph(t));
}
// a resident graph over a CSR in host memory, validated as BVGraph::store validates its input
inline std::unique_ptr<ParsedGraph> graphFromCSR(const std::vector<uint64_t>& adjOff, const std::vector<int64_t>& adj, int device = 0) {
    if (adjOff.empty()) throw std::invalid_argument("graphFromCSR: adjOff holds nodes + 1 entries");
    bvg_text* t = nullptr;
    const int st = bvg_transform_from_csr((int64_t)adjOff.size() - 1, adjOff.data(), adj.empty() ? nullptr : adj.data(), device, &t);
    return finishTransform(st, t, "graphFromCSR");
}
template <class G> std::unique_ptr<ParsedGraph> identityGraph(G& g) {
    bvg_text* t = nullptr; const bvg_transform_src s = transformSource(g);
    const int st = bvg_transform_identity(&s, &t);
    return finishTransform(st, t, "identityGraph");
}
// Transform.mapOffline: -1 deletes a node; the result has max(map) + 1 nodes
template <class G> std::unique_ptr<ParsedGraph> mapGraph(G& g, const std::vector<int64_t>& map) {
    bvg_text* t = nullptr; const bvg_transform_src s = transformSource(g);
    const int st = bvg_transform_map(&s, map.empty() ? nullptr : map.data(), (int64_t)map.size(), &t);
    return finishTransform(st, t, "mapGraph");
}
// Transform.filterArcs: kind = BVG_TRANSFORM_NO_LOOPS (no classes), BVG_TRANSFORM_SAME_CLASS / _DIFFERENT_CLASS (NodeClassFilter)
template <class G> std::unique_ptr<ParsedGraph> filterArcs(G& g, int kind, const std::vector<int64_t>& nodeClass = std::vector<int64_t>()) {
    bvg_text* t = nullptr; const bvg_transform_src s = transformSource(g);
    const int st = bvg_transform_filter(&s, kind, nodeClass.empty() ? nullptr : nodeClass.data(), (int64_t)nodeClass.size(), &t);
    return finishTransform(st, t, "filterArcs");
}
template <class G> std::unique_ptr<ParsedGraph> transposeGraph(G& g) {
    bvg_text* t = nullptr; const bvg_transform_src s = transformSource(g);
    const int st = bvg_transform_transpose(&s, &t);
    return finishTransform(st, t, "transposeGraph");
}
// Transform.symmetrizeOffline; dropLoops: Transform.simplifyOffline
template <class G> std::unique_ptr<ParsedGraph> symmetrizeGraph(G& g, bool dropLoops = false) {
    bvg_text* t = nullptr; const bvg_transform_src s = transformSource(g);
    const int st = bvg_transform_symmetrize(&s, dropLoops ? BVG_TRANSFORM_DROP_LOOPS : 0u, &t);
    return finishTransform(st, t, "symmetrizeGraph");
}
template <class G> std::unique_ptr<ParsedGraph> simplifyGraph(G& g) { return symmetrizeGraph(g, true); }
// Transform.union; dropLoops: Transform.simplify(g, t)
template <class A, class B> std::unique_ptr<ParsedGraph> unionGraphs(A& a, B& b, bool dropLoops = false) {
    bvg_text* t = nullptr; const bvg_transform_src sa = transformSource(a), sb = transformSource(b);
    const int st = bvg_transform_union(&sa, &sb, dropLoops ? BVG_TRANSFORM_DROP_LOOPS : 0u, &t);
    return finishTransform(st, t, "unionGraphs");
}
// Transform.compose (unlabelled): row x = the sorted union of b's lists over a's successors of x; max(nodes) nodes, a successor b does not
// have contributes nothing.  report: products, arcs, the rows each tier took (bvg_compose_report)
typedef bvg_compose_report ComposeReport;
template <class A, class B> std::unique_ptr<ParsedGraph> composeGraphs(A& a, B& b, ComposeReport* report = nullptr) {
    bvg_text* t = nullptr; const bvg_transform_src sa = transformSource(a), sb = transformSource(b);
    const int st = bvg_compose(&sa, &sb, report, &t);
    return finishTransform(st, t, "composeGraphs");
}
// perm[node] = the node's new name (kind = BVG_PERM_LEX / BVG_PERM_GRAY / BVG_PERM_RANDOM), ready for mapGraph
template <class G> std::vector<int64_t> permutation(G& g, int kind, uint64_t seed = 0) {
    std::vector<int64_t> perm((size_t)g.numNodes());
    const bvg_transform_src s = transformSource(g);
    check(bvg_transform_permutation(&s, kind, seed, perm.empty() ? nullptr : perm.data()), "permutation");
    return perm;
}
template <class G> std::vector<int64_t> lexicographicalPermutation(G& g) { return permutation(g, BVG_PERM_LEX); }
template <class G> std::vector<int64_t> grayCodePermutation(G& g) { return permutation(g, BVG_PERM_GRAY); }
template <class G> std::vector<int64_t> randomPermutation(G& g, uint64_t seed) { return permutation(g, BVG_PERM_RANDOM, seed); }

// ---- arc-labelled graphs on the device (bvg_lgraph_*): a CSR resident on the device plus one int label per arc and the label class
// (BVG_LABEL_GAMMA_INT / BVG_LABEL_FIXED_INT).  The labelled half of Transform goes from LabelledGraph to LabelledGraph; storeLabels is
// BitStreamArcLabelledImmutableGraph.store's label stream, written on the device
class LabelledGraph {
    bvg_lgraph* l_; int64_t n_ = 0; uint64_t m_ = 0; int kind_ = 0, width_ = 0;
public:
    explicit LabelledGraph(bvg_lgraph* l) : l_(l) {                          // owns l from here on: closed if the constructor fails
        const int st = bvg_lgraph_info(l_, &n_, &m_, &kind_, &width_);
        if (st != BVG_OK) { bvg_lgraph_close(l_); check(st, "lgraph_info"); }
    }
    LabelledGraph(const LabelledGraph&) = delete; LabelledGraph& operator=(const LabelledGraph&) = delete;
    ~LabelledGraph() { bvg_lgraph_close(l_); }
    // a resident graph over a CSR and its labels in host memory: the CSR validated as graphFromCSR validates it, every label against its class
    static std::unique_ptr<LabelledGraph> fromCSR(const std::vector<uint64_t>& adjOff, const std::vector<int64_t>& adj, const std::vector<int32_t>& labels, int kind,
                                                  int width = 0, int device = 0) {
        if (adjOff.empty() || labels.size() != adj.size()) throw std::invalid_argument("LabelledGraph::fromCSR: adjOff holds nodes + 1 entries, labels one per arc");
        bvg_lgraph* l = nullptr;
        check(bvg_lgraph_from_csr((int64_t)adjOff.size() - 1, adjOff.data(), adj.empty() ? nullptr : adj.data(), labels.empty() ? nullptr : labels.data(), kind, width, device, &l),
              "LabelledGraph::fromCSR");
        return std::unique_ptr<LabelledGraph>(new LabelledGraph(l));
    }
    // a BitStreamArcLabelledImmutableGraph, decoded once
    static std::unique_ptr<LabelledGraph> fromGraph(BitStreamArcLabelledImmutableGraph& g) {
        bvg_lgraph* l = nullptr;
        check(bvg_lgraph_from_labelled(g.underlying()->handle(), g.handle(), &l), "LabelledGraph::fromGraph");
        return std::unique_ptr<LabelledGraph>(new LabelledGraph(l));
    }
    int64_t numNodes() const { return n_; }
    int64_t numArcs() const { return (int64_t)m_; }
    int kind() const { return kind_; }
    int width() const { return width_; }
    bvg_lgraph* handle() const { return l_; }
    void csr(std::vector<uint64_t>& adjOff, std::vector<int64_t>& adj, std::vector<int32_t>& labels) const {
        adjOff.resize((size_t)n_ + 1); adj.resize((size_t)m_); labels.resize((size_t)m_);
        check(bvg_lgraph_get(l_, adjOff.data(), adjOff.size(), m_ ? adj.data() : nullptr, m_, m_ ? labels.data() : nullptr, m_), "lgraph_get");
    }
    // the unlabelled graph as a ParsedGraph of its own: every unlabelled transform and ParsedGraph::store apply to it
    std::unique_ptr<ParsedGraph> underlying() const {
        bvg_text* t = nullptr;
        check(bvg_lgraph_underlying(l_, &t), "lgraph_underlying");
        return std::unique_ptr<ParsedGraph>(new ParsedGraph(t));
    }
    // the bytes of basename.labels and the nodes + 1 label offsets (bit positions)
    void storeLabels(std::vector<uint8_t>& stream, std::vector<uint64_t>& labelOffsets) const {
        uint8_t* s = nullptr; uint64_t nb = 0; uint64_t* o = nullptr;
        check(bvg_lgraph_store_labels(l_, &s, &nb, &o), "lgraph_store_labels");
        stream.assign(s, s + nb); labelOffsets.assign(o, o + n_ + 1);
        bvg_free(s); bvg_free(o);
    }
};
inline std::unique_ptr<LabelledGraph> finishLabelled(int st, bvg_lgraph* l, const char* what) {
    check(st, what);
    return std::unique_ptr<LabelledGraph>(new LabelledGraph(l));
}
// Transform.transposeOffline on a labelled graph: arc (x, y) with label l becomes (y, x) with label l
inline std::unique_ptr<LabelledGraph> transposeLabelled(const LabelledGraph& g) {
    bvg_lgraph* l = nullptr;
    const int st = bvg_lgraph_transpose(g.handle(), &l);
    return finishLabelled(st, l, "transposeLabelled");
}
// Transform.union with a merge strategy (BVG_LMERGE_KEEP_FIRST / _MIN / _MAX): an arc of both gets merge(label_a, label_b)
inline std::unique_ptr<LabelledGraph> unionLabelled(const LabelledGraph& a, const LabelledGraph& b, int strategy = BVG_LMERGE_KEEP_FIRST) {
    bvg_lgraph* l = nullptr;
    const int st = bvg_lgraph_union(a.handle(), b.handle(), strategy, &l);
    return finishLabelled(st, l, "unionLabelled");
}
// Transform.compose with a LabelSemiring (bvg_lcompose): the successors of composeGraphs on the underlying graphs, and on (x, z) the semiring's sum
// over every y with x -> y in a and y -> z in b of label_a(x, y) (x) label_b(y, z).  outWidth: the width of a FixedWidthIntLabel result (-1: the
// sources').  Exact arithmetic: a label outside the result's class throws std::invalid_argument, with the count and the first such arc in *report
enum Semiring { SEMIRING_MIN_PLUS = BVG_SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS = BVG_SEMIRING_MAX_PLUS, SEMIRING_MAX_MIN = BVG_SEMIRING_MAX_MIN,
                SEMIRING_MIN_MAX = BVG_SEMIRING_MIN_MAX, SEMIRING_PLUS_TIMES = BVG_SEMIRING_PLUS_TIMES };
typedef bvg_lcompose_report LabelledComposeReport;
inline std::unique_ptr<LabelledGraph> composeLabelled(const LabelledGraph& a, const LabelledGraph& b, Semiring semiring, int outWidth = -1, LabelledComposeReport* report = nullptr) {
    bvg_lgraph* l = nullptr;
    const int st = bvg_lcompose(a.handle(), b.handle(), (int)semiring, outWidth, report, &l);
    return finishLabelled(st, l, "composeLabelled");
}
// Transform.symmetrizeOffline on a labelled graph: union(g, transpose(g), strategy)
inline std::unique_ptr<LabelledGraph> symmetrizeLabelled(const LabelledGraph& g, int strategy = BVG_LMERGE_KEEP_FIRST) {
    bvg_lgraph* l = nullptr;
    const int st = bvg_lgraph_symmetrize(g.handle(), strategy, &l);
    return finishLabelled(st, l, "symmetrizeLabelled");
}
// Transform.filterArcs with a LabelledArcFilter: kind = BVG_LFILTER_NO_LOOPS, _SAME_CLASS / _DIFFERENT_CLASS (nodeClass), or _LOWER_BOUND
// (Transform.LowerBound as its code has it: label >= lowerBound stays)
inline std::unique_ptr<LabelledGraph> filterLabelledArcs(const LabelledGraph& g, int kind, const std::vector<int64_t>& nodeClass = std::vector<int64_t>(), int64_t lowerBound = 0) {
    bvg_lgraph* l = nullptr;
    const int st = bvg_lgraph_filter(g.handle(), kind, nodeClass.empty() ? nullptr : nodeClass.data(), (int64_t)nodeClass.size(), lowerBound, &l);
    return finishLabelled(st, l, "filterLabelledArcs");
}

}  // namespace webgraph
