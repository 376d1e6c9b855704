/*
 * bvgraph_hip.h — C ABI of libbvgraph_hip.so: the MI355X (gfx950) BVGraph successor-list decoder.
 *
 * This is the drop-in boundary for ONE path of vigna/webgraph-big (reference paths relative to
 * /root/reference, BVG = src/it/unimi/dsi/big/webgraph/BVGraph.java, IG = .../ImmutableGraph.java):
 * the BVGraph decode half behind nodeIterator()/successors()/outdegree().  A JNI (or ctypes / C++)
 * shim binds exactly these entry points; INTEGRATION.md shows the Java side.
 *
 * Conventions: every function returns 0 or a negative bvg_status; no exceptions / longjmp cross the
 * boundary; all output buffers are caller-allocated host memory unless the name ends in _dev;
 * functions on ONE handle are not re-entrant, different handles (incl. bvg_copy() flyweights) are
 * (IG:187-197 threading contract).  There is no CPU fallback: without a gfx950 device every compute
 * entry point fails with BVG_E_HIP.
 */
#ifndef BVGRAPH_HIP_H
#define BVGRAPH_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVG_ABI_VERSION 4

/* Status codes; each maps 1:1 to the exception class the reference throws at the cited line. */
typedef enum bvg_status {
    BVG_OK = 0,
    BVG_E_ARG = -1,          /* IllegalArgumentException   BVG:823,863,1000,1128 (node out of range) */
    BVG_E_STATE = -2,        /* IllegalStateException      BVG:701 (ref > window), BVG:832,1136 (no offsets) */
    BVG_E_UNSUPPORTED = -3,  /* UnsupportedOperationException BVG:631,658,699,733,763,794,864 */
    BVG_E_IO = -4,           /* IOException                BVG:1492-1497,1326 (class / version / flag / file) */
    BVG_E_EOF = -5,          /* EOFException from the bit stream (record runs past the end of .graph) */
    BVG_E_NOMEM = -6,        /* OutOfMemoryError (host or device) */
    BVG_E_HIP = -7,          /* no gfx950 device / HIP runtime failure (no CPU fallback exists) */
    BVG_E_CAPACITY = -8      /* caller's successor buffer too small; *n_succ holds the size needed */
} bvg_status;

/* Coding ids, CompressionFlags.java:26-44. */
enum { BVG_DELTA = 1, BVG_GAMMA = 2, BVG_GOLOMB = 3, BVG_SKEWED_GOLOMB = 4, BVG_UNARY = 5, BVG_ZETA = 6, BVG_NIBBLE = 7 };

/* load_mode of bvg_open, = offsetType of BVG:1479 (loadInternal). */
enum { BVG_LOAD_OFFLINE = -1, BVG_LOAD_SEQUENTIAL = 0, BVG_LOAD_STANDARD = 1, BVG_LOAD_MAPPED = 2 };

/* The keys of basename.properties that drive decoding (BVG:1495-1503) + the six coding selectors
 * (setFlags, BVG:1281-1289; defaults BVG:527-542). */
typedef struct bvg_params {
    int64_t nodes;
    int64_t arcs;                 /* -1 if the properties do not say */
    int32_t window_size;          /* default 7  (BVG:455) */
    int32_t max_ref_count;        /* default 3  (BVG:461) */
    int32_t min_interval_length;  /* default 4  (BVG:467); 0 = NO_INTERVALS (BVG:379) */
    int32_t zeta_k;               /* default 3  (BVG:473) */
    int32_t outdegree_coding;     /* GAMMA | DELTA */
    int32_t block_coding;         /* GAMMA | DELTA | UNARY (the decoder's switch, BVG:759-764) */
    int32_t residual_coding;      /* ZETA | GAMMA | DELTA | GOLOMB | NIBBLE */
    int32_t reference_coding;     /* UNARY | GAMMA | DELTA */
    int32_t block_count_coding;   /* GAMMA | DELTA | UNARY */
    int32_t offset_coding;        /* GAMMA | DELTA */
} bvg_params;

/* Result of a fused on-chip scan (the SpeedTest loop, test/SpeedTest.java:127-141, plus a checksum). */
typedef struct bvg_scan_result {
    uint64_t nodes;        /* nodes scanned */
    uint64_t arcs;         /* sum of outdegrees */
    uint64_t chk;          /* sum over arcs (x,y) of bvg_arc_mix(x + node_base, y + node_base) mod 2^64 */
    uint64_t graph_bytes;  /* ALGORITHMIC bytes: compressed .graph bytes covering the scanned node range */
    uint64_t index_bytes;  /* device index bytes the kernels read on top (offsets + block plan + residual skip entries) */
    double kernel_ms;      /* hipEvent time of the scan kernel(s) on the handle's stream */
    uint32_t launches;     /* kernel launches issued (1 + slow-path relaunches) */
    uint32_t slow_blocks;  /* node blocks that had to take the global-memory slow path */
    uint64_t index_entries; /* residual skip entries of the scanned blocks that an index was present for (0 = the scan ran index-less) */
    uint32_t lean_blocks;  /* node blocks launched on the lean scan kernel (validated blocks of an indexed scan; bvg_scan.hip) */
    uint32_t reserved0;
} bvg_scan_result;

typedef struct bvg_graph bvg_graph;

/* ---- load (replaces ImmutableGraph.load -> BVGraph.loadInternal, IG:674-713, BVG:1479-1574) ---- */

void bvg_default_params(bvg_params* p);
/* Parses the text of a .properties file (BVG:1479-1503; class check BVG:1491, version BVG:1496). */
int bvg_parse_properties(const char* text, size_t len, bvg_params* out);
/* Decodes the n+1 gamma/delta coded offset gaps of basename.offsets (readOffset BVG:627-633,
 * OffsetsLongIterator BVG:870-898) into out[0..nodes]. Host-side, one-off at load (the reference
 * builds an Elias-Fano list here, BVG:1556-1558). */
int bvg_decode_offsets(const uint8_t* obytes, size_t nbytes, int64_t nodes, int coding, uint64_t* out);

/* BVGraph.load / loadMapped / loadOffline / loadSequential(basename) (BVG:1345-1464).  Reads
 * basename.properties/.graph[/.offsets], uploads to `device`.  BVG_LOAD_SEQUENTIAL / _OFFLINE need
 * no .offsets file: the index is then derived on the device (BVGraph -O / writeOffsets, BVG:2595-2609) by chunk-parallel speculative
 * walks iterated to the one consistent walk -- measured 0.4-10 s per GiB of stream on 0.25 GiB inputs, the fixed part being the
 * regions that settle one 4 KiB chunk per round (profiles/r03_derive_bench.txt); windows > 127 and streams the parallel walk finds
 * odd take one sequential pass of a single wavefront (~360 s per GiB).  A stream that cannot be derived is refused with the status the
 * reference's sequential iterator would end with: BVG_E_STATE for a reference above the window (BVG:701), BVG_E_EOF for a stream that
 * runs out or whose counts contradict each other.  A reference before node 0 is derived as the reference does it (an empty list there:
 * BVG:1018, 1030). */
int bvg_open(const char* basename, int load_mode, int device, bvg_graph** out);
/* Same from host memory.  offsets: nodes+1 bit positions or NULL (derive on device). */
int bvg_open_mem(const bvg_params* p, const uint8_t* graph, uint64_t nbytes, const uint64_t* offsets, int device, bvg_graph** out);
/* Same from DEVICE memory already resident in HBM.  d_graph is adopted, not copied: it must stay
 * alive until bvg_close and be readable up to nbytes rounded up to 16 + 16 bytes.  d_offsets
 * (nodes+1 uint64) is read once: the library keeps its own packed index (4 bytes per node + 8 per
 * 1024 nodes, the counterpart of the Elias-Fano list of BVG:1545-1558) and the caller may free the
 * array when the call returns -- except when 1024 consecutive records span 2^32 bits or more (or
 * BVG_WIDE_OFFSETS=1 is set): then the plain array is used in place and must stay alive. */
int bvg_open_dev(const bvg_params* p, const void* d_graph, uint64_t nbytes, const void* d_offsets, int device, bvg_graph** out);
/* BVGraph.copy() (BVG:553-578): flyweight sharing the immutable device data, with its own stream
 * and workspace, usable from another thread. */
int bvg_copy(const bvg_graph* g, bvg_graph** out);
void bvg_close(bvg_graph* g);

int bvg_info(const bvg_graph* g, bvg_params* out);           /* numNodes/numArcs/windowSize/... */
/* The handle may stand for nodes [node_base, node_base + nodes) of a larger graph (a shard made by
 * ImmutableGraph.splitNodeIterators, IG:405-436): node ids and successors reported by scan /
 * decode are shifted by node_base.  Default 0. */
int bvg_set_node_base(bvg_graph* g, uint64_t node_base);
/* Copies the device offsets index back (nodes+1 entries): BVGraph -O / writeOffsets (BVG:2595-2609). */
int bvg_get_offsets(bvg_graph* g, uint64_t* out);

/* ---- decode (replaces BVG:821-867 outdegree/successors and BVG:1100-1245 BVGraphNodeIterator) ---- */

/* outdegree(x) for x in [from,to) (BVG:821-842). */
int bvg_outdegrees(bvg_graph* g, int64_t from, int64_t to, int32_t* out);
/* Materialises successors of nodes [from,to): outdeg[to-from] and the concatenated, strictly
 * increasing successor lists in succ (bit-exact with nodeIterator(from)...successorBigArray()).
 * to == from+1 is successors(x) (BVG:860-867).  If succ_cap is too small returns BVG_E_CAPACITY
 * with *n_succ = required size (succ may be NULL to query).  outdeg may be NULL. */
int bvg_decode_range(bvg_graph* g, int64_t from, int64_t to, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ);
/* Same with the successors as 32-bit ids: graphs whose ids + node base stay BELOW 2^32 - 1 (nodes + node_base <= 0xFFFFFFFF; otherwise
 * BVG_E_UNSUPPORTED), host buffers only.  Half the bytes over PCIe, which bounds this path; the caller widens
 * (NodeIterator.successorBigArray() hands out longs, NodeIterator.java:80-96).  A missing successor of a malformed stream (-1 above) reads
 * 0xFFFFFFFF -- never a legal id here, which is why the limit is one below 2^32 -- and the widening caller maps it back to -1. */
int bvg_decode_range32(bvg_graph* g, int64_t from, int64_t to, int32_t* outdeg, uint32_t* succ, uint64_t succ_cap, uint64_t* n_succ);
/* Same, successor / outdegree buffers in device memory (stay in HBM for a downstream kernel). */
int bvg_decode_range_dev(bvg_graph* g, int64_t from, int64_t to, void* d_outdeg, void* d_succ, uint64_t succ_cap, uint64_t* n_succ);
/* Page-locked host memory for the buffers handed to bvg_decode_range / bvg_successors_batch: device -> host copies into it run
 * at the PCIe rate and need no staging (a JNI caller wraps it in a direct ByteBuffer, NewDirectByteBuffer).  Plain malloc'ed /
 * Java-heap buffers work too, only slower.  The iterator's buffer of NodeIterator.successorBigArray() (NodeIterator.java:80-96)
 * is the intended use: one pair of buffers per iterator, reused batch after batch. */
void* bvg_host_alloc(size_t bytes);
void bvg_host_free(void* p);
/* successors(x) for a whole frontier at once (BVG:860-867 per element; the access pattern of
 * algo/ParallelBreadthFirstVisit.java -- bvg_bfs_visit below runs it without leaving the device -- and algo/HyperBall.java:774-822): nodes[count] in any order, repeats
 * allowed; outdeg[count] and the successor lists concatenated in request order.  Each request is
 * decoded together with the few earlier nodes its reference chain reaches (the recursion of BVG:1084). */
int bvg_successors_batch(bvg_graph* g, const int64_t* nodes, int64_t count, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ);
/* Full sequential successor scan of [from,to) consumed on-chip (arc count + checksum).
 * The first scan of >= 4096 nodes also builds the residual skip index of the node blocks it covers (a header walk that counts the
 * entries, a dense walk that fills them, and a validating decode that uses and checks them -- and reports this very scan's result, so
 * the first scan IS the build; a shard of a multi-GPU scan therefore indexes its own part only, a later scan of other nodes indexes the
 * whole graph); a materialising call (bvg_decode_range) builds it for the whole graph once it covers >= 1/4 of the nodes.  The index is shared by bvg_copy()
 * flyweights: 6 bytes (10 for graphs on the 64-bit successor kernels: more than 2^32 - 256 nodes) per 16 residuals of lists
 * with >= 16 residuals -- per 8 of lists with >= 8 on graphs with references below 40 arcs per node; the granularity is chosen when
 * the index is built and travels with it -- (cf. the offset cache the reference builds at load, BVG:1545-1558).  The same passes VALIDATE the
 * blocks: the lean scan kernel then skips the checks a well-formed stream cannot fail, blocks that failed one stay on the
 * checking kernels for good. */
int bvg_scan(bvg_graph* g, int64_t from, int64_t to, bvg_scan_result* out);
/* Builds that index for the blocks of [from,to) now (0, nodes = the whole graph) instead of inside the first scan; a no-op when
 * they are covered already.  entries / bytes (either may be NULL) report what the index of the graph holds afterwards. */
int bvg_build_index(bvg_graph* g, int64_t from, int64_t to, uint64_t* entries, uint64_t* bytes);
/* The device index on disk: the block plan and the residual skip index (with its validation marks) as they stand, written to `path` and
 * loaded back by a later process instead of rebuilt (cf. the reference's cached offsets big list, basename.obl, BVG:1545-1555).
 * bvg_open() loads basename.bvgidx by itself when it exists and is not older than basename.graph; a file that does not belong to
 * the graph (format 2: size, every parameter that shapes a record, block size, a hash of EVERY byte of the stream computed on the device) or is damaged (a
 * checksum over its payload; range checks on every array) is refused with BVG_E_IO and the index is built as usual: the lean kernels trust the marks. */
int bvg_save_index(bvg_graph* g, const char* path);
int bvg_load_index(bvg_graph* g, const char* path);
/* Node-range split points for k shards of ~equal compressed size (the balanced variant of
 * IG:405-436; cf. algo/HyperBall.java:748-768): bounds[0..k], bounds[0]=0, bounds[k]=nodes. */
int bvg_split_by_bits(bvg_graph* g, int k, int64_t* bounds);
/* The same with ~equal ARC counts per shard: bounds[j] = first node whose cumulative outdegree reaches j * arcs / k (the
 * skipTo() walk over algo/EliasFanoCumulativeOutdegreeList.java:30-75 that algo/HyperBall.java:748-768 uses for its tasks);
 * outdegrees and their prefix sum are computed on the device. */
int bvg_split_by_arcs(bvg_graph* g, int k, int64_t* bounds);

/* ---- node-range shards over several GPUs (ImmutableGraph.splitNodeIterators, IG:405-436; arc-balanced tasks as in
 * algo/HyperBall.java:748-768).  Shards are independent: each decodes its own node range (and re-derives its halo locally), the
 * only thing ever combined is {nodes, arcs, chk}, by a plain sum. ---- */
enum { BVG_BALANCE_NODES = 0,   /* ceil(n/k) nodes per shard: the reference's rule, IG:415-433 */
       BVG_BALANCE_BITS = 1,    /* ~equal compressed bits (bvg_split_by_bits) */
       BVG_BALANCE_ARCS = 2 };  /* ~equal arc counts (bvg_split_by_arcs) */
/* bounds[0..k] of the k-way split; cached in the graph, so flyweights and later calls agree. */
int bvg_shard_bounds(bvg_graph* g, int k, int balance, int64_t* bounds);
/* The scan of shard r of k: nodes [bounds[r], bounds[r+1]) (returned in *from / *to when not NULL).  One rank of a
 * one-process-per-GPU job calls this on its replica and all-reduces {arcs, chk} (RCCL: 16 bytes); the sum over r = 0..k-1
 * equals bvg_scan(g, 0, nodes). */
int bvg_scan_shard(bvg_graph* g, int k, int r, int balance, bvg_scan_result* out, int64_t* from, int64_t* to);
/* One process, ngpu devices (a JVM host): per_gpu[i] = a handle of the SAME graph on device i (or bvg_copy() flyweights on
 * one device); shard i runs on per_gpu[i], all shards concurrently, results summed on the host (total; per_shard[ngpu]
 * optional).  total->kernel_ms = the slowest shard. */
int bvg_scan_multi(bvg_graph* const* per_gpu, int ngpu, int balance, bvg_scan_result* total, bvg_scan_result* per_shard);

/* ---- transposition feed (the decode + sort of Transform.transposeOffline, Transform.java:1058-1160; processBatch :938) ----
 * Decodes every arc (x,y) of the graph on the device, sorts the pairs by target (stable radix sort, so sources stay increasing)
 * and returns the TRANSPOSE in CSR form: toffsets[nodes+1] = exclusive prefix of the in-degrees, tsucc[arcs] = for each node y
 * the sources of its incoming arcs in increasing order (what ArcListASCIIGraph / BVGraph.store of the transpose would list).
 * tsucc may be NULL to query *n_arcs (returns BVG_E_CAPACITY).  Requires node_base == 0.  _dev: both buffers in device memory. */
int bvg_transpose(bvg_graph* g, uint64_t* toffsets, int64_t* tsucc, uint64_t tsucc_cap, uint64_t* n_arcs);
int bvg_transpose_dev(bvg_graph* g, void* d_toffsets, void* d_tsucc, uint64_t tsucc_cap, uint64_t* n_arcs);

/* Transform.symmetrizeOffline (Transform.java:546-575) = union(g, transposeOffline(g)): the SYMMETRISED graph in CSR form —
 * soffsets[nodes+1], ssucc = for each node the increasing union of its successors and its predecessors (an arc present in both
 * directions once; loops kept).  *n_arcs = arcs of the result, known only after the transposition: a call with too small a
 * buffer (or ssucc NULL) returns BVG_E_CAPACITY with soffsets and *n_arcs filled and costs the full pass; 2 x numArcs() always
 * suffices.  Requires node_base == 0. */
int bvg_symmetrize(bvg_graph* g, uint64_t* soffsets, int64_t* ssucc, uint64_t ssucc_cap, uint64_t* n_arcs);
int bvg_symmetrize_dev(bvg_graph* g, void* d_soffsets, void* d_ssucc, uint64_t ssucc_cap, uint64_t* n_arcs);

/* ---- weakly connected components (algo/ConnectedComponents.java) ----
 * comp[nodes]: the weak component of every node, numbered as ConnectedComponents.compute numbers them on a symmetric graph
 * (ParallelBreadthFirstVisit.visitAll, ParallelBreadthFirstVisit.java:272-337): component c is the one whose smallest node is the
 * c-th smallest among the components' smallest nodes.  Arcs are taken in both directions, so a directed graph gives its weak
 * components (= compute(new UnionImmutableGraph(g, gT)), the reference's `main -t`) without a transpose.  A concurrent union-find over
 * one parent element per node (4 bytes; 8 on the 64-bit kernels) consumes the decode one arc-bounded batch at a time: the graph never
 * has to fit in HBM as a CSR.  sizes (may be NULL) = computeSizes(): sizes[c] = nodes of component c; *n_components = their number.
 * sizes_cap below the count: BVG_E_CAPACITY, *n_components and comp written all the same.  Requires node_base == 0.  Malformed
 * streams report the decode's status (a successor outside [0, nodes): BVG_E_EOF).  _dev: comp / sizes in device memory (int64). */
#define BVG_CC_SORT_BY_SIZE 1u   /* ConnectedComponents.sortBySize: components renumbered by decreasing size, ties by smallest node */
int bvg_components(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap, uint64_t* n_components);
int bvg_components_dev(bvg_graph* g, uint32_t flags, void* d_comp, void* d_sizes, uint64_t sizes_cap, uint64_t* n_components);

/* ---- strongly connected components (algo/StronglyConnectedComponents.java) ----
 * comp[nodes]: the strongly connected component of every node.  The partition, *n_components, the sizes and the buckets are the
 * reference's; THE NUMBERING IS NOT: the reference numbers a component when Tarjan's visit emits it, here component c is the one whose
 * smallest node is the c-th smallest among the components' smallest nodes (the numbering of the weak components above), and with
 * BVG_SCC_SORT_BY_SIZE (sortBySize) components go by decreasing size, ties by smallest node.  sizes (may be NULL) = computeSizes().
 * BVG_SCC_BUCKETS (computeBuckets): buckets (required then: one byte per node, 0 / 1) marks the nodes whose component has at least one arc
 * and no arc leaving it -- a lone node with only a self-loop is a bucket, a node without successors is not.
 * The computation sweeps the compressed graph over forward arcs only (trimming, one forward-backward step from the live node of largest
 * outdegree, then colouring rounds: DESIGN.md 7e): no transpose, and the graph never has to fit in HBM as a CSR.  Device memory: two
 * elements (4 bytes each; 8 on the 64-bit kernels) and one byte per node, one arc-bounded batch of the decode (as the weak components),
 * 12 bytes per node while numbering; BVG_E_NOMEM leaves g usable.  The cost is one sweep per step of the longest propagation: a chain of k
 * nodes costs about k / 2 sweeps.  counters (may be NULL): out[BVG_SCC_COUNTERS] = sweeps, batch decodes, trim passes, nodes retired by
 * trimming, size of the forward-backward component, colouring rounds, components found by colouring, 1 if a single resident batch was used.
 * g, n_components NULL, unknown flag bits, BVG_SCC_BUCKETS without buckets, node_base != 0: BVG_E_ARG, checked before any device call.  sizes_cap
 * below the count: BVG_E_CAPACITY, *n_components and comp written all the same.  An empty graph has 0 components.  Malformed streams report
 * the decode's status (a successor outside [0, nodes): BVG_E_EOF, never used as an index).  _dev: comp / sizes (int64) and buckets (bytes)
 * in device memory. */
#define BVG_SCC_SORT_BY_SIZE 1u
#define BVG_SCC_BUCKETS      2u
#define BVG_SCC_COUNTERS     8
int bvg_scc(bvg_graph* g, uint32_t flags, int64_t* comp, int64_t* sizes, uint64_t sizes_cap,
            uint64_t* n_components, uint8_t* buckets, uint64_t* counters);
int bvg_scc_dev(bvg_graph* g, uint32_t flags, void* d_comp, void* d_sizes, uint64_t sizes_cap,
                uint64_t* n_components, void* d_buckets, uint64_t* counters);

/* ---- exact geometric centralities (algo/LinearGeometricCentrality.java) ----
 * centrality[s - from] = sum over the nodes y reachable from s of coeff(d(s, y)), s itself included with coeff(0), and reachable[s - from] =
 * the number of those nodes (s included), for the sources s in [from, to): what the reference computes with one breadth-first visit per
 * source.  Here 64 W consecutive sources (W = 1, 2, 4 or 8 64-bit words per node) advance together, one bit each, and ONE sweep of the
 * compressed graph moves all of them by one level.  coeff by `kind`:
 *   BVG_GEO_HARMONIC     d == 0 ? 0 : 1 / d                     (HarmonicCoefficients)
 *   BVG_GEO_POWER_LAW    pow(d, param)                          (PowerLawCoefficients; param < 0: coeff(0) = +inf and so is every value)
 *   BVG_GEO_EXPONENTIAL  pow(param, d)                          (ExponentialCoefficients)
 *   BVG_GEO_TABLE        table[d] for d < table_len, 0 beyond   (any finite-support centrality; the visits still run to their end)
 * THE ROUNDING IS NOT THE REFERENCE'S: it adds coeff to a float once per discovered node (one float rounding per reached node); here
 * coeff(d) times the number of nodes at distance d is summed over d in double and rounded to float once -- the reference's value up to
 * that accumulated float error, and closer to the exact sum.
 * centrality (float) and reachable (int64) hold to - from elements; either may be NULL.  hist (may be NULL): hist[d] = the number of
 * (source, node) pairs at distance d (hist[0] = to - from), *hist_len (required with hist) = distances present; hist_cap below that:
 * BVG_E_CAPACITY, *hist_len and the other outputs written all the same.  counters (may be NULL): out[BVG_GEO_COUNTERS] = passes, sweeps,
 * batch decodes, words per node, levels of the deepest pass, levels skipped without atomics (0: not built), 1 if a single resident batch
 * was used, reserved.  Device memory: 24 W bytes per node, one arc-bounded batch of the decode, O(64 W) accumulators; BVG_E_NOMEM leaves g
 * usable.  g NULL, unknown kind, BVG_GEO_TABLE without a table or with table_len 0, from > to or a range outside [0, nodes], hist without
 * hist_len, node_base != 0: BVG_E_ARG, checked before any device call.  An empty range succeeds and writes nothing.  Malformed streams
 * report the decode's status (a successor outside [0, nodes): BVG_E_EOF, never used as an index).  _dev: centrality / reachable in device
 * memory, hist and counters on the host. */
enum { BVG_GEO_HARMONIC = 0, BVG_GEO_POWER_LAW = 1, BVG_GEO_EXPONENTIAL = 2, BVG_GEO_TABLE = 3 };
#define BVG_GEO_COUNTERS 8
int bvg_geometric(bvg_graph* g, int kind, double param, const double* table, uint64_t table_len, int64_t from, int64_t to,
                  float* centrality, int64_t* reachable, uint64_t* hist, uint64_t hist_cap, uint64_t* hist_len, uint64_t* counters);
int bvg_geometric_dev(bvg_graph* g, int kind, double param, const double* table, uint64_t table_len, int64_t from, int64_t to,
                      void* d_centrality, void* d_reachable, uint64_t* hist, uint64_t hist_cap, uint64_t* hist_len, uint64_t* counters);

/* ---- graph statistics (Stats.java) ----
 * One pass over all successor lists, as Stats.run: arcs, loops, dangling nodes (outdegree 0), terminal nodes (outdegree 0, or one arc that
 * is a loop), the outdegree and indegree extremes with their nodes, num_gaps / tot_gap (per list of d > 1 arcs: d gaps, (last - first) +
 * int2nat(first - x)), tot_loc (sum of |y - x| over the arcs) and log_delta[b] = the arcs (x, y), y != x, with msb(|y - x|) == b.  tot_gap
 * and tot_loc are 128-bit values in two words each.  Ties are the reference's: the smallest node among those of min / max outdegree, the
 * largest node among those of min / max indegree.  Every integer is exact.  An empty graph gives 0 everywhere except min_outdegree =
 * min_indegree = INT64_MAX, and distributions of length 1 holding 0.
 * bvg_stats_compute runs the whole pass and returns an object that holds the summary, both distributions (host memory) and, with
 * BVG_STATS_KEEP_INDEGREES, the indegree of every node on the device (without it that array is freed once its distribution exists).
 * Device memory: 4 bytes per node (8 on the 64-bit path) for the indegrees, 4 per node more while the outdegrees are counted, one
 * arc-bounded batch of the decode (as bvg_components), and 8 bytes per entry of a distribution; BVG_E_NOMEM leaves g usable.  An outdegree
 * or indegree above 2^31 - 1: BVG_E_UNSUPPORTED (the reference throws).  Malformed streams report the decode's status (a successor
 * outside [0, nodes): BVG_E_EOF, never used as an index).  g or out NULL, unknown flag bits, node_base != 0: BVG_E_ARG, checked before
 * any device call.  *out is set to NULL before the pass and stays NULL on every failure of it (BVG_E_EOF, BVG_E_NOMEM, ...): there is
 * nothing to close then.  The object does not refer to g afterwards.
 * bvg_stats_distribution: which = BVG_STATS_OUT / BVG_STATS_IN; *len = the largest degree + 1, always written; out[d] = the nodes of
 * degree d; cap below *len: BVG_E_CAPACITY and out untouched.  bvg_stats_indegrees: the indegrees of [from, to) as int64 (BVG_E_ARG for a
 * range outside [0, nodes], BVG_E_UNSUPPORTED without BVG_STATS_KEEP_INDEGREES); _dev: into device memory. */
typedef struct bvg_stats bvg_stats;
typedef struct bvg_stats_summary {          /* 82 x 8 = 656 bytes */
    uint64_t nodes, arcs, loops, dangling, terminal, num_gaps;
    uint64_t tot_gap_lo, tot_gap_hi, tot_loc_lo, tot_loc_hi;
    int64_t  min_outdegree, max_outdegree, min_outdegree_node, max_outdegree_node;
    int64_t  min_indegree,  max_indegree,  min_indegree_node,  max_indegree_node;
    uint64_t log_delta[64];
} bvg_stats_summary;
#define BVG_STATS_KEEP_INDEGREES 1u
#define BVG_STATS_OUT 0
#define BVG_STATS_IN  1
int  bvg_stats_compute(bvg_graph* g, uint32_t flags, bvg_stats** out);
void bvg_stats_close(bvg_stats* s);
int  bvg_stats_get(const bvg_stats* s, bvg_stats_summary* out);
int  bvg_stats_distribution(const bvg_stats* s, int which, uint64_t* out, uint64_t cap, uint64_t* len);
int  bvg_stats_indegrees(bvg_stats* s, int64_t from, int64_t to, int64_t* out);
int  bvg_stats_indegrees_dev(bvg_stats* s, int64_t from, int64_t to, void* d_out);

/* ---- breadth-first visits (algo/ParallelBreadthFirstVisit.java) ----
 * A visit object keeps on the device what the reference's class keeps (ParallelBreadthFirstVisit.java:79-148): marker[nodes] (-1 = not
 * enqueued yet; otherwise the round in which the node was reached, or its parent with BVG_BFS_PARENT), the round counter (-1 before the
 * first visit), the queue of the last visit and its cut points -- level d is queue[cut[d] .. cut[d + 1]), the last cut point is the queue
 * size, maxDistance() = n_cutpoints - 2, nodeAtMaxDistance() = the last queue element -- plus dist[nodes] (int32): the level of every node
 * of the queue, -1 for every other node.  It holds a bvg_copy() flyweight of g (own stream and workspaces), so g stays usable from
 * another thread and may be closed first.  Requires node_base == 0 (BVG_E_ARG).  One object is not re-entrant.
 * DETERMINISM, where the reference depends on thread timing (:183, :188-190): inside each level the queue holds the nodes in INCREASING
 * ID; with BVG_BFS_PARENT the parent of a node is the SMALLEST node of the previous level that has it as a successor, the root's parent
 * is itself.
 * bvg_bfs_clear: every marker and the round back to -1 (:141-147); the queue, the cut points and dist are forgotten too.
 * bvg_bfs_visit: visit(start) (:222-266).  A start that is marked already: *visited = 0 and nothing changes, not even the queue.  Otherwise
 * the round is incremented, queue and cut points are replaced, *visited = the queue size.  Start outside [0, nodes): BVG_E_ARG.
 * bvg_bfs_visit_all: visitAll() (:272-339): clear, then one visit per node that is still unmarked, in increasing node order, each with its
 * own round.  As in the reference (:309-317) a node with no successors, or whose only successor is itself, gets its marker and its round
 * but does not replace queue and cut points: afterwards they (and dist) are those of the last visit that had something to expand.  On a
 * symmetric graph the round markers are the component numbers of bvg_components.
 * bvg_bfs_get / _get_dev (device buffers): any pointer may be NULL; marker, queue (int64) and cutpoints (uint64) as sized by bvg_bfs_info,
 * dist int32[nodes]; a capacity below the size is BVG_E_CAPACITY and nothing is written.
 * Malformed streams report the decode's status (a successor outside [0, nodes): BVG_E_EOF, never used as an index).  After an error the
 * object is in the cleared state.  Each level is expanded by random access to the frontier's lists or, when the frontier is large, by a
 * sequential decode of the whole graph in arc-bounded batches; bvg_bfs_counters reports what ran: out[BVG_BFS_COUNTERS] =
 * levels on the frontier route, levels on the sweep route, requests decoded through the block plan ("deep"), frontier batches, sweep
 * batches, levels whose queue segment was sorted, levels compacted from the node range, route of the last visit's first level (1 / 2). */
#define BVG_BFS_PARENT 1u
#define BVG_BFS_COUNTERS 8
typedef struct bvg_bfs bvg_bfs;
int bvg_bfs_create(bvg_graph* g, uint32_t flags, bvg_bfs** out);
void bvg_bfs_close(bvg_bfs* v);
int bvg_bfs_clear(bvg_bfs* v);
int bvg_bfs_visit(bvg_bfs* v, int64_t start, uint64_t* visited);
int bvg_bfs_visit_all(bvg_bfs* v);
int bvg_bfs_info(const bvg_bfs* v, int64_t* round, uint64_t* queue_size, uint64_t* n_cutpoints);
int bvg_bfs_get(bvg_bfs* v, int64_t* marker, int64_t* queue, uint64_t queue_cap, uint64_t* cutpoints, uint64_t cut_cap, int32_t* dist);
int bvg_bfs_get_dev(bvg_bfs* v, void* d_marker, void* d_queue, uint64_t queue_cap, void* d_cutpoints, uint64_t cut_cap, void* d_dist);
int bvg_bfs_counters(const bvg_bfs* v, uint64_t* out);

/* ---- HyperBall (algo/HyperBall.java; non-systolic iterations, counters in device memory) ----
 * One HyperLogLog counter of m = 2^log2m registers per node, log2m in [4, 12] (below: BVG_E_ARG, above: BVG_E_UNSUPPORTED).  An iteration
 * makes every counter the register-wise maximum of itself and of the counters of the node's successors that the previous iteration
 * modified (self-loops skipped), counts it, and adds the count to a new term of the neighbourhood function (HyperBall.java:777-919 with
 * systolic == local == external == false, :1000-1182); with BVG_HB_SUM_OF_DISTANCES / BVG_HB_HARMONIC a node whose counter changed by
 * delta = count after - count before > 0 in iteration k (from 0) adds (float)(delta (k + 1)) / (float)(delta / (k + 1)) to its float32
 * sum of distances / sum of inverse distances.  After the pass the term is raised to the previous one if it is smaller (:1165).
 * THE HASH IS THIS LIBRARY'S (the reference takes its counters from a library outside its tree): register contents are not those of
 * the Java implementation, the algorithm and the estimator are.  Node v under `seed` goes to
 *     x = mix64(v + (seed + 1) * 0x9E3779B97F4A7C15)      mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     j = x & (m - 1)                                                z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *     r = ctz((x >> log2m) | 1 << (64 - log2m)) + 1
 *     reg[j] = max(reg[j], r)                             (all arithmetic modulo 2^64; r <= 65 - log2m: one byte per register)
 * count = alpha m^2 / sum_j 2^-reg[j], alpha = 0.673, 0.697, 0.709 for m = 16, 32, 64 and 0.7213 / (1 + 1.079 / m) above; when some register
 * is 0 and the count is below 2.5 m it is m ln(m / zeroes) instead.  The sum is exact before its one rounding, so counts do not depend
 * on the order of anything; the terms of the neighbourhood function are added in a fixed order (no floating-point atomics).
 * The object holds a bvg_copy() flyweight of g (own stream and workspaces): g stays usable and may be closed first.  Requires
 * node_base == 0 (BVG_E_ARG).  Device memory: 2 nodes m bytes of counters (one byte per register), nodes / 4 of modified bits, 4 nodes
 * per centrality array, and one arc-bounded batch of the decode (as bvg_components); BVG_E_NOMEM leaves g usable.
 * bvg_hyperball_create: allocates; nothing is initialised yet.  bvg_hyperball_init: init(seed) (:580-607) -- node i added to counter i,
 *   neighbourhood function = [nodes], iteration = -1, every counter modified, centralities 0.  bvg_hyperball_iterate: one iteration;
 *   before init: BVG_E_STATE.  bvg_hyperball_run: run(upperBound, threshold) (:1222-1239) with the seed of create or of the last init:
 *   init, then at most min(upper_bound, nodes) iterations (upper_bound < 0: no bound), stopping after one that modified nothing, or, from
 *   the fifth on, after one whose relative increment is below 1 + threshold (-1: never).
 * bvg_hyperball_info: iteration (-1 after init), modified() of the last iteration (nodes after init), the last relative increment, the
 *   length of the neighbourhood function; any pointer may be NULL.  bvg_hyperball_neighbourhood_function: out[cap >= length].
 * bvg_hyperball_registers: counters [from, to) as (to - from) m bytes, register j of counter x at out[(x - from) m + j].
 * bvg_hyperball_counts / _dev (device buffer): the counts of counters [from, to) (double).
 * bvg_hyperball_centrality / _dev: float[nodes] by the formulas of HyperBall.main (:1349-1388) -- the sum of distances d; the harmonic
 *   centrality (sum of inverse distances); closeness d == 0 ? 0 : 1 / d; Lin d == 0 ? 1 : count^2 / d; Nieminen count^2 - d; reachable =
 *   count.  The first, closeness, Lin and Nieminen need BVG_HB_SUM_OF_DISTANCES, harmonic needs BVG_HB_HARMONIC: BVG_E_STATE otherwise.
 * bvg_hyperball_relative_standard_deviation: beta / sqrt(m), beta = 1.106, 1.070, 1.054, 1.046 for log2m 4..7 and 1.04 above.
 * Malformed streams report the decode's status (a successor outside [0, nodes): BVG_E_EOF, never used as an index); after an error of an
 * iteration the object needs bvg_hyperball_init (BVG_E_STATE until then).  NULL or invalid arguments: BVG_E_ARG, no device touched.
 * Not built: systolic / local iterations (they need the transpose as a graph), external counters, discount functions, node weights. */
#define BVG_HB_SUM_OF_DISTANCES 1u
#define BVG_HB_HARMONIC 2u
enum { BVG_HB_WHICH_SUM_OF_DISTANCES = 0, BVG_HB_WHICH_HARMONIC = 1, BVG_HB_WHICH_CLOSENESS = 2, BVG_HB_WHICH_LIN = 3, BVG_HB_WHICH_NIEMINEN = 4, BVG_HB_WHICH_REACHABLE = 5 };
typedef struct bvg_hyperball bvg_hyperball;
int bvg_hyperball_create(bvg_graph* g, int log2m, uint32_t flags, uint64_t seed, bvg_hyperball** out);
void bvg_hyperball_close(bvg_hyperball* h);
int bvg_hyperball_init(bvg_hyperball* h, uint64_t seed);
int bvg_hyperball_iterate(bvg_hyperball* h);
int bvg_hyperball_run(bvg_hyperball* h, int64_t upper_bound, double threshold);
int bvg_hyperball_info(const bvg_hyperball* h, int64_t* iteration, uint64_t* modified, double* relative_increment, uint64_t* nf_len);
int bvg_hyperball_neighbourhood_function(const bvg_hyperball* h, double* out, uint64_t cap);
int bvg_hyperball_registers(bvg_hyperball* h, int64_t from, int64_t to, uint8_t* out);
int bvg_hyperball_counts(bvg_hyperball* h, int64_t from, int64_t to, double* out);
int bvg_hyperball_counts_dev(bvg_hyperball* h, int64_t from, int64_t to, void* d_out);
int bvg_hyperball_centrality(bvg_hyperball* h, int which, float* out);
int bvg_hyperball_centrality_dev(bvg_hyperball* h, int which, void* d_out);
double bvg_hyperball_relative_standard_deviation(int log2m);

/* ---- arc labels stored as a bit stream (labelling/BitStreamArcLabelledImmutableGraph.java) ----
 * basename.labels holds, node after node, the labels of the node's arcs in successor order (:75-84); basename.labeloffsets the
 * gamma-coded bit lengths of those runs after a leading gamma(0) (store(), :655-680).  The node iterator reads `outdegree`
 * labels per node (:565-582).  Built for the scalar label classes: GammaCodedIntLabel (GammaCodedIntLabel.java:60-64) and
 * FixedWidthIntLabel (FixedWidthIntLabel.java:70-73), and for FixedWidthIntListLabel (FixedWidthIntListLabel.java:73-78:
 * gamma length + elements of `width` bits per arc) and FixedWidthLongListLabel (elements of up to 64 bits, below); user label
 * classes return BVG_E_UNSUPPORTED. */
enum { BVG_LABEL_GAMMA_INT = 1, BVG_LABEL_FIXED_INT = 2, BVG_LABEL_FIXED_INT_LIST = 3, BVG_LABEL_FIXED_LONG_LIST = 4 };
typedef struct bvg_labels bvg_labels;
/* Label.toSpec() text, e.g. "it.unimi.dsi.big.webgraph.labelling.FixedWidthIntLabel(FOO,10)" -> kind, width. */
int bvg_labels_parse_spec(const char* spec, int* kind, int* width);
/* label_offsets: nodes+1 bit positions into the label stream (decode basename.labeloffsets with bvg_decode_offsets(.., BVG_GAMMA, ..)).
 * BVG_E_EOF if the last one lies behind the stream, else BVG_E_IO if they are not non-decreasing; no handle is returned then. */
int bvg_labels_open_mem(int kind, int width, int64_t nodes, const uint8_t* stream, uint64_t nbytes, const uint64_t* label_offsets, int device, bvg_labels** out);
/* basename.properties alone (host-only): label class and the basename of the underlying graph (property underlyinggraph,
 * resolved against the property file, :95-97). */
int bvg_labels_read_properties(const char* basename, int* kind, int* width, char* underlying, size_t underlying_cap);
/* BitStreamArcLabelledImmutableGraph.load (:378-484): reads basename.{properties,labels,labeloffsets}; `underlying` receives the
 * basename of the underlying graph (property underlyinggraph, resolved against the property file), to be opened with bvg_open.
 * nodes = numNodes() of that graph. */
int bvg_labels_open(const char* basename, int64_t nodes, int device, bvg_labels** out, char* underlying, size_t underlying_cap);
void bvg_labels_close(bvg_labels* l);
int bvg_labels_info(const bvg_labels* l, int* kind, int* width, int64_t* nodes, uint64_t* stream_bytes);
/* Labels of the arcs of nodes [from,to) in the order bvg_decode_range lists the successors; outdeg[to-from] as returned by it.
 * *n_labels = sum of the outdegrees; BVG_E_CAPACITY if cap is smaller; BVG_E_EOF if a node's run does not end at the next offset
 * (the outdegrees do not belong to this label stream, or the stream is damaged), and if a gamma-coded label is 2^31 or more:
 * GammaCodedIntLabel cannot write such a value, the reference's readGamma() would wrap it to a negative int, and a negative label
 * handed on silently is worse than an error.  `labels` is written only when the call returns 0. */
int bvg_labels_decode_range(bvg_labels* l, int64_t from, int64_t to, const int32_t* outdeg, int32_t* labels, uint64_t cap, uint64_t* n_labels);
/* List labels (kind BVG_LABEL_FIXED_INT_LIST): list_off[arcs+1] = exclusive prefix of the list lengths of the arcs of [from,to) in
 * successor order, values[cap] = the concatenated elements; *n_values = their number.  BVG_E_CAPACITY if cap is smaller (list_off is
 * filled either way: size the buffer from list_off[arcs] and call again).  BVG_E_EOF as for bvg_labels_decode_range; a gamma-coded
 * list LENGTH of 2^31 or more is refused in the same way (readGamma() is an int).  Next to BVG_E_EOF `values` is not written, and
 * list_off counts every list that cannot be read inside its node's run as empty, along with the lists behind it in that node. */
int bvg_labels_decode_range_lists(bvg_labels* l, int64_t from, int64_t to, const int32_t* outdeg, uint64_t* list_off, int32_t* values, uint64_t cap, uint64_t* n_values);
/* The same for FixedWidthLongListLabel (labelling/FixedWidthLongListLabel.java:81-87: gamma(length), then readLong(width), width <= 64):
 * kind BVG_LABEL_FIXED_LONG_LIST, 64-bit elements. */
int bvg_labels_decode_range_lists64(bvg_labels* l, int64_t from, int64_t to, const int32_t* outdeg, uint64_t* list_off, int64_t* values, uint64_t cap, uint64_t* n_values);
/* Same as bvg_labels_decode_range, outdegrees (int32) and labels (int32) in device memory: chains with bvg_decode_range_dev without leaving HBM.
 * Next to BVG_E_CAPACITY nothing is written; next to BVG_E_EOF d_labels[0, *n_labels) holds no labels to be used. */
int bvg_labels_decode_range_dev(bvg_labels* l, int64_t from, int64_t to, const void* d_outdeg, void* d_labels, uint64_t cap, uint64_t* n_labels);

/* ---- the compressor on the device (second half): BVGraph.store (BVG:2329-2470; CompressionThread.call
 * :2216-2327, diffComp :1977-2159, intervalize :1595-1618) from an adjacency in CSR form -- adj_off[nodes+1], adj[adj_off[nodes]] with
 * strictly increasing successor lists -- to the bytes of basename.graph and the nodes+1 bit offsets (write basename.offsets from them
 * with the gamma / delta coded gaps of BVG:2228,2311).  p gives windowsize, maxrefcount (-1 = unbounded), minintervallength, zetak and
 * the codings (nodes / arcs are ignored).  chunk_nodes > 0 compresses ranges of that many nodes with a fresh window each, as the
 * reference's multi-threaded store does (BVG:2404-2457); 0 = one range = the single-threaded store, byte for byte.
 * minintervallength = 1 means runs of two or more consecutive extras, as in the reference (only v[i] + 1 == v[i + 1] opens an interval,
 * BVG:1604): a lone extra is a residual whatever the minimum; 0 disables intervals.  windowsize above 127 is BVG_E_UNSUPPORTED.
 * *graph / *offsets are malloc'ed (bvg_free).  The input is checked on the device before any list is read; BVG_E_ARG, and nothing
 * written, for offsets that do not start at 0 (adj_off[0] != 0: adj_off indexes adj itself, not a slice of a larger array), decrease,
 * pass adj_off[nodes] or span more than 2^31 - 1 successors, and for lists that are not strictly increasing or leave [0, nodes).
 * adj must hold adj_off[nodes] elements (it may be NULL only if that is 0). */
int bvg_store(const bvg_params* p, int64_t nodes, const uint64_t* adj_off, const int64_t* adj, int64_t chunk_nodes, int device,
              uint8_t** graph, uint64_t* graph_bytes, uint64_t** offsets);
void bvg_free(void* p);

/* ---- EFGraph: the quasi-succinct (Elias-Fano) graph format (EFGraph.java, "EF" below) ----
 * basename.properties: graphclass it.unimi.dsi.big.webgraph.EFGraph (it.unimi.dsi.webgraph.EFGraph accepted, EF:683), version <= 0
 * (EF:686-687), nodes, arcs, upperbound (default nodes, EF:690), quantum (a power of two, EF:691-693), byteorder (LITTLE_ENDIAN /
 * BIG_ENDIAN, EF:695-698).  basename.graph: 64-bit words in that byte order; bit p of the stream is bit p & 63 of word p >> 6 (least
 * significant bit first, LongWordOutputBitStream EF:294-414 -- the opposite of BVGraph); close() always writes the current word
 * (EF:408-413), so the file holds bits / 64 + 1 words.  basename.offsets: nodes + 1 delta-coded gaps in an ordinary MSB-first stream,
 * the first being 0 (EF:785, EF:812): bvg_decode_offsets(.., BVG_DELTA, ..) reads it.
 * Record of a node with outdegree d, upper bound U, quantum 2^q; the list gets a terminator equal to U, so L = d + 1 (EF:803, EF:522):
 *   l = max(0, msb(U / L)) (EF:140-142), ps = max(0, ceilLog2(L + (U >> l))) (EF:152-154), P = (U >> l) >> q (EF:165-168)
 *   gamma(d) | P pointers of ps bits | L lower fields of l bits | (U >> l) + d + 1 upper bits
 *   gamma(x) (EF:394-406): v = x + 1, m = msb(v): m zero bits, a one bit, the low m bits of v.  Element i (e_d = U): lower field e_i & (2^l - 1),
 *   upper bit (e_i >> l) + i set.  Pointer k (from 1) = k 2^q + #{i : (e_i >> l) < k 2^q}: the position just past the (k 2^q)-th zero (EF:511-513).
 * So a record's length is a closed form of d, element i is (select1(upper, i) - i) << l | lower[i], and nothing is a chain.
 * Conventions are those of the bvg_ entry points above: 0 or a negative bvg_status, caller-allocated host buffers unless the name ends in
 * _dev, one handle not re-entrant, bvg_ef_copy() flyweights for other threads.  Not built: multi-GPU shards, node bases, 32-bit successor
 * output, the analytics on an EFGraph, the cached offsets list (basename.obl, EF:723-735). */
typedef struct bvg_ef_params {          /* 32 bytes */
    int64_t nodes;
    int64_t arcs;                       /* -1 if the properties do not say */
    int64_t upper_bound;                /* >= nodes */
    int32_t log2_quantum;               /* 0..62 */
    int32_t big_endian;                 /* byte order of the words of the FILE: swapped once at load, the device holds little-endian words */
} bvg_ef_params;
typedef struct bvg_efgraph bvg_efgraph;
/* EFGraph.loadInternal's property checks (EF:675-698): BVG_E_IO for another class, a missing or newer version, missing nodes / quantum /
 * byteorder; BVG_E_ARG (IllegalArgumentException) for a quantum that is no power of two, an unknown byte order, upperbound < nodes. */
int bvg_ef_parse_properties(const char* text, size_t len, bvg_ef_params* out);
/* Host only: the nodes + 1 offsets of a bare stream by one walk (gamma, the closed-form length, repeat): what a load without
 * basename.offsets derives.  BVG_E_EOF for a record that runs past the stream, BVG_E_UNSUPPORTED for an outdegree of 2^31 or more. */
int bvg_ef_derive_offsets(const bvg_ef_params* p, const uint8_t* bytes, uint64_t nbytes, uint64_t* out);
/* EFGraph.load / loadMapped / loadOffline / loadSequential (EF:542-673).  BVG_LOAD_SEQUENTIAL / _OFFLINE do not read basename.offsets:
 * the offsets are derived on the host (serial, a few operations per node). */
int bvg_ef_open(const char* basename, int load_mode, int device, bvg_efgraph** out);
/* Same from host memory; bytes in the byte order p says.  offsets: nodes + 1 bit positions, or NULL (derived).  Offsets given by the
 * caller are checked where they are used: every call verifies, for the nodes it touches and before it writes anything, that
 * offsets[x + 1] - offsets[x] is the closed-form length of the record at offsets[x] and that the record ends inside the stream;
 * a mismatch is BVG_E_EOF and nothing is written for that call. */
int bvg_ef_open_mem(const bvg_ef_params* p, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, int device, bvg_efgraph** out);
/* Same from DEVICE memory: little-endian words (nbytes a multiple of 8, p->big_endian 0) adopted, not copied -- they must stay alive
 * until the last handle closes; d_offsets (nodes + 1 uint64) is copied and may be freed when the call returns. */
int bvg_ef_open_dev(const bvg_ef_params* p, const void* d_words, uint64_t nbytes, const void* d_offsets, int device, bvg_efgraph** out);
int bvg_ef_copy(const bvg_efgraph* g, bvg_efgraph** out);      /* EFGraph.copy() (EF:1173-1176) */
void bvg_ef_close(bvg_efgraph* g);
int bvg_ef_info(const bvg_efgraph* g, bvg_ef_params* out);
int bvg_ef_get_offsets(bvg_efgraph* g, uint64_t* out);         /* nodes + 1 entries */
/* outdegree(x) for x in [from, to) (EF:1008-1014). */
int bvg_ef_outdegrees(bvg_efgraph* g, int64_t from, int64_t to, int32_t* out);
/* The successors of nodes [from, to) (EF:1081-1095 per list), with the capacity contract of bvg_decode_range: BVG_E_CAPACITY and
 * *n_succ = the size needed when succ_cap is smaller (succ may be NULL to query); outdeg may be NULL.  A record that fails the length
 * check (above), or whose outdegree is 2^31 or more (BVG_E_UNSUPPORTED), fails the call before anything is written.  An upper-bits
 * region that does not hold exactly d + 1 ones is BVG_E_EOF with the slots of the missing ones written as -1 and every other list of
 * the call intact; no write ever leaves a list's own d slots. */
int bvg_ef_decode_range(bvg_efgraph* g, int64_t from, int64_t to, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ);
int bvg_ef_decode_range_dev(bvg_efgraph* g, int64_t from, int64_t to, void* d_outdeg, void* d_succ, uint64_t succ_cap, uint64_t* n_succ);
/* successors(x) for nodes[count] in any order, repeats allowed; lists concatenated in request order.  A node outside [0, nodes): BVG_E_ARG. */
int bvg_ef_successors_batch(bvg_efgraph* g, const int64_t* nodes, int64_t count, int32_t* outdeg, int64_t* succ, uint64_t succ_cap, uint64_t* n_succ);
/* The scan of [from, to) consumed on chip under the contract of bvg_scan: chk = the sum of bvg_arc_mix over the arcs, one multiply-add
 * per produced successor, so {nodes, arcs, chk} equal bvg_scan of the same graph stored as a BVGraph.  graph_bytes = the bytes of the
 * words covering the range, index_bytes = the offsets read, kernel_ms = from the header kernel to the last decode kernel (one host
 * round trip for the sizes included), launches; every other field is 0. */
int bvg_ef_scan(bvg_efgraph* g, int64_t from, int64_t to, bvg_scan_result* out);
/* LazyLongSkippableIterator.skipTo(bounds[i]) on a FRESH iterator over successors(nodes[i]) (EF:1098-1160): out[i] = the smallest
 * successor >= bounds[i], or -1.  The result is defined on the d real successors only (the reference compares the terminator with
 * nodes, EF:1106, EF:1157, and so hands out a terminator upperbound != nodes as if it were a successor).  When (bound >> l) exceeds the
 * quantum the walk starts at skip pointer (bound >> l) >> q.  A node outside [0, nodes): BVG_E_ARG; a bad record: BVG_E_EOF and out untouched. */
int bvg_ef_skip_to_batch(bvg_efgraph* g, const int64_t* nodes, const int64_t* bounds, int64_t count, int64_t* out);
/* hipEvent time of the kernel of the last bvg_ef_skip_to_batch (or of the last bvg_ef_scan) on this handle: measurements only. */
int bvg_ef_last_kernel_ms(bvg_efgraph* g, double* ms);
/* EFGraph.store (EF:773-820) on the device, from an adjacency in CSR form as bvg_store takes it, with the same checks (BVG_E_ARG, nothing
 * written: offsets that do not start at 0, decrease or span more than 2^31 - 1 successors; lists that are not strictly increasing or
 * leave [0, nodes)) and upper_bound >= nodes, 0 <= log2_quantum <= 62 besides.  *graph = the bytes of basename.graph in the byte order
 * asked for, the trailing word included (*graph_bytes = 8 (bits / 64 + 1)); *offsets = nodes + 1 bit positions (write basename.offsets
 * from their delta-coded gaps).  Both malloc'ed (bvg_free). */
int bvg_ef_store(int64_t nodes, int64_t upper_bound, int log2_quantum, int big_endian, const uint64_t* adj_off, const int64_t* adj, int device,
                 uint8_t** graph, uint64_t* graph_bytes, uint64_t** offsets);

/* ---- text graphs: ASCIIGraph (ASCIIGraph.java, "AG") and arc lists (ArcListASCIIGraph.java, "AL"; ScatteredArcsASCIIGraph.java) ----
 * basename.graph-txt: the node count n on a line of its own, then one line per node holding its successors in increasing order, each
 * followed by one space (AG:259-260).  An arc list: one `source TAB target` line per arc (AL:311).
 * READING, both formats.  Line breaks are "\n", "\r\n" and a lone "\r": a '\r' always breaks a line, a '\n' does unless the byte before
 * it is '\r'.  Every other byte of value 0..32 separates tokens; digits form numbers, with any number of leading zeros, at most 19
 * significant digits and a value of at most 2^63 - 1; every other byte ('-', '.', '/', '#', quotes, letters, bytes >= 128) is refused.
 * DELIBERATE DEVIATIONS: the reference reads numbers through a double ((long)st.nval): it accepts "3.0", loses exactness past 2^53 and
 * treats '/' as a comment -- here integers are read exactly and the rest is refused; Long.parseLong accepts a signed header -- here
 * digits only.
 * An ASCIIGraph: the first line is n, digits and nothing else; the next n lines are the lists; bytes behind line n + 1 are never looked
 * at (the reference never reads them; a header "0" may even lack its line break).  Refused, with *err = {byte offset, 1-based line,
 * reason} of the SMALLEST byte offset at which anything is wrong (at one offset: the smallest reason):
 *   BVG_TEXT_BAD_BYTE        BVG_E_IO   a byte that is no digit, separator or line break; at that byte
 *   BVG_TEXT_BAD_HEADER      BVG_E_IO   a separator inside the header line (at it), or an empty header line (at byte 0)
 *   BVG_TEXT_TOO_LARGE       BVG_E_IO   more than 19 significant digits, or a value above 2^63 - 1; at the first byte of the number
 *   BVG_TEXT_NOT_NODE        BVG_E_IO   a successor >= n (AG:180); at the first byte of the number
 *   BVG_TEXT_NOT_INCREASING  BVG_E_ARG  a successor not above the one before it on its line (the reference does not check, every
 *                                       consumer here demands it); at the first byte of the second number
 *   BVG_TEXT_EOF             BVG_E_IO   fewer than n complete lines behind the header -- a last line without its line break is incomplete,
 *                                       the reference meets EOF inside it; at byte offset nbytes, on the line the text ends in
 * An arc list: every line holds two numbers or none; a line whose first byte is '#' is skipped whole (ScatteredArcsASCIIGraph); `shift` is
 * added to both ends; sources in any order; a duplicate arc appears once; nodes = max(largest id + 1, min_nodes); an empty text gives
 * min_nodes nodes and no arcs.  BVG_TEXT_SYMMETRIZE adds the reverse of every arc, BVG_TEXT_NO_LOOPS drops the arcs x -> x (the two
 * switches of ScatteredArcsASCIIGraph); unknown flag bits: BVG_E_ARG.  Identifiers that are not node numbers: "scattered arc lists" below.  Refused besides
 * BVG_TEXT_BAD_BYTE and BVG_TEXT_TOO_LARGE:
 *   BVG_TEXT_SHIFT_RANGE     BVG_E_ARG  id + shift below 0 or above 2^63 - 1 (AL:157); at the first byte of the number (a shift of -2^63 is
 *                                       BVG_E_ARG for every entry point that takes one, before anything is read)
 *   BVG_TEXT_ARC_FIELDS      BVG_E_IO   a line with one number (at the line break that ends it; at nbytes when none does) or with
 *                                       three or more (at the first byte of the third)
 * Ids of 2^40 or more are BVG_E_NOMEM: adj_off alone would not fit.
 * DEVICE MEMORY.  The text and its CSR must fit on the device together: 1 byte per text byte (none for the _dev forms, which read the
 * caller's buffer), 8 bytes per number and 8 per line break while parsing, and 16 bytes per 4 KiB of text; a text of single-digit
 * successors therefore peaks near 5 bytes per text byte, a text of empty lines at 9.  An arc list takes, while it is sorted, 44 bytes per
 * arc on top (88 with BVG_TEXT_SYMMETRIZE) plus the sort's own workspace.  What stays in the object: 8 (nodes + 1) + 8 arcs (an
 * ASCIIGraph keeps the array of all its numbers: 8 bytes more, and 8 per number behind line n + 1).  BVG_E_NOMEM leaves nothing allocated.
 * *out is NULL after every failure; err may be NULL.  One text of 8 TiB or more, or an arc list of 2^31 pairs or more (2^30 with
 * BVG_TEXT_SYMMETRIZE): BVG_E_UNSUPPORTED.
 * bvg_text_get / _get_dev: adj_off[nodes + 1] and adj[arcs] (sizes from bvg_text_info); either may be NULL; a capacity (in elements) below
 * the size: BVG_E_CAPACITY, nothing written.  bvg_text_store: bvg_store on the resident CSR, no host round trip, the same bytes.
 * WRITING.  bvg_text_format_ascii: for each node of [from, to) every successor in decimal followed by one space, then '\n' -- AG:259-260
 * without the header line, which the file writer puts first.  bvg_text_format_arcs: (s + shift) TAB (t + shift) '\n' per arc (AL:311).  Node
 * ids include the handle's node base.  bvg_text_format_csr: the same for an adjacency in host memory that came from elsewhere (kind =
 * BVG_TEXT_ASCII / BVG_TEXT_ARCS; node x of the array is node first_node + x; adj_off may start anywhere; shift is ignored for
 * BVG_TEXT_ASCII), on the calling thread's current device.  out == NULL or cap below the size: BVG_E_CAPACITY with *nbytes filled -- only
 * the sizing pass is paid for, no text is written.  A negative successor, or an id the shift takes out of [0, 2^63 - 1]: BVG_E_ARG.
 * One call formats fewer than 2^31 successors + nodes: writers go range by range (bvg_split_by_arcs) and append; the output does not
 * depend on the ranges.  Device memory: 12 bytes per successor and per node of the range, the decoded range, and the text. */
typedef struct bvg_text bvg_text;
typedef struct bvg_text_error {             /* 24 bytes */
    uint64_t byte;                          /* offset of the offending byte */
    int64_t  line;                          /* 1-based: 1 + the line breaks before `byte` */
    int32_t  reason;                        /* BVG_TEXT_BAD_BYTE ... */
    int32_t  reserved;
} bvg_text_error;
enum { BVG_TEXT_BAD_BYTE = 1, BVG_TEXT_BAD_HEADER = 2, BVG_TEXT_TOO_LARGE = 3, BVG_TEXT_NOT_NODE = 4, BVG_TEXT_NOT_INCREASING = 5,
       BVG_TEXT_SHIFT_RANGE = 6, BVG_TEXT_ARC_FIELDS = 7, BVG_TEXT_EOF = 8 };
enum { BVG_TEXT_ASCII = 0, BVG_TEXT_ARCS = 1 };
#define BVG_TEXT_SYMMETRIZE 1u
#define BVG_TEXT_NO_LOOPS   2u
int  bvg_text_parse_ascii(const void* text, uint64_t nbytes, int device, bvg_text** out, bvg_text_error* err);
int  bvg_text_parse_ascii_dev(const void* d_text, uint64_t nbytes, int device, bvg_text** out, bvg_text_error* err);
int  bvg_text_parse_arcs(const void* text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err);
int  bvg_text_parse_arcs_dev(const void* d_text, uint64_t nbytes, int64_t shift, uint32_t flags, int64_t min_nodes, int device, bvg_text** out, bvg_text_error* err);
void bvg_text_close(bvg_text* t);
int  bvg_text_info(const bvg_text* t, int64_t* nodes, uint64_t* arcs);
int  bvg_text_get(bvg_text* t, uint64_t* adj_off, uint64_t off_cap, int64_t* adj, uint64_t adj_cap);
int  bvg_text_get_dev(bvg_text* t, void* d_adj_off, uint64_t off_cap, void* d_adj, uint64_t adj_cap);
int  bvg_text_store(bvg_text* t, const bvg_params* p, int64_t chunk_nodes, uint8_t** graph, uint64_t* graph_bytes, uint64_t** offsets);
int  bvg_text_format_ascii(bvg_graph* g, int64_t from, int64_t to, void* out, uint64_t cap, uint64_t* nbytes);
int  bvg_text_format_ascii_dev(bvg_graph* g, int64_t from, int64_t to, void* d_out, uint64_t cap, uint64_t* nbytes);
int  bvg_text_format_arcs(bvg_graph* g, int64_t from, int64_t to, int64_t shift, void* out, uint64_t cap, uint64_t* nbytes);
int  bvg_text_format_arcs_dev(bvg_graph* g, int64_t from, int64_t to, int64_t shift, void* d_out, uint64_t cap, uint64_t* nbytes);
int  bvg_text_format_csr(int kind, int64_t first_node, int64_t nodes, const uint64_t* adj_off, const int64_t* adj, int64_t shift,
                         void* out, uint64_t cap, uint64_t* nbytes);

/* ---- scattered arc lists (ScatteredArcsASCIIGraph.java, "SA"): arc lists whose identifiers are not node numbers ----
 * Every newly seen identifier gets the next node number, offending lines are counted and skipped, and the identifiers in order of
 * appearance stay with the result (ids[node]; basename.ids).  The result is a bvg_text: bvg_text_info / _get / _get_dev / _store / _close
 * and every bvg_transform_* call and bvg_compose take it.
 * LINES end at "\r", "\n" or "\r\n" (the rule of the text graphs above); a last line without a terminator counts.  WHITESPACE is every
 * byte 0..32; a TOKEN is a maximal run of other bytes (bytes >= 0x80 belong to tokens).  A line of whitespace only is skipped; a line
 * whose very first byte is '#' is a comment (" #x 1" is not: its source "#x" is a bad token).
 * An IDENTIFIER is an optional '-' followed by decimal digits, of a value in [-2^63, 2^63); leading zeros do not count; a lone "-" is 0, as
 * in the reference (SA:869-887).  "+1", "--1", "1-", "1x" are bad tokens.  A token is read from left to right and the first thing wrong
 * with it decides: a byte that is no digit makes it BAD, a 20th significant digit or (at its end) a value outside the range makes it
 * TOO_LARGE.  DELIBERATE DEVIATION: the reference wraps around silently on overflow; here such a token is refused, not wrapped.
 * PER LINE, in this order (SA:495-654): a bad source -- the line is ignored, its target is NOT registered even if valid; a good source
 * is registered as a node, also when no target follows (NO_TARGET) or the target is bad (BAD_TARGET), and such a line adds no arc; a good
 * source and a good target -- the target is registered and the arc kept; further tokens on the line count as TRAILING, the arc is kept.
 * BVG_TEXT_NO_LOOPS drops x -> x after both ends are registered ("5 5" alone: one node, no arc); BVG_TEXT_SYMMETRIZE adds the reverse
 * of every kept arc; a duplicate arc appears once.
 * NODE NUMBERS.  An identifier's node number is the rank of its first occurrence among all first occurrences; ids[node] is the
 * identifier; nodes = the distinct registered identifiers.  Nothing depends on the order in which the device gets to the lines.
 * GIVEN NUMBERING (known_ids != NULL; the reference's translation function, for numeric identifiers): node i has identifier known_ids[i],
 * nodes = n_known whatever the text mentions (an identifier never mentioned is an isolated node), ids = known_ids.  A line of two
 * identifiers whose source is not among them is skipped and counted as UNKNOWN_SOURCE, else one whose target is not as UNKNOWN_TARGET
 * (a line that is NO_TARGET, BAD_TARGET or TOO_LARGE is that, whoever its source is).  A value that occurs twice
 * in known_ids: BVG_E_ARG.  known_ids == NULL with n_known > 0, or n_known < 0: BVG_E_ARG.
 * THE REPORT (rep may be NULL): lines = the line breaks, plus one when bytes follow the last of them; arcs = the lines whose arc was
 * kept (before the reverse arcs are added and duplicates removed; dropped loops are not in it); one count per category, every line in at
 * most one of bad_source, bad_target, no_target, too_large, unknown_source, unknown_target (too_large: the source or the target is
 * TOO_LARGE) and besides that in trailing when it has more than two tokens and both ends are identifiers; first_byte / first_line /
 * first_reason: the offending line (any category but TRAILING, which is a warning) of the smallest byte offset -- the offset of the
 * token at fault, of the source for NO_TARGET -- and first_reason = 0 when there is none.
 * BVG_TEXT_STRICT: an offending line refuses the call, BVG_E_IO, with that position and reason (BVG_SCATTERED_*) in *err, *out = NULL;
 * the report is filled all the same.  Unknown flag bits: BVG_E_ARG.
 * bvg_scattered_ids / _ids_dev: ids[nodes], under the capacity contract of bvg_text_get; BVG_E_UNSUPPORTED on a bvg_text that has none
 * (every other producer's).
 * DEVICE MEMORY on top of the text: 16 bytes per token and 32 per line while the lines are classified; then 16 bytes per occurrence
 * (a registered end of a line) plus a table of 16-byte slots, a power of two of at least 4/3 of the occurrences (21 to 43 bytes per
 * occurrence), 32 bytes per distinct identifier plus the sort's workspace while they are numbered, and 20 bytes per arc; then what an arc
 * list takes while it is sorted (44 bytes per arc, 88 with BVG_TEXT_SYMMETRIZE).  What stays in the object: 8 (nodes + 1) + 8 arcs +
 * 8 nodes.  Limits: a text of 8 TiB, 2^31 lines, 2^31 occurrences or 2^31 pairs (2^30 arcs with BVG_TEXT_SYMMETRIZE) or more:
 * BVG_E_UNSUPPORTED.  String identifiers (URLs) are not built. */
typedef struct bvg_scattered_report {       /* 104 bytes */
    uint64_t lines, arcs;
    uint64_t bad_source, bad_target, no_target, too_large, trailing, unknown_source, unknown_target, dropped_loops;
    uint64_t first_byte;                    /* the first offending line: offset of the token at fault */
    int64_t  first_line;                    /* 1-based; 0 when there is none */
    int32_t  first_reason;                  /* BVG_SCATTERED_BAD_SOURCE ...; 0 when there is none */
    int32_t  reserved;
} bvg_scattered_report;
enum { BVG_SCATTERED_BAD_SOURCE = 1, BVG_SCATTERED_BAD_TARGET = 2, BVG_SCATTERED_NO_TARGET = 3, BVG_SCATTERED_TOO_LARGE = 4,
       BVG_SCATTERED_TRAILING = 5, BVG_SCATTERED_UNKNOWN_SOURCE = 6, BVG_SCATTERED_UNKNOWN_TARGET = 7 };
#define BVG_TEXT_STRICT     4u
int  bvg_scattered_parse(const void* text, uint64_t nbytes, uint32_t flags, const int64_t* known_ids, int64_t n_known, int device,
                         bvg_text** out, bvg_scattered_report* rep, bvg_text_error* err);
int  bvg_scattered_parse_dev(const void* d_text, uint64_t nbytes, uint32_t flags, const void* d_known_ids, int64_t n_known, int device,
                             bvg_text** out, bvg_scattered_report* rep, bvg_text_error* err);
int  bvg_scattered_ids(bvg_text* t, int64_t* ids, uint64_t cap);
int  bvg_scattered_ids_dev(bvg_text* t, void* d_ids, uint64_t cap);

/* ---- Transform (Transform.java, "T"): map, filter, transpose, symmetrise, union, and the lex / Gray / random permutations ----
 * Every graph-valued call returns the CSR-in-HBM handle of the text graphs above (bvg_text): bvg_text_info / _get / _get_dev / _store /
 * _close serve it unchanged, and a result can be the source of the next call without leaving the device.
 * SOURCES.  bvg_transform_src names exactly one of a bvg_graph (decoded once into a CSR in HBM; its node base must be 0: BVG_E_ARG; a
 * malformed stream gives the decode's status, a successor outside [0, nodes) BVG_E_EOF) and a bvg_text (used where it lies, never
 * changed).  Both or neither set: BVG_E_ARG.  The two sources of bvg_transform_union must live on one device (BVG_E_ARG).
 * Every call works on the whole CSR in HBM.  LIMITS: a source or a result of 2^31 arcs or more (the prefix sums of the pairs and the
 * filter stages take fewer than 2^31 elements), or a permutation of 2^31 nodes or more: BVG_E_UNSUPPORTED; a map value of 2^40 or
 * more: BVG_E_NOMEM.  *out is written on success only: every failure leaves it untouched.  The _dev twins take the caller's array in
 * device memory.
 *   bvg_transform_from_csr   a handle over a copy of the caller's CSR, validated as bvg_store validates its input (adj_off[0] = 0, never
 *                            decreasing, lists strictly increasing and inside [0, nodes): else BVG_E_ARG).
 *   bvg_transform_identity   the source as a handle of its own (a copy).
 *   bvg_transform_map        T.mapOffline (T:1208-1269).  map_len != nodes or a value below -1: BVG_E_ARG.  -1 deletes the node and every
 *                            arc that touches it.  The result has max(map) + 1 nodes (0 when every entry is -1; values at or beyond
 *                            `nodes` give empty tail nodes).  Equal images merge, duplicate arcs collapse, loops created by merging stay.
 *   bvg_transform_filter     T.filterArcs with T.NO_LOOPS (node_class must be NULL and class_len 0) or NodeClassFilter (T:154-194) with
 *                            keepOnlySame true (SAME_CLASS: arcs between nodes of equal class stay) / false (DIFFERENT_CLASS); class_len
 *                            must equal nodes.  The node count is unchanged.
 *   bvg_transform_transpose  T.transposeOffline.   bvg_transform_symmetrize  T.symmetrizeOffline; with BVG_TRANSFORM_DROP_LOOPS
 *                            T.simplifyOffline.   bvg_transform_union  T.union: max(nodes_a, nodes_b) nodes, common arcs once; with
 *                            BVG_TRANSFORM_DROP_LOOPS the loops are dropped (T.simplify(g, t)).  Unknown flag bits: BVG_E_ARG.
 *   bvg_transform_permutation   perm[node] = the node's new name, ready for bvg_transform_map; perm holds `nodes` entries.
 *     BVG_PERM_LEX   the order of T:2017-2032 AS THE CODE HAS IT: the first differing position decides, a list that ends goes before one
 *                    that continues, and otherwise the LARGER successor goes first (the comparator returns the sign of b - a; its
 *                    javadoc says the opposite).
 *     BVG_PERM_GRAY  the order of T:1946-1975: the same walk with parity = the position is odd.  At an even position a list that ends
 *                    goes first, otherwise the larger successor; at an odd position the smaller successor goes first and a list that
 *                    ends goes last.
 *     Equal lists (the reference's quicksort leaves them in no particular order) are ordered by node id: the result is unique and one
 *     the reference could have produced.
 *     BVG_PERM_RANDOM  the order of (mix64(seed, node), node), the library's own sequence (not XoRoShiRo128PlusRandom's):
 *         z = seed + (node + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *         z = (z ^ (z >> 27)) * 0x94D049BB133111EB;    mix64 = z ^ (z >> 31)          (all in 64-bit unsigned arithmetic)
 * DEVICE MEMORY, besides source and result: map 32 bytes per arc plus the sort's workspace; transpose 16 per arc plus the sort's;
 * filter 12 per arc; union 12 per node; a permutation 36 bytes per node plus the sorts' workspaces.  BVG_E_NOMEM leaves nothing allocated. */
typedef struct bvg_transform_src { bvg_graph* graph; bvg_text* csr; } bvg_transform_src;   /* exactly one non-NULL */
enum { BVG_TRANSFORM_NO_LOOPS = 0, BVG_TRANSFORM_SAME_CLASS = 1, BVG_TRANSFORM_DIFFERENT_CLASS = 2 };
enum { BVG_PERM_LEX = 0, BVG_PERM_GRAY = 1, BVG_PERM_RANDOM = 2 };
#define BVG_TRANSFORM_DROP_LOOPS 1u
int  bvg_transform_from_csr(int64_t nodes, const uint64_t* adj_off, const int64_t* adj, int device, bvg_text** out);
int  bvg_transform_from_csr_dev(int64_t nodes, const void* d_adj_off, const void* d_adj, int device, bvg_text** out);
int  bvg_transform_identity(const bvg_transform_src* src, bvg_text** out);
int  bvg_transform_map(const bvg_transform_src* src, const int64_t* map, int64_t map_len, bvg_text** out);
int  bvg_transform_map_dev(const bvg_transform_src* src, const void* d_map, int64_t map_len, bvg_text** out);
int  bvg_transform_filter(const bvg_transform_src* src, int kind, const int64_t* node_class, int64_t class_len, bvg_text** out);
int  bvg_transform_filter_dev(const bvg_transform_src* src, int kind, const void* d_node_class, int64_t class_len, bvg_text** out);
int  bvg_transform_transpose(const bvg_transform_src* src, bvg_text** out);
int  bvg_transform_symmetrize(const bvg_transform_src* src, uint32_t flags, bvg_text** out);
int  bvg_transform_union(const bvg_transform_src* a, const bvg_transform_src* b, uint32_t flags, bvg_text** out);
int  bvg_transform_permutation(const bvg_transform_src* src, int kind, uint64_t seed, int64_t* perm);
int  bvg_transform_permutation_dev(const bvg_transform_src* src, int kind, uint64_t seed, void* d_perm);

/* ---- Compose (Transform.compose, T:1666-1775, the unlabelled form): the product of two graphs, every row hashed on chip ----
 * The result has n = max(nodes0, nodes1) nodes.  Row x is the sorted set of the successors in g1 of the successors of x in g0: the union of
 * N1(y) over y in N0(x) with y < nodes1.  Rows x >= nodes0 are empty.  A successor y >= nodes1 contributes nothing: the reference would
 * throw when its iterator reaches such a node; here a node a graph does not have is a node without successors, as in the padding of
 * bvg_transform_union.  The sources are those of Transform above (a bvg_graph is decoded once and checked, node base 0: else BVG_E_ARG;
 * both or neither member set, or a NULL source: BVG_E_ARG); when g0 and g1 name the same handle it is resolved once.  The result is the
 * bvg_text of the transforms and can be the source of the next call.
 * LIMITS: a source or a result of 2^31 arcs or more, or 2^31 nodes or more: BVG_E_UNSUPPORTED.  A row holds at most nodes1 < 2^31
 * successors, so no single row's count can wrap.  The number of products (pairs of an arc x -> y of g0 and an arc y -> z of g1) has no
 * limit: no stage stores them.  Sources on different devices: BVG_E_ARG.  *out is written on success only.  `report` (may be NULL) is filled
 * on success, and also when the result is refused for its size: products, rows, limit, and arcs = the total that was refused.
 * DEVICE MEMORY, besides sources and result: 16 bytes per node (the rows' bounds, 8; their lengths, 4; the tier lists, 4; the scan's
 * temporaries) plus 8 bytes per row of tier 2, and tier 2's workspace: hash tables of 16 pow2ceil(min(bound, nodes)) bytes per row, as many
 * rows side by side as fit 256 MiB (a row whose table alone is larger gets a workspace of that size); the host holds 12 bytes per node
 * during the call.  BVG_E_NOMEM leaves nothing allocated.  A probe sequence that does not end within its table (it cannot: a table is at
 * most half full) is BVG_E_HIP, never a spin. */
typedef struct bvg_compose_report {   /* 64 bytes */
    uint64_t products;     /* sum of the rows' bounds: arcs (x, y) of g0 times outdeg1(y) */
    uint64_t arcs;         /* of the result */
    uint64_t rows[3];      /* rows with a bound > 0 that tier 0 (a wavefront, LDS) / 1 (a workgroup, LDS) / 2 (a workgroup, HBM) took */
    uint64_t limit[2];     /* the largest bound a row of tier 0 / tier 1 may have, in this build */
    uint64_t batches;      /* launches of tier 2's batches per pass; 0 when no row needed it */
} bvg_compose_report;
int  bvg_compose(const bvg_transform_src* g0, const bvg_transform_src* g1, bvg_compose_report* report, bvg_text** out);

/* ---- Arc-labelled graphs on the device: Transform's labelled half and BitStreamArcLabelledImmutableGraph.store ("BS") ----
 * A bvg_lgraph is a graph as the transforms above hold it (a CSR in HBM) plus int32 labels[arcs] in successor order and the label class:
 * kind BVG_LABEL_GAMMA_INT (GammaCodedIntLabel: every label >= 0) or BVG_LABEL_FIXED_INT (FixedWidthIntLabel: width in 0..31,
 * FixedWidthIntLabel.java:41-42, every label in [0, 2^width)).  Every graph-valued call goes from bvg_lgraph to bvg_lgraph and keeps the class, so
 * a result can be the source of the next call, be read back, or be written as a label stream without leaving the device.  The list label
 * classes are BVG_E_UNSUPPORTED everywhere here.  *out is written on success only; NULL handles, unknown kinds and strategies: BVG_E_ARG,
 * decided before any handle is looked at.
 *   bvg_lgraph_from_csr[_dev]  a handle over a copy of the caller's CSR and labels.  The CSR is validated exactly as bvg_transform_from_csr
 *                        validates it (the same kernel, the same refusals); the labels are validated on the device: a negative gamma label, a
 *                        fixed label outside [0, 2^width) or a width outside 0..31 is BVG_E_ARG, a list kind BVG_E_UNSUPPORTED.
 *   bvg_lgraph_from_labelled   an open BVGraph and its label stream: the graph is decoded once and checked as a bvg_transform_src is, the labels
 *                        through bvg_labels_decode_range_dev (its errors are handed on unchanged).  Different devices, different node counts or
 *                        a node base other than 0: BVG_E_ARG; list labels, and a FixedWidthIntLabel of 32 bits: BVG_E_UNSUPPORTED.
 *   bvg_lgraph_info / _get / _get_dev   sizes and class; adj_off[nodes + 1], adj[arcs], labels[arcs] under the capacity contract of bvg_text_get
 *                        (any of the three may be NULL; a capacity in elements below the size: BVG_E_CAPACITY, nothing written).
 *   bvg_lgraph_underlying   the unlabelled graph as a bvg_text of its own (a copy): every bvg_transform_* call, bvg_compose and bvg_text_store
 *                        apply to it.
 *   bvg_lgraph_transpose T.transposeOffline(ArcLabelledImmutableGraph...) (T:1337-1631): arc (x, y) with label l becomes (y, x) with label l, lists
 *                        sorted by successor.  (target, source) is unique, so nothing about the result is left open.
 *   bvg_lgraph_union     T.union / UnionArcLabelledImmutableGraph: max(nodes_a, nodes_b) nodes; an arc of one source keeps its label, an arc of
 *                        both gets merge(label_a, label_b), a's label first (UnionArcLabelledImmutableGraph.java:188).  Strategies:
 *                        BVG_LMERGE_KEEP_FIRST (Labels.KEEP_FIRST_MERGE_STRATEGY, the only one the reference ships), BVG_LMERGE_MIN, BVG_LMERGE_MAX.
 *                        All three pick one of their arguments, so the result is storable in the sources' class.  A LabelMergeStrategy written
 *                        by the user is Java code and cannot run on the device: there is no entry point for one.  Sources whose (kind, width)
 *                        differ or that live on different devices: BVG_E_ARG.
 *   bvg_lgraph_symmetrize   union(g, transpose(g), strategy), as T:633-635 has it.
 *   bvg_lgraph_filter    T.filterArcs with a LabelledArcFilter.  BVG_LFILTER_NO_LOOPS / _SAME_CLASS / _DIFFERENT_CLASS are the filters of
 *                        bvg_transform_filter under the same numbers and rules (node_class NULL and class_len 0 without classes; class_len =
 *                        nodes with them); BVG_LFILTER_LOWER_BOUND is T.LowerBound AS THE CODE HAS IT (T:213): an arc stays iff
 *                        label >= lower_bound (the javadoc says "larger").  lower_bound must be 0 with every other kind, node_class NULL with
 *                        LOWER_BOUND: BVG_E_ARG.  The node count is unchanged.
 *   bvg_lgraph_store_labels   BS.store (BS:654-684): the bytes of basename.labels -- per arc gamma(label) (2 msb(label + 1) + 1 bits, up to 63) or
 *                        `width` bits, MSB first, zero-padded to a byte -- and label_offsets[nodes + 1], the bit position of every node's first
 *                        label (write basename.labeloffsets from their gamma-coded gaps after a leading gamma(0)).  Width 0: an empty stream and
 *                        offsets all zero.  Both buffers are malloc'ed (bvg_free), as bvg_text_store returns its buffers.  _dev: the caller's
 *                        device buffers, d_stream of `cap` bytes and d_label_offsets of nodes + 1 uint64 (either may be NULL); *nbytes is always
 *                        filled, cap below it is BVG_E_CAPACITY and nothing is written.
 * LIMITS: a source or a result of 2^31 arcs or more: BVG_E_UNSUPPORTED.  DEVICE MEMORY, besides sources and result: transpose 16 bytes per arc
 * plus the sort's workspace; union 4 bytes per arc of a and 16 per arc of b; symmetrize both, and the transpose itself; filter 12 per arc;
 * store_labels 12 per arc, 8 per node and the stream.  BVG_E_NOMEM leaves nothing allocated.
 * Not built: list labels through the transforms, user-written strategies, filters and semirings, several devices.  (The composition over a
 * semiring is bvg_lcompose, below.) */
typedef struct bvg_lgraph bvg_lgraph;
enum { BVG_LMERGE_KEEP_FIRST = 0, BVG_LMERGE_MIN = 1, BVG_LMERGE_MAX = 2 };
enum { BVG_LFILTER_NO_LOOPS = 0, BVG_LFILTER_SAME_CLASS = 1, BVG_LFILTER_DIFFERENT_CLASS = 2, BVG_LFILTER_LOWER_BOUND = 3 };
int  bvg_lgraph_from_csr(int64_t nodes, const uint64_t* adj_off, const int64_t* adj, const int32_t* labels, int kind, int width, int device, bvg_lgraph** out);
int  bvg_lgraph_from_csr_dev(int64_t nodes, const void* d_adj_off, const void* d_adj, const void* d_labels, int kind, int width, int device, bvg_lgraph** out);
int  bvg_lgraph_from_labelled(bvg_graph* g, bvg_labels* labels, bvg_lgraph** out);
void bvg_lgraph_close(bvg_lgraph* l);
int  bvg_lgraph_info(const bvg_lgraph* l, int64_t* nodes, uint64_t* arcs, int* kind, int* width);
int  bvg_lgraph_get(bvg_lgraph* l, uint64_t* adj_off, uint64_t off_cap, int64_t* adj, uint64_t adj_cap, int32_t* labels, uint64_t labels_cap);
int  bvg_lgraph_get_dev(bvg_lgraph* l, void* d_adj_off, uint64_t off_cap, void* d_adj, uint64_t adj_cap, void* d_labels, uint64_t labels_cap);
int  bvg_lgraph_underlying(const bvg_lgraph* l, bvg_text** out);
int  bvg_lgraph_transpose(const bvg_lgraph* src, bvg_lgraph** out);
int  bvg_lgraph_union(const bvg_lgraph* a, const bvg_lgraph* b, int strategy, bvg_lgraph** out);
int  bvg_lgraph_symmetrize(const bvg_lgraph* src, int strategy, bvg_lgraph** out);
int  bvg_lgraph_filter(const bvg_lgraph* src, int kind, const int64_t* node_class, int64_t class_len, int64_t lower_bound, bvg_lgraph** out);
int  bvg_lgraph_store_labels(const bvg_lgraph* l, uint8_t** stream, uint64_t* nbytes, uint64_t** label_offsets);
int  bvg_lgraph_store_labels_dev(const bvg_lgraph* l, void* d_stream, uint64_t cap, uint64_t* nbytes, void* d_label_offsets);

/* ---- Labelled compose (Transform.compose(ArcLabelledImmutableGraph, ArcLabelledImmutableGraph, LabelSemiring), T:1792-1918) ----
 * The sparse matrix product of two arc-labelled graphs over a semiring.  The result has max(nodes0, nodes1) nodes; row x holds the successors
 * z of bvg_compose's row x, and the label of (x, z) is the semiring's sum, over every y < nodes1 with x -> y in g0 and y -> z in g1, of
 * label0(x, y) (x) label1(y, z).  An arc exists wherever the unlabelled product has one, whatever its label (the reference puts
 * unconditionally, T:1849), so bvg_lgraph_underlying of the result is, for every semiring, bvg_compose of the sources' underlying graphs.
 * SEMIRINGS: a LabelSemiring written by the user is Java code and cannot run on the device (as a LabelMergeStrategy cannot): the menu is
 * BVG_SEMIRING_<ADD>_<MULTIPLY>.  MIN_PLUS is two-hop shortest paths (the reference's only test), PLUS_TIMES the ordinary matrix product, MAX_MIN
 * the widest two-hop path.  Every `add` is commutative and associative on integers, so the result does not depend on the order in which the
 * device meets the products: the call is deterministic.
 * LABEL CLASS: sources whose (kind, width) differ or that live on different devices: BVG_E_ARG (T:1793).  The result keeps the sources' kind.
 * BVG_LABEL_FIXED_INT: out_width in 0..31 is the result's width, -1 keeps the sources' (a (min, +) sum needs one bit more than its terms);
 * BVG_LABEL_GAMMA_INT: out_width must be -1.  Any other out_width, an unknown semiring, a NULL handle or a NULL `out`: BVG_E_ARG, decided before
 * any handle is looked at.
 * ARITHMETIC (a deviation from the reference): the reference adds and multiplies Java ints and wraps silently.  Here every label is accumulated
 * exactly in 64 bits, and a result label outside the result's class -- [0, 2^31 - 1] for gamma, [0, 2^out_width) for fixed -- refuses the call
 * with BVG_E_ARG: nothing is written to *out, and the report holds how many arcs were out of range and the smallest (row, successor) among them
 * (row first), which is as deterministic as the result.  PLUS_TIMES: every product is clamped to 2^32 before it is added; a key receives
 * fewer than 2^31 products, so the sum stays below 2^63 and cannot wrap, and it is exact whenever it is in range (a clamped product alone
 * is out of range).
 * `report` (may be NULL) is filled on success and on the two refusals that come with data: the result refused for its size (arcs = the total
 * that was refused) and the range refusal.
 * LIMITS: those of bvg_compose -- a source or a result of 2^31 arcs or more, or 2^31 nodes or more: BVG_E_UNSUPPORTED.  The list label kinds:
 * BVG_E_UNSUPPORTED.  *out is written on success only.
 * DEVICE MEMORY, besides sources and result: 16 bytes per node (the rows' bounds, their lengths, the tier lists, the scan's temporaries) plus
 * 8 bytes per row of tier 2, and tier 2's workspace: hash tables of 32 pow2ceil(min(bound, nodes)) bytes per row (a key and a 64-bit value a
 * slot), as many rows side by side as fit 512 MiB (a row whose table alone is larger gets a workspace of that size); the host holds 12 bytes
 * per node during the call.  BVG_E_NOMEM leaves nothing allocated.  A probe sequence that does not end within its table is BVG_E_HIP, never
 * a spin. */
enum { BVG_SEMIRING_MIN_PLUS = 0, BVG_SEMIRING_MAX_PLUS = 1, BVG_SEMIRING_MAX_MIN = 2, BVG_SEMIRING_MIN_MAX = 3, BVG_SEMIRING_PLUS_TIMES = 4 };   /* (add, multiply) */
typedef struct bvg_lcompose_report {   /* 88 bytes */
    uint64_t products;          /* as bvg_compose_report: sum of the rows' bounds */
    uint64_t arcs;              /* of the result */
    uint64_t rows[3];           /* rows with a bound > 0 that tier 0 / 1 / 2 took */
    uint64_t limit[2];          /* the largest bound a row of tier 0 / tier 1 may have, in this build (a slot is 16 bytes here: not bvg_compose's) */
    uint64_t batches;           /* launches of tier 2's batches per pass; 0 when no row needed it */
    uint64_t out_of_range;      /* arcs whose label is outside the result's class; 0 on success */
    int64_t  first_row;         /* the smallest (row, successor) among them, row first; -1, -1 when there is none */
    int64_t  first_successor;
} bvg_lcompose_report;
int  bvg_lcompose(const bvg_lgraph* g0, const bvg_lgraph* g1, int semiring, int out_width, bvg_lcompose_report* report, bvg_lgraph** out);

/* ---- synthetic-workload helper (bench only): K back-to-back copies of the graph ----
 * BV records are translation invariant (every value is coded relative to the node id, Appendix A.3
 * of SURVEY.md), so the concatenation of K copies of the bit stream is a valid BVGraph with K*nodes
 * nodes in which copy j is the base graph shifted by j*nodes.  Built on the device. */
int bvg_tile(const bvg_graph* base, int64_t copies, bvg_graph** out);
/* The same with k <= 16 different base graphs (same device, same BV parameters): the cycle {bases[0], ..., bases[k-1]} repeated `cycles`
 * times -- a synthetic workload whose tiles differ in seed and degree mix. */
int bvg_mosaic(const bvg_graph* const* bases, int k, int64_t cycles, bvg_graph** out);

/* ---- tuning knobs (optional) ---- */
typedef struct bvg_tuning {
    uint32_t block_bits;     /* target compressed bits per node block (one wavefront each); 0 = default */
    uint32_t force_wide;     /* 1 = use the 64-bit successor kernels even when every node id fits 32 bits (nodes <= 2^32 - 256); steady-state scans of
                                such a graph still run the scan kernel, on 32-bit lists of ids relative to a per-block base */
    uint32_t force_slow;     /* 1 = route every block through the global-memory slow path (tests) */
    uint32_t reserved;       /* low byte 2 = experimental streaming kernel as tier 0; bits 8.. = its grab threshold */
    uint32_t no_index;       /* 1 = calls on THIS handle neither build nor read the residual skip index (nor the validation marks, so every
                                block stays on the checking kernels): what a cold consumer gets from a graph it scans once; bench.py times
                                a bvg_copy() flyweight with it (`value_no_index`) beside the indexed steady state (ABI version 3).
                                2 = "marks only" (round 6): the index THIS handle builds holds the validation marks (one byte per block of
                                ~4 KiB of stream: the lean scan kernel takes the block) but entries only for lists of >= 4 096 residuals --
                                ~0.03 % of the stream instead of ~50 %; the residuals of a list are then one lane's walk.  Measured
                                (profiles/r06_ab_marks_*.txt): eu15 stand-in 113 G edges/s (indexed 310, checking kernels 45), cnr-2000
                                tiled 142 (151, 80).
                                The index belongs to the graph, shared by every bvg_copy() flyweight, not to the handle that builds it: the mode
                                (0 / 2) of the handle that builds it FIRST decides its granularity, and an index that exists already is used as it
                                is.  A later scan outside it widens it to the whole graph in its own granularity and width, whatever the calling
                                handle's mode; a handle of the other width (force_wide) never replaces it and scans without it.  Only when no good
                                index exists (none yet, or its build failed) does the calling handle's mode decide.  Values above 2 are refused
                                with BVG_E_ARG (ABI version 4). */
} bvg_tuning;
int bvg_set_tuning(bvg_graph* g, const bvg_tuning* t);

const char* bvg_strerror(int status);
int bvg_abi_version(void);

/* ---- checksum definition (shared with the CPU oracle) ----
 *   h  = (u32)x * 0x9E3779B1 + (u32)(x >> 32) * 0x85EBCA77;  h ^= h >> 15;  h *= 0x2C1B3C6D;  h ^= h >> 12     (mod 2^32)
 *   k1 = h | 1;   k0 = h * 0x297A2D39;  k0 ^= k0 >> 15                   (a per-node key, k1 odd; ten 32-bit operations)
 *   bvg_arc_mix(x, y) = k1 * y + k0                                      (mod 2^64)
 * chk = sum of bvg_arc_mix over all arcs, mod 2^64 (a successor missing from a list that came out short -- the -1 the decode reports
 * whatever the node base -- counts as y + node_base = 2^64 - 1): commutative, so node-range shards reduce with
 * a plain sum (one RCCL all-reduce of {arcs, chk}).  Linear in y under the node's key: a kernel pays
 * one 32 x 32 + 64 multiply-add per successor (the reference's SpeedTest.java:127-135 does nothing
 * with them) and adds d * k0 per node.
 * WHAT THE SCAN MUST DO (round 6, the contract the timed region is held to): ONE multiply-add per
 * PRODUCED successor -- every decoded residual, every element of an interval, every element a copy
 * block keeps, leaf or stored list alike, is read (or generated) and multiplied on its own.  The
 * linear form has closed forms over runs (len * left + len (len - 1) / 2 for an interval, a
 * difference of prefix sums for a kept block): the kernels never use one -- that would be work
 * skipped.  The only per-node constants folded are d * k0 and d * k1 * base (base = the node base /
 * block base every id of the block is stored relative to).  tests/test_gpu_checksum_integrity.py
 * changes ONE element of a stored list and checks that every node copying it moves by exactly
 * k1(node) * delta, through the lean kernel.
 * WHAT IT DETECTS: a single wrong, missing, surplus or misattributed successor changes the sum
 * unless k1 * dy + (0 or k0) == 0 mod 2^64 -- never for one wrong value with |dy| < 2^63 (k1 is
 * odd), with probability ~2^-32 for a missing / surplus / misattributed one (32-bit keys; nodes
 * whose 32-bit hashes collide share a key).  Two errors inside ONE node that cancel in the sum of
 * its successors are invisible: the materialising parity tests (every successor against the oracle
 * / the golden) are the primary gate, this is the scan's self-check; bench.py's untimed gate also
 * materialises one tile through bvg_decode_range: every successor against the oracle's.  (Rounds 1-4 used a non-linear
 * mix: six vector instructions per arc, a quarter of what a decoded successor has to cost.) */
uint64_t bvg_arc_mix(uint64_t x, uint64_t y);

#ifdef __cplusplus
}
#endif
#endif /* BVGRAPH_HIP_H */
