"""webgraph-big_amd — MI355X-native BVGraph successor-list decoding.

The package holds only what the decode path needs: csrc/ (HIP kernels + C ABI), host/ (the C++ mirror), bvgraph.py (host-side
mirror of the reference's ImmutableGraph / NodeIterator / LazyLongIterator API over the C ABI) and shard.py (the node-range
shard helpers bench.py and the tests share); experimental/ holds kernels that lost to the product's and are built only by
`make experimental`.  The CPU encoder and the synthetic graph generators are test tooling and live outside the package (tooling/).
"""
from ._abi import *  # noqa: F401,F403
from ._abi import Params, ScanResult, Tuning, StatsSummary, EFParams, TextError, ScatteredReport, TransformSrc, ComposeReport, default_params  # noqa: F401
from .bvgraph import (BVGraph, NodeIterator, LazyLongIterator, BVGraphError, IllegalArgumentException,  # noqa: F401
                      IllegalStateException, UnsupportedOperationException, IOException, EOFException, DeviceError,
                      NoSuchElementException, parse_properties, decode_offsets, arc_mix, build, lib, library_path,
                      BitStreamArcLabelledImmutableGraph, LabelledArcIterator, parse_label_spec, LABEL_GAMMA_INT, LABEL_FIXED_INT, LABEL_FIXED_INT_LIST, LABEL_FIXED_LONG_LIST,
                      scan_multi, mosaic, BALANCE_NODES, BALANCE_BITS, BALANCE_ARCS, store,
                      CC_SORT_BY_SIZE, ComponentsResult, store_components, load_components, components_main,
                      BFS_PARENT, BFS_COUNTERS, BreadthFirstVisit,
                      SCC_SORT_BY_SIZE, SCC_BUCKETS, SCC_COUNTERS, SCCResult, store_scc, load_scc, scc_main,
                      GraphStats, java_double_str, store_stats, stats_main,
                      GEO_COUNTERS, GeometricResult, parse_coefficients_spec, store_geometric, load_geometric, geometric_main,
                      HB_SUM_OF_DISTANCES, HB_HARMONIC, HyperBall, hyperball_main, store_floats, load_floats)
from .efgraph import EFGraph, parse_ef_properties, derive_ef_offsets, store_efgraph, write_efgraph, efgraph_main  # noqa: F401,E402
from . import textgraph  # noqa: F401,E402
from .textgraph import (ParsedGraph, parse_ascii_graph, parse_arc_list, parse_ascii_graph_dev, parse_arc_list_dev, load_ascii_graph, load_arc_list,  # noqa: F401,E402
                        format_csr, write_bvgraph, coded_gaps, asciigraph_main, arclist_main, bvgraph_main,
                        ScatteredGraph, parse_scattered_arcs, parse_scattered_arcs_dev, load_scattered_arcs, scattered_main)
from . import transform  # noqa: F401,E402
from .transform import (identity_graph, map_graph, filter_arcs, transpose_graph, symmetrize_graph, simplify_graph, union, remove_dangling,  # noqa: F401,E402
                        lexicographical_permutation, gray_code_permutation, random_permutation, permutation_dev, load_longs, store_longs, transform_main, compose, compose_main)
from . import labelled  # noqa: F401,E402
from .labelled import (LabelledGraph, transpose_labelled, union_labelled, symmetrize_labelled, filter_labelled_arcs, label_spec,  # noqa: F401,E402
                       labelled_transform_main, compose_labelled, labelled_compose_main, SEMIRING_MIN_PLUS, SEMIRING_MAX_PLUS, SEMIRING_MAX_MIN,
                       SEMIRING_MIN_MAX, SEMIRING_PLUS_TIMES)
