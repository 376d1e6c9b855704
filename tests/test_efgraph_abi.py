"""CPU: the host-only half of the EFGraph entry points (bvg_ef_*) -- properties parsing and every refusal, the offsets derivation
against the model, truncated streams, struct sizes -- and that the compute calls fail loudly without a GPU."""
import ctypes as C

import numpy as np
import pytest

import efgraph_model as M

PROPS = "#EFGraph properties\nnodes=10\narcs=33\nquantum=256\nbyteorder=LITTLE_ENDIAN\ngraphclass=it.unimi.dsi.big.webgraph.EFGraph\nversion=0\n"


def test_struct_sizes(W):
    assert C.sizeof(W.EFParams) == 32 and C.sizeof(W.ScanResult) == 72


def test_properties(W):
    p = W.parse_ef_properties(PROPS)
    assert (p.nodes, p.arcs, p.upper_bound, p.log2_quantum, p.big_endian) == (10, 33, 10, 8, 0)
    p = W.parse_ef_properties(PROPS.replace("LITTLE", "BIG").replace("quantum=256", "quantum=1\nupperbound=17").replace("big.webgraph", "webgraph"))
    assert (p.upper_bound, p.log2_quantum, p.big_endian) == (17, 0, 1)
    p = W.parse_ef_properties(PROPS.replace("version=0", "version=-1").replace("graphclass=", "graphclass=class ").replace("arcs=33\n", ""))
    assert (p.nodes, p.arcs) == (10, -1)


@pytest.mark.parametrize("text,exc", [
    (PROPS.replace("EFGraph\n", "BVGraph\n"), "IOException"),                  # another class (EFGraph.java:683)
    (PROPS.replace("graphclass=it.unimi.dsi.big.webgraph.EFGraph\n", ""), "IOException"),
    (PROPS.replace("version=0\n", ""), "IOException"),                         # "Missing format version information" (:686)
    (PROPS.replace("version=0", "version=1"), "IOException"),                  # a newer format (:687)
    (PROPS.replace("nodes=10\n", ""), "IOException"),
    (PROPS.replace("quantum=256\n", ""), "IOException"),
    (PROPS.replace("byteorder=LITTLE_ENDIAN\n", ""), "IOException"),
    (PROPS.replace("quantum=256", "quantum=96"), "IllegalArgumentException"),  # not a power of two (:693)
    (PROPS.replace("quantum=256", "quantum=0"), "IllegalArgumentException"),
    (PROPS.replace("LITTLE_ENDIAN", "PDP_ENDIAN"), "IllegalArgumentException"),  # "Unknown byte order" (:698)
    (PROPS + "upperbound=9\n", "IllegalArgumentException"),                    # below the number of nodes
    (PROPS.replace("nodes=10", "nodes=-1"), "IllegalArgumentException"),
])
def test_properties_refusals(W, text, exc):
    with pytest.raises(getattr(W, exc)):
        W.parse_ef_properties(text)


@pytest.mark.parametrize("q", [0, 3, 8])
@pytest.mark.parametrize("ub", ["n", "n+7", "n2", "2^40"])
def test_host_derivation_equals_the_models_offsets(W, q, ub):
    n = 150
    lists = M.random_lists(n, 1500, seed=q, degrees=(0, 1, 2, 3, 63, 64, 65, 150))
    U = {"n": n, "n+7": n + 7, "n2": n * n, "2^40": 1 << 40}[ub]
    for order in ("LITTLE_ENDIAN", "BIG_ENDIAN"):
        data, off, _ = M.store(lists, U, q, order)
        p = W.EFParams(nodes=n, arcs=-1, upper_bound=U, log2_quantum=q, big_endian=int(order == "BIG_ENDIAN"))
        assert np.array_equal(W.derive_ef_offsets(p, data), off)
    assert np.array_equal(W.decode_offsets(M.write_delta_offsets(off), n, W.DELTA), off)       # basename.offsets is read by the existing entry point


def test_derivation_of_records_of_every_small_outdegree(W):
    """Each closed form on its own: one list of d successors, d = 0..130, for several upper bounds and quanta."""
    for U in (131, 1000, 1 << 33):
        for q in (0, 2, 8):
            lists = [np.arange(d, dtype=np.int64) for d in range(131)]
            data, off, _ = M.store(lists, U, q)
            p = W.EFParams(nodes=131, arcs=-1, upper_bound=U, log2_quantum=q, big_endian=0)
            assert np.array_equal(W.derive_ef_offsets(p, data), off)


def test_truncated_and_damaged_streams(W):
    lists = M.random_lists(150, 1500, seed=1)
    data, off, _ = M.store(lists, 150, 3)
    p = W.EFParams(nodes=150, arcs=-1, upper_bound=150, log2_quantum=3, big_endian=0)
    for cut in (0, 8, len(data) // 2 // 8 * 8, len(data) - 16):
        with pytest.raises(W.EOFException):
            W.derive_ef_offsets(p, data[:cut])
    with pytest.raises(W.EOFException):
        W.derive_ef_offsets(p, bytes(len(data)))                               # all zeros: the first gamma never ends
    huge = (1 << 33).to_bytes(8, "little") + bytes(64)                          # 33 zeros, a one: an outdegree of 2^33 - 1 and more
    with pytest.raises(W.UnsupportedOperationException):
        W.derive_ef_offsets(W.EFParams(nodes=1, arcs=-1, upper_bound=1, log2_quantum=0, big_endian=0), huge)
    with pytest.raises(W.IllegalArgumentException):
        W.derive_ef_offsets(W.EFParams(nodes=5, arcs=-1, upper_bound=4, log2_quantum=0, big_endian=0), data)
    assert np.array_equal(W.derive_ef_offsets(W.EFParams(nodes=0, arcs=0, upper_bound=0, log2_quantum=0, big_endian=0), bytes(8)), [0])


def test_compute_fails_loudly_without_a_gpu(W, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lists = [[1, 3], [], [0, 1, 2, 3], [2]]
    data, off, _ = M.store(lists, 4, 1)
    p = W.EFParams(nodes=4, arcs=7, upper_bound=4, log2_quantum=1, big_endian=0)
    with pytest.raises(W.DeviceError):
        W.EFGraph.from_memory(p, data, off)
    with pytest.raises(W.DeviceError):
        W.EFGraph.from_memory(p, data, None)
    with pytest.raises(W.DeviceError):
        W.store_efgraph(lists, 4, 1)
    base = str(tmp_path / "g")
    open(base + ".graph", "wb").write(data)
    open(base + ".offsets", "wb").write(M.write_delta_offsets(off))
    open(base + ".properties", "w").write(PROPS.replace("nodes=10", "nodes=4").replace("arcs=33", "arcs=7").replace("quantum=256", "quantum=2"))
    with pytest.raises(W.DeviceError):
        W.EFGraph.load(base)
    with pytest.raises(W.IOException):
        W.EFGraph.load(str(tmp_path / "does-not-exist"))
    assert W.efgraph_main([base]) == 1                                         # no destination: a message, not a crash
