"""CPU: the oracle's own derivation of the offsets (oracle/bvg_oracle.c, bvgo_write_offsets: the sequential node iterator from node 0, the
bit position before every record and behind the last -- BVGraph.writeOffsets, BVGraph.java:2595-2609), pinned on the reference's own
cnr-2000.offsets and on the encoder's offsets over the parameter sets of tests/test_gpu_derive.py; and the generator of
tests/test_gpu_derive_fuzz.py: the oracle derives every stream it draws, so no device case can end without a comparison."""
import numpy as np
import pytest

from conftest import CNR
from derive_cases import oracle_offsets
from test_gpu_derive import SETS, _shapes
from test_gpu_derive_fuzz import draw


def test_oracle_derives_the_offsets_of_the_cnr_2000_golden(oracle):
    g = oracle.Graph.load(CNR)
    want = oracle.decode_offsets(open(CNR + ".offsets", "rb").read(), g.params.nodes, g.params.offset_coding)
    bare = oracle.Graph.from_memory(g.params, open(CNR + ".graph", "rb").read(), None)
    assert bare.offsets() is None
    assert np.array_equal(bare.derive_offsets(), want)


@pytest.mark.parametrize("group", sorted(SETS))
def test_oracle_derives_the_encoders_offsets(W, tools, oracle, group):
    for name, (off, adj) in _shapes(tools, group):
        for kw in SETS[group]:
            st = tools.store((off, adj), W.default_params(**kw))
            assert np.array_equal(oracle_offsets(oracle, st.params, st.graph), st.offsets), (name, kw)


def test_oracle_reports_the_iterators_status(W, tools, oracle):
    st = tools.synth_store(2000, seed=1, threads=1)
    with pytest.raises(oracle.OracleError) as e:
        oracle_offsets(oracle, st.params, st.graph[:len(st.graph) // 2])
    assert e.value.code == -5                                               # EOFException from the bit stream
    with pytest.raises(oracle.OracleError) as e:
        oracle_offsets(oracle, st.params.clone(window_size=0), st.graph)     # (the stream holds references: read as outdegrees, it runs out)
    assert e.value.code == -5                                               # (it runs out: EOFException)


def test_every_drawn_fuzz_case_is_derived_by_the_oracle(W, tools, oracle):
    """2 000 cases of the device fuzz's generator: the oracle derives the encoder's offsets for every one (100 %: the generator leaves out
    what does not fit 64 bits, so the device test has nothing to skip)."""
    ok = 0
    for case in range(2000):
        what, st, route, expect = draw(np.random.default_rng([77, case]), tools, W)
        assert np.array_equal(oracle_offsets(oracle, st.params, st.graph), st.offsets), what
        ok += 1
    assert ok == 2000
