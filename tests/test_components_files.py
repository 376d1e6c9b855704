"""CPU: the result files of ConnectedComponents.main (.wcc / .wccsizes: BinIO.storeLongs -- big-endian longs, no header) and the
argument handling of components_main that needs no device."""
import numpy as np
import pytest


def test_wcc_files_are_big_endian_longs(W, tmp_path):
    comp = np.array([0, 0, 1, 2, 1, 0, (1 << 40) + 3], dtype=np.int64)
    sizes = np.array([3, 2, 1, 1], dtype=np.int64)
    paths = W.store_components(W.ComponentsResult(4, comp, sizes), str(tmp_path / "r"))
    assert paths == [str(tmp_path / "r.wcc"), str(tmp_path / "r.wccsizes")]
    raw = (tmp_path / "r.wcc").read_bytes()
    assert len(raw) == 8 * len(comp)
    assert raw[:16] == bytes(16) and raw[16:24] == b"\x00\x00\x00\x00\x00\x00\x00\x01"
    assert raw[48:56] == b"\x00\x00\x01\x00\x00\x00\x00\x03"
    assert (tmp_path / "r.wccsizes").read_bytes() == b"".join(int(v).to_bytes(8, "big") for v in sizes)
    c, s = W.load_components(str(tmp_path / "r"))
    assert c.dtype == np.int64 and np.array_equal(c, comp) and np.array_equal(s, sizes)


def test_wcc_without_sizes_writes_one_file(W, tmp_path):
    paths = W.store_components(W.ComponentsResult(1, np.zeros(5, dtype=np.int64)), str(tmp_path / "one"))
    assert paths == [str(tmp_path / "one.wcc")]
    assert not (tmp_path / "one.wccsizes").exists()
    c, s = W.load_components(str(tmp_path / "one"))
    assert s is None and np.array_equal(c, np.zeros(5, dtype=np.int64))


def test_components_main_arguments(W):
    from importlib import import_module
    ap = import_module("webgraph-big_amd.bvgraph").components_arg_parser()
    a = ap.parse_args(["g"])
    assert (a.basename, a.results_basename, a.sizes, a.renumber) == ("g", None, False, False)
    a = ap.parse_args(["-s", "--renumber", "g", "out"])
    assert (a.basename, a.results_basename, a.sizes, a.renumber) == ("g", "out", True, True)
    a = ap.parse_args(["--sizes", "-r", "g"])
    assert a.sizes and a.renumber
    with pytest.raises(SystemExit):
        W.components_main([])                                                  # the basename is required
    with pytest.raises(SystemExit):
        W.components_main(["-x", "g"])                                         # unknown option


def test_components_main_missing_graph_is_an_io_error(W, tmp_path):
    with pytest.raises(W.IOException):
        W.components_main([str(tmp_path / "does-not-exist")])
