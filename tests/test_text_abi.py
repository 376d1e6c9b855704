"""CPU: the text graph entry points (bvg_text_*) are declared in include/bvgraph_hip.h, exported by the library cross-compiled for gfx950
and bound by the ctypes mirror; the ABI version stays 4; argument checks, the offsets writer and the command lines need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import CNR, ROOT

NAMES = sorted(["bvg_text_parse_ascii", "bvg_text_parse_ascii_dev", "bvg_text_parse_arcs", "bvg_text_parse_arcs_dev", "bvg_text_close", "bvg_text_info",
                "bvg_text_get", "bvg_text_get_dev", "bvg_text_store", "bvg_text_format_ascii", "bvg_text_format_ascii_dev", "bvg_text_format_arcs",
                "bvg_text_format_arcs_dev", "bvg_text_format_csr"])


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvgraph_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bvg_text_[a-z_0-9]*)\s*\(", text))) == NAMES
    assert re.search(r"#define BVG_TEXT_SYMMETRIZE 1u", text) and re.search(r"#define BVG_TEXT_NO_LOOPS\s+2u", text)
    for name, value in (("BAD_BYTE", 1), ("BAD_HEADER", 2), ("TOO_LARGE", 3), ("NOT_NODE", 4), ("NOT_INCREASING", 5), ("SHIFT_RANGE", 6), ("ARC_FIELDS", 7), ("EOF", 8),
                        ("ASCII", 0), ("ARCS", 1)):
        assert re.search(r"\bBVG_TEXT_%s = %d\b" % (name, value), text), name
    assert re.search(r"#define BVG_ABI_VERSION 4\b", text)                      # additive: the version stays


def test_library_exports_and_mirror_binds_them(W):
    lib = C.CDLL(W.build())
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert lib.bvg_abi_version() == 4
    sigs = W._abi.text_signatures()
    assert sorted(sigs) == NAMES
    L = W.textgraph._text_fns()
    for n in NAMES:
        assert getattr(L, n).argtypes == sigs[n]
    assert C.sizeof(W.TextError) == 24 and W.TextError.line.offset == 8 and W.TextError.reason.offset == 16
    assert W._abi.TEXT_REASONS == {1: "bad_byte", 2: "bad_header", 3: "too_large", 4: "not_node", 5: "not_increasing", 6: "shift_range", 7: "arc_fields", 8: "eof"}
    assert (W._abi.TEXT_ASCII, W._abi.TEXT_ARCS, W._abi.TEXT_SYMMETRIZE_FLAG, W._abi.TEXT_NO_LOOPS_FLAG) == (0, 1, 1, 2)


def test_argument_checks_need_no_device(W):
    L = W.textgraph._text_fns()
    h = C.c_void_p(0x1234); err = W.TextError(byte=7); nb = C.c_uint64(5)
    assert L.bvg_text_parse_ascii(b"1\n\n", 3, 0, None, C.byref(err)) == W.E_ARG               # no out
    assert L.bvg_text_parse_ascii(None, 3, 0, C.byref(h), C.byref(err)) == W.E_ARG             # bytes promised, none given
    assert L.bvg_text_parse_arcs(b"1 2\n", 4, 0, 4, 0, 0, C.byref(h), C.byref(err)) == W.E_ARG   # unknown flag bit
    assert L.bvg_text_parse_arcs(b"1 2\n", 4, 0, 0, -1, 0, C.byref(h), C.byref(err)) == W.E_ARG  # negative min_nodes
    assert h.value == 0x1234 and err.byte == 7                                                   # nothing was written
    assert L.bvg_text_info(None, None, None) == W.E_ARG and L.bvg_text_get(None, None, 0, None, 0) == W.E_ARG
    assert L.bvg_text_store(None, C.byref(W.default_params()), 0, C.byref(h), C.byref(nb), C.byref(h)) == W.E_ARG
    for fn in (L.bvg_text_format_ascii, L.bvg_text_format_ascii_dev):
        assert fn(None, 0, 1, None, 0, C.byref(nb)) == W.E_ARG
    for fn in (L.bvg_text_format_arcs, L.bvg_text_format_arcs_dev):
        assert fn(None, 0, 1, 0, None, 0, C.byref(nb)) == W.E_ARG
    off = np.array([0, 1], dtype=np.uint64); adj = np.zeros(1, dtype=np.int64)
    assert L.bvg_text_format_csr(2, 0, 1, off.ctypes.data, adj.ctypes.data, 0, None, 0, C.byref(nb)) == W.E_ARG      # no such kind
    assert L.bvg_text_format_csr(0, -1, 1, off.ctypes.data, adj.ctypes.data, 0, None, 0, C.byref(nb)) == W.E_ARG
    assert L.bvg_text_format_csr(0, 0, 1, off[::-1].copy().ctypes.data, adj.ctypes.data, 0, None, 0, C.byref(nb)) == W.E_ARG   # offsets that decrease
    assert L.bvg_text_format_csr(0, 0, 1, off.ctypes.data, None, 0, None, 0, C.byref(nb)) == W.E_ARG
    assert nb.value == 5
    L.bvg_text_close(None)                                                                       # a no-op


def test_mirrors_expose_the_surface(W):
    for name in ("ParsedGraph", "parse_ascii_graph", "parse_arc_list", "load_ascii_graph", "load_arc_list", "write_bvgraph", "format_csr",
                 "asciigraph_main", "arclist_main", "bvgraph_main", "TextError"):
        assert hasattr(W, name), name
    for cls in (W.BVGraph, W.EFGraph, W.ParsedGraph):
        assert hasattr(cls, "to_ascii_graph") and hasattr(cls, "to_arc_list")
    for name in ("num_nodes", "num_arcs", "csr", "store", "close"):
        assert hasattr(W.ParsedGraph, name)


def test_offsets_file_writer(W):
    """basename.offsets as the reference writes it: the fixture's own file comes back byte for byte, and both codings read back."""
    raw = open(CNR + ".offsets", "rb").read()
    off = W.decode_offsets(raw, 325557)
    assert W.coded_gaps(off, W.GAMMA) == raw
    odd = np.array([0, 0, 1, 2, 3, 4, 7, 8, 1 << 20, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40, (1 << 62) + 5], dtype=np.uint64)
    for coding in (W.GAMMA, W.DELTA):
        assert np.array_equal(W.decode_offsets(W.coded_gaps(odd, coding), len(odd) - 1, coding), odd)
    with pytest.raises(W.UnsupportedOperationException):
        W.coded_gaps(odd, W.ZETA)


def test_properties_text_reads_back(W):
    p = W.default_params(window_size=5, max_ref_count=2, min_interval_length=0, zeta_k=4, residual_coding=W.DELTA, offset_coding=W.DELTA)
    q = W.parse_properties(W.textgraph.properties_text(p, 10, 33, 1000))
    assert (q.nodes, q.arcs, q.window_size, q.max_ref_count, q.min_interval_length, q.zeta_k, q.residual_coding, q.offset_coding, q.block_coding) == \
        (10, 33, 5, 2, 0, 4, W.DELTA, W.DELTA, W.GAMMA)
    assert "compressionflags=\n" in W.textgraph.properties_text(W.default_params(), 0, 0, 0)


def test_command_lines(W, tmp_path, capsys):
    for main in (W.asciigraph_main, W.arclist_main, W.bvgraph_main):
        with pytest.raises(SystemExit):
            main([])                                                            # source and destination are required
    assert W.bvgraph_main(["-o", "a", "b"]) == 1                                # an option of the reference that is not built: a message
    assert "not supported" in capsys.readouterr().err
    assert W.bvgraph_main(["-c", "RESIDUALS_FOO", "a", "b"]) == 1
    with pytest.raises(SystemExit):
        W.asciigraph_main(["-g", "NoSuchGraph", "a", "b"])
    a = W.textgraph.bvgraph_arg_parser().parse_args(["-g", "ASCIIGraph", "-w", "5", "-m", "2", "-i", "0", "-k", "4", "-c", "RESIDUALS_GAMMA", "s", "d"])
    assert (a.graph_class, a.window_size, a.max_ref_count, a.min_interval_length, a.zeta_k, a.comp, a.sourceBasename, a.destBasename) == \
        ("ASCIIGraph", 5, 2, 0, 4, ["RESIDUALS_GAMMA"], "s", "d")
    a = W.textgraph.arclist_arg_parser().parse_args(["-S", "-1", "s", "d"])
    assert (a.graph_class, a.shift) == ("BVGraph", -1)
    with pytest.raises(W.IOException):
        W.bvgraph_main(["-g", "ASCIIGraph", str(tmp_path / "none"), str(tmp_path / "out")])
    with pytest.raises(W.IOException):
        W.arclist_main([str(tmp_path / "none"), str(tmp_path / "out")])


def test_compute_fails_loudly_without_a_gpu(W):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(W.DeviceError):
        W.parse_ascii_graph(b"1\n\n")
    with pytest.raises(W.DeviceError):
        W.parse_arc_list(b"0 1\n")
    with pytest.raises(W.DeviceError):
        W.format_csr(W.TEXT_ASCII, 0, [0, 1], [0])
