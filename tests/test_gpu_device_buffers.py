"""The device-buffer entry points (include/bvgraph_hip.h, names ending in _dev) with torch HIP tensors as the buffers: bvg_open_dev,
bvg_decode_range_dev, bvg_transpose_dev, bvg_symmetrize_dev, bvg_labels_decode_range_dev.  Every result against the host calls, the
oracle or numpy; every output buffer has a sentinel-filled guard region behind its capacity that must stay untouched.

Each test runs its body in a fresh child process (this file as a script) that imports torch BEFORE the product library: torch's HIP
library asks for libamdhip64.so, the product's for libamdhip64.so.7, so a process that loaded the product first gets a second HIP runtime
from torch, which sees no device (bench.py imports torch first for the same reason)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 256
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A


def _buf(torch, n, dtype):
    return torch.full((n + GUARD,), SENT64 if dtype == torch.int64 else SENT32, dtype=dtype, device="cuda")


def _guard_ok(torch, t, frm):
    torch.cuda.synchronize()
    return bool((t[frm:] == (SENT64 if t.dtype == torch.int64 else SENT32)).all().item())


def _host(torch, t, n):
    torch.cuda.synchronize()
    return t[:n].cpu().numpy()


def _check_graph(g, og, n, what):
    o = og.scan()
    for _ in range(2):                                                          # (the second scan runs on the index the first one built)
        r = g.scan()
        assert (r["nodes"], r["arcs"], r["chk"]) == (o["nodes"], o["arcs"], o["chk"]), what
    deg, succ = g.decode_range(0, n)
    odeg, osucc = og.decode_range(0, n)
    assert np.array_equal(deg, odeg) and np.array_equal(succ, osucc), what
    for a, b in ((0, 1), (n // 3, n // 2), (n - 7, n)):
        ra, oa = g.scan(a, b), og.scan(a, b)
        assert (ra["arcs"], ra["chk"]) == (oa["arcs"], oa["chk"]), (what, a, b)
        d2, s2 = g.decode_range(a, b)
        od, os_ = og.decode_range(a, b)
        assert np.array_equal(d2, od) and np.array_equal(s2, os_), (what, a, b)
    nodes = np.array([n - 1, 0, n // 2, 17, n // 2], dtype=np.int64)
    bd, bs = g.successors_batch(nodes)
    assert np.array_equal(bs, np.concatenate([og.decode_range(int(x), int(x) + 1)[1] for x in nodes])), what


def _open_from_device_memory(W, tools, oracle, torch, wide_offsets):
    """bvg_open_dev adopts the graph tensor and reads the offsets tensor once: after the call the offsets tensor is overwritten (with the offsets in
    reverse order: wrong for every node, yet inside the stream) and everything still matches the oracle.  With BVG_WIDE_OFFSETS=1 the plain array is
    used in place: it stays alive and intact, and the results are checked again after more calls."""
    assert bool(os.environ.get("BVG_WIDE_OFFSETS")) == wide_offsets
    n = 20000
    st = tools.synth_store(n, seed=31, synth=tools.eu_like(), threads=4)
    og = oracle.Graph.from_memory(oracle.Params(**st.params.as_dict()), st.graph.tobytes(), st.offsets)
    nbytes = len(st.graph)
    dg = torch.zeros(((nbytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device="cuda")         # readable up to nbytes rounded up to 16, + 16
    dg[:nbytes] = torch.from_numpy(np.ascontiguousarray(st.graph)).cuda()
    do = torch.from_numpy(st.offsets.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    g = W.BVGraph.from_device(st.params, dg.data_ptr(), nbytes, do.data_ptr(), keep=(dg,))
    if not wide_offsets:
        do.copy_(torch.flip(do, [0]))
        torch.cuda.synchronize()
    assert np.array_equal(g.offsets(), st.offsets)
    _check_graph(g, og, n, "open_dev, wide offsets %s" % wide_offsets)
    if wide_offsets:
        _check_graph(g, og, n, "open_dev, wide offsets, again")
        assert np.array_equal(do.cpu().numpy().view(np.uint64), st.offsets)    # used in place, never written
    g.close()


def _decode_range_dev_sizes(W, tools, oracle, torch):
    """cap = total, cap = total - 1 (BVG_E_CAPACITY, *n_succ = total) and d_succ = NULL (a size query), against the host decode_range; the guards behind
    cap (successors) and behind to - from (outdegrees) stay untouched in every case."""
    n = 30000
    st = tools.synth_store(n, seed=32, synth=tools.web_like(), threads=4)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    L = W.lib()
    for a, b in ((0, n), (0, 1), (4000, 4001), (n // 3, n // 3 + 5000), (n - 100, n), (123, 123 + n // 2)):
        hdeg, hsucc = g.decode_range(a, b)
        total, cnt = len(hsucc), b - a
        assert total > 0, (a, b)
        need = C.c_uint64(0)
        # cap = total
        d_deg, d_succ = _buf(torch, cnt, torch.int32), _buf(torch, total, torch.int64)
        torch.cuda.synchronize()
        assert L.bvg_decode_range_dev(g._h, a, b, d_deg.data_ptr(), d_succ.data_ptr(), total, C.byref(need)) == 0 and need.value == total, (a, b)
        assert np.array_equal(_host(torch, d_succ, total), hsucc) and np.array_equal(_host(torch, d_deg, cnt), hdeg), (a, b)
        assert _guard_ok(torch, d_succ, total) and _guard_ok(torch, d_deg, cnt), (a, b)
        # cap = total - 1
        d_deg, d_succ = _buf(torch, cnt, torch.int32), _buf(torch, total - 1, torch.int64)
        torch.cuda.synchronize()
        need.value = 0
        assert L.bvg_decode_range_dev(g._h, a, b, d_deg.data_ptr(), d_succ.data_ptr(), total - 1, C.byref(need)) == W.E_CAPACITY and need.value == total, (a, b)
        assert _guard_ok(torch, d_succ, total - 1) and _guard_ok(torch, d_deg, cnt), (a, b)
        # size query
        d_deg = _buf(torch, cnt, torch.int32)
        torch.cuda.synchronize()
        need.value = 0
        assert L.bvg_decode_range_dev(g._h, a, b, d_deg.data_ptr(), None, 0, C.byref(need)) == W.E_CAPACITY and need.value == total, (a, b)
        assert _guard_ok(torch, d_deg, cnt), (a, b)
    need = C.c_uint64(7)
    assert L.bvg_decode_range_dev(g._h, 5, 5, None, None, 0, C.byref(need)) == 0 and need.value == 0          # an empty range
    g.close()


def _cpu_transpose(n, deg, succ):
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    order = np.argsort(succ, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(succ, minlength=n))]).astype(np.uint64), src[order]


def _cpu_symmetrize(n, deg, succ):
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    keys = np.unique(np.concatenate([src * n + succ, succ * n + src]))
    s, t = keys // n, keys % n
    return np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))]).astype(np.uint64), t.astype(np.int64)


def _transpose_and_symmetrize_dev_on_cnr(W, tools, oracle, torch):
    """bvg_transpose_dev / bvg_symmetrize_dev on the reference's cnr-2000 against numpy (as the host calls are in test_gpu_api.py), with their
    capacity calls: a size query, one element short, exactly enough."""
    from conftest import CNR
    g = W.BVGraph.load(CNR)
    deg, succ = oracle.Graph.load(CNR).decode_range(0, g.num_nodes())
    n, L = g.num_nodes(), W.lib()
    ctoff, ctsucc = _cpu_transpose(n, deg, succ)
    need = C.c_uint64(0)
    d_off = _buf(torch, n + 1, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_transpose_dev(g._h, d_off.data_ptr(), None, 0, C.byref(need)) == W.E_CAPACITY and need.value == len(ctsucc)
    arcs = int(need.value)
    d_ts = _buf(torch, arcs - 1, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_transpose_dev(g._h, d_off.data_ptr(), d_ts.data_ptr(), arcs - 1, C.byref(need)) == W.E_CAPACITY and need.value == arcs
    assert _guard_ok(torch, d_ts, arcs - 1) and _guard_ok(torch, d_off, n + 1)
    d_ts = _buf(torch, arcs, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_transpose_dev(g._h, d_off.data_ptr(), d_ts.data_ptr(), arcs, C.byref(need)) == 0 and need.value == arcs
    assert np.array_equal(_host(torch, d_off, n + 1).view(np.uint64), ctoff) and np.array_equal(_host(torch, d_ts, arcs), ctsucc)
    assert _guard_ok(torch, d_ts, arcs) and _guard_ok(torch, d_off, n + 1)

    csoff, cssucc = _cpu_symmetrize(n, deg, succ)
    m = len(cssucc)
    d_off = _buf(torch, n + 1, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_symmetrize_dev(g._h, d_off.data_ptr(), None, 0, C.byref(need)) == W.E_CAPACITY and need.value == m
    assert np.array_equal(_host(torch, d_off, n + 1).view(np.uint64), csoff) and _guard_ok(torch, d_off, n + 1)       # the offsets come with the size query
    d_ss = _buf(torch, m - 1, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_symmetrize_dev(g._h, d_off.data_ptr(), d_ss.data_ptr(), m - 1, C.byref(need)) == W.E_CAPACITY and need.value == m
    assert _guard_ok(torch, d_ss, m - 1)
    d_off, d_ss = _buf(torch, n + 1, torch.int64), _buf(torch, m, torch.int64)
    torch.cuda.synchronize()
    assert L.bvg_symmetrize_dev(g._h, d_off.data_ptr(), d_ss.data_ptr(), m, C.byref(need)) == 0 and need.value == m
    assert np.array_equal(_host(torch, d_off, n + 1).view(np.uint64), csoff) and np.array_equal(_host(torch, d_ss, m), cssucc)
    assert _guard_ok(torch, d_ss, m) and _guard_ok(torch, d_off, n + 1)
    g.close()


def _labels_chained_on_decode_range_dev(W, tools, oracle, torch, kind, width):
    """bvg_labels_decode_range_dev takes the outdegrees bvg_decode_range_dev left in HBM, without a trip through the host: the labels equal the host
    call's; one label short is BVG_E_CAPACITY and leaves the guard alone."""
    from test_labels import _labelled
    n = 20000
    st, off, adj, vals, sl = _labelled(tools, n, 33, kind, width, synth=tools.eu_like() if kind == 1 else None)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    lg = W.BitStreamArcLabelledImmutableGraph.from_memory(g, kind, width, sl.stream, sl.offsets)
    L = W.lib()
    for a, b in ((0, n), (777, 778), (n // 4, n // 2), (n - 50, n)):
        hdeg, hsucc, hlab = lg.decode_range(a, b)
        total, cnt = len(hsucc), b - a
        need = C.c_uint64(0)
        d_deg, d_succ = _buf(torch, cnt, torch.int32), _buf(torch, total, torch.int64)
        torch.cuda.synchronize()
        assert L.bvg_decode_range_dev(g._h, a, b, d_deg.data_ptr(), d_succ.data_ptr(), total, C.byref(need)) == 0 and need.value == total, (a, b)
        d_lab = _buf(torch, total, torch.int32)
        torch.cuda.synchronize()
        assert L.bvg_labels_decode_range_dev(lg._h, a, b, d_deg.data_ptr(), d_lab.data_ptr(), total, C.byref(need)) == 0 and need.value == total, (a, b)
        assert np.array_equal(_host(torch, d_lab, total), hlab) and _guard_ok(torch, d_lab, total), (a, b)
        assert np.array_equal(_host(torch, d_succ, total), hsucc), (a, b)
        if total:
            d_lab = _buf(torch, total - 1, torch.int32)
            torch.cuda.synchronize()
            assert L.bvg_labels_decode_range_dev(lg._h, a, b, d_deg.data_ptr(), d_lab.data_ptr(), total - 1, C.byref(need)) == W.E_CAPACITY and need.value == total, (a, b)
            assert _guard_ok(torch, d_lab, total - 1), (a, b)
    lg.close(); g.close()


# ---- the tests: each body in a child process (see the module docstring) ----

def _in_child(name, *args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name] + [str(a) for a in args], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    if r.returncode == 77:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0, "child %s%r failed (rc %d):\n%s\n%s" % (name, args, r.returncode, r.stdout[-4000:], r.stderr[-6000:])


@pytest.mark.parametrize("wide_offsets", [False, True])
def test_open_from_device_memory(wide_offsets):
    _in_child("open_from_device_memory", int(wide_offsets), env={"BVG_WIDE_OFFSETS": "1"} if wide_offsets else {"BVG_WIDE_OFFSETS": ""})


def test_decode_range_dev_sizes():
    _in_child("decode_range_dev_sizes")


def test_transpose_and_symmetrize_dev_on_cnr():
    _in_child("transpose_and_symmetrize_dev_on_cnr")


@pytest.mark.parametrize("kind,width", [(1, 0), (2, 10)])
def test_labels_chained_on_decode_range_dev(kind, width):
    _in_child("labels_chained_on_decode_range_dev", kind, width)


if __name__ == "__main__":
    import torch                                                    # (first: see the module docstring)
    if not torch.cuda.is_available():
        print("the _dev entry points need torch on a GPU")
        sys.exit(77)
    if not os.environ.get("BVG_WIDE_OFFSETS"):
        os.environ.pop("BVG_WIDE_OFFSETS", None)
    from conftest import ROOT                                       # noqa: F401  (the repository on sys.path, BVG_TEST_KNOBS)
    import webgraph_big_amd as W
    import tooling as T
    from oracle import bvg_oracle as O
    T.lib(); O.lib()
    globals()["_" + sys.argv[1]](W, T, O, torch, *[int(a) for a in sys.argv[2:]])
    print("ok")
