"""Test helper of tests/test_gpu_derive.py and tests/test_gpu_derive_fuzz.py: one derivation of the offsets index (bvg_open_mem with
offsets = NULL: csrc/bvg_derive.hip, csrc/bvg_derive_seq.hip) on BOTH walks, each checked against the two CPU restatements -- the offsets
the writer of the stream recorded (the encoder's, or tests/bvrecords.py's) and the oracle's own derivation (oracle/bvg_oracle.c,
bvgo_write_offsets: BVGraph.writeOffsets, BVGraph.java:2595-2609).  The two walks are never compared with each other alone: both are code
under test."""
import numpy as np

CHUNK_BITS = 32768            # kChunkBits of csrc/bvg_derive.hip: 4 KiB of stream per walk
MAX_PARALLEL_WINDOW = 127     # kMaxDeriveWindow
MAX_WINDOW = 2048 - 64        # kMaxWindowBig of csrc/bvg_kernels.h (kRingBig - 64)

# BVG_DERIVE_WARM / BVG_DERIVE_CRAWL (csrc/bvg_derive.hip): with no warm-up every chunk starts from the raw guess, so detect / adopt settle
# most of the chunks; crawl 0 sends every later round to derive_round_kernel over the list, a huge value to derive_crawl_kernel
ROUTES = {
    "default": {},
    "warm0": dict(BVG_DERIVE_WARM="0"),
    "warm0_list": dict(BVG_DERIVE_WARM="0", BVG_DERIVE_CRAWL="0"),
    "warm0_crawl": dict(BVG_DERIVE_WARM="0", BVG_DERIVE_CRAWL="1000000000"),
}


LAST = {"err": "", "route": "default"}     # stderr of the last open_on(), the route set_route() chose


def chunks_of(graph):
    return max(1, (len(graph) * 8 + CHUNK_BITS - 1) // CHUNK_BITS)


def set_route(monkeypatch, route):
    for k in ("BVG_DERIVE_WARM", "BVG_DERIVE_CRAWL", "BVG_DERIVE_SEQ"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    LAST["route"] = route


def open_on(W, capfd, monkeypatch, p, graph, walk):
    """bvg_open_mem without offsets on one walk ("parallel": the default path; "seq": BVG_DERIVE_SEQ=1).  Returns (handle or None, status
    exception class or None, "parallel" / "fallback" as the BVG_DEBUG line of bvg_plan.hip says, rounds)."""
    monkeypatch.setenv("BVG_DEBUG", "1")
    if walk == "seq":
        monkeypatch.setenv("BVG_DERIVE_SEQ", "1")
    else:
        monkeypatch.delenv("BVG_DERIVE_SEQ", raising=False)
    capfd.readouterr()
    g, exc = None, None
    try:
        g = W.BVGraph.from_memory(p, graph, None)
    except W.BVGraphError as e:
        exc = type(e)
    err = capfd.readouterr().err
    LAST["err"] = err
    monkeypatch.delenv("BVG_DERIVE_SEQ", raising=False)
    lines = [l for l in err.splitlines() if "derive offsets: parallel walk" in l]
    assert len(lines) == 1, err[-2000:]
    used = "parallel" if "parallel walk ok" in lines[0] else "fallback"
    assert used == "parallel" or "not used / failed" in lines[0], lines[0]
    rounds = int(lines[0].split("(")[1].split(" rounds")[0])
    return g, exc, used, rounds


def oracle_offsets(oracle, p, graph):
    og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), bytes(graph), None)
    return og.derive_offsets()


def check_derivation(W, oracle, capfd, monkeypatch, p, graph, want, expect="parallel", scan=True, what=None):
    """Both walks derive `want` (nodes + 1 offsets of the stream's writer), which the oracle's derivation must give too; the default path
    used the walk `expect` ("parallel": a silent fall-back fails; "fallback"), in at most chunks + 1 rounds (after round r the chunks 0..r are
    exact: the induction of bvg_derive.hip's header); one scan on the derived index equals the oracle's.  Returns the rounds of the
    parallel walk."""
    graph = np.ascontiguousarray(graph, dtype=np.uint8)
    want = np.ascontiguousarray(want, dtype=np.uint64)
    n = int(p.nodes)
    assert len(want) == n + 1
    ours = oracle_offsets(oracle, p, graph)
    assert np.array_equal(ours, want), ("the oracle's derivation differs from the writer's offsets", what)
    oscan = None
    rounds_par = 0
    for walk in ("parallel", "seq"):
        g, exc, used, rounds = open_on(W, capfd, monkeypatch, p, graph, walk)
        assert exc is None, (what, walk, exc)
        try:
            assert used == (expect if walk == "parallel" else "fallback"), (what, walk, used)
            if used == "parallel":
                assert 1 <= rounds <= chunks_of(graph) + 1, (what, rounds, chunks_of(graph))
                rounds_par = rounds
                check_route(want, rounds, chunks_of(graph), what)
            got = g.offsets()
            assert np.array_equal(got, want), (what, walk, "offsets differ from node %d on" % int(np.argmax(got != want)))
            if scan:
                if oscan is None:
                    oscan = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), want).scan()
                r = g.scan()
                assert (r["nodes"], r["arcs"], r["chk"]) == (oscan["nodes"], oscan["arcs"], oscan["chk"]), (what, walk)
        finally:
            g.close()
    return rounds_par


def check_route(want, rounds, chunks, what):
    """The knobs of the route took effect, from the BVG_DEBUG lines of the rounds (csrc/bvg_derive.hip names the kernel and the warm-up of
    every later round).  Without warm-up chunk 1 enters in the guess "a record starts on my first bit, the window is empty": where no
    record starts on the first chunk boundary that guess is wrong, so there is a second round."""
    route = LAST["route"]
    later = [l for l in LAST["err"].splitlines() if "] derive round " in l]
    assert (rounds >= 2) == bool(later), (what, rounds, later)
    if route != "default" and chunks >= 2 and CHUNK_BITS not in set(int(v) for v in want):
        assert rounds >= 2, (what, route, "no second round without warm-up")
    for l in later:
        assert ("(warm-up 8 chunks)" if route == "default" else "(warm-up 0 chunks)") in l, (what, route, l)
        if route == "warm0_list": assert "by the list kernel" in l, (what, l)
        if route in ("warm0_crawl", "warm0", "default") and chunks <= 2048: assert "by the crawl kernel" in l, (what, l)


def with_empty_nodes(off, adj, lead, trail):
    """The adjacency with `lead` empty nodes in front (every id moves up by lead) and `trail` behind: records are translation invariant,
    so the stream is `lead` one-bits (gamma(0)) in front of the same bits, and `trail` more behind."""
    off = np.asarray(off, dtype=np.uint64)
    o = np.concatenate([np.zeros(lead, np.uint64), off, np.full(trail, off[-1], np.uint64)])
    return o, np.asarray(adj, dtype=np.int64) + lead


def golomb_bound_ok(off, adj, m):
    """Golomb residuals (modulus m in zeta_k) are decoded by the device from one 64-bit window with a unary quotient below 40
    (csrc/bvg_lds_codes.h, decode_generic_w): every coded value v must have v // m <= 39 (the code then has at most 40 + bit_length(m)
    <= 64 bits for m < 2^24).  A coded value is at most max(2 |s - x| + 1 over the successors s of x, max(list) - min(list)): the first residual is the signed distance to x
    (BVG:917), a later one the gap to the residual before it (BVG:929), and residuals are elements of the list."""
    off = np.asarray(off, dtype=np.int64); adj = np.asarray(adj, dtype=np.int64)
    n = len(off) - 1
    if len(adj) == 0:
        return True
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    v = int((2 * np.abs(adj - src) + 1).max())
    nz = np.flatnonzero(np.diff(off) > 0)
    v = max(v, int((adj[off[nz + 1] - 1] - adj[off[nz]]).max()))
    return v // m <= 39 and int(m) < (1 << 24)


def local_adjacency(rng, n, reach=20, deg=6):
    """Lists within `reach` of their node (what Golomb residuals need), one in three a copy of most of the list before."""
    lists = []
    for x in range(n):
        lo, hi = max(0, x - reach), min(n, x + reach + 1)
        k = int(rng.integers(0, deg + 1))
        l = np.unique(rng.integers(lo, hi, k)) if k else np.empty(0, np.int64)
        if lists and rng.random() < 0.3 and lists[-1].size:
            prev = lists[-1]; keep = prev[(prev >= lo) & (prev < hi) & (rng.random(prev.size) < 0.7)]
            l = np.union1d(keep, l[:2])
        lists.append(l.astype(np.int64))
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum([l.size for l in lists])
    return off, (np.concatenate(lists) if off[-1] else np.empty(0, np.int64))
