"""GPU: scattered arc lists on the device (bvg_scattered_*): arc lists whose identifiers are arbitrary 64-bit integers.  Every case is held
against the plain-Python model of the contract (tests/scattered_model.py, itself checked against the reference's expectations in
tests/test_scattered_model.py): the ids, the CSR and the whole report; refusals as the whole record (status, line, byte, reason)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import scattered_model as M
from scattered_cases import REFERENCE_CASES

pytestmark = pytest.mark.gpu

EMPTY_MARKER = -1                       # the identifier that the table keeps outside its slots (csrc/bvg_scattered.hip: kEmptyKey)
SPECIAL = tuple(dict.fromkeys((0, -1, M.INT64_MIN, M.INT64_MAX, EMPTY_MARKER)))


def same(W, text, symmetrize=False, no_loops=False, ids=None, parse=None):
    """Parses on the device and with the model; everything observable agrees.  Returns the model's answer."""
    want = M.parse(text, symmetrize, no_loops, ids)
    with (parse or W.parse_scattered_arcs)(text, symmetrize=symmetrize, no_loops=no_loops, ids=ids) as g:
        off, adj = g.csr()
        woff, wadj = M.csr(want["nodes"], want["arcs"])
        assert g.num_nodes() == want["nodes"] and g.ids.tolist() == want["ids"]
        assert g.num_arcs() == len(want["arcs"]) and np.array_equal(off, woff) and np.array_equal(adj, wadj)
        assert g.report == want["report"]
    return want


def refusal(W, text, **kw):
    try:
        W.parse_scattered_arcs(text, strict=True, **kw).close()
    except W.BVGraphError as e:
        return (e.status, e.line, e.byte, e.reason)
    return None


def lines(pairs, sep=b" ", end=b"\n"):
    return b"".join(b"%d%s%d%s" % (s, sep, t, end) for s, t in pairs)


# ---- the reference's cases

@pytest.mark.parametrize("case", range(len(REFERENCE_CASES)))
def test_reference_cases(W, case):
    text, sym, nol, arcs, ids = REFERENCE_CASES[case]
    want = same(W, text, sym, nol)
    assert (want["ids"], want["arcs"]) == (ids, sorted(arcs))


# ---- token grammar, line ends, skipped lines

TOKENS = [b"-", b"-0", b"+1", b"--1", b"1-", b"1x", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809",
          b"1234567890123456789012345", b"12345678901234567890x", b"1234567890123456789x", b"0" * 30 + b"5", b"caf\xc3\xa9", b"1\x80", b"\xff", b"#1", b"1#"]


def test_token_grammar(W):
    for tok in TOKENS:
        for text in (tok + b" 1\n", b"1 " + tok + b"\n", b"3 4\n" + tok + b"\t" + tok, tok):
            same(W, text)
    same(W, b"\n".join(a + b" " + b for a in TOKENS for b in TOKENS))
    same(W, b"1\x002\n3\x0b4\n5\x1f6\x01\x02 7\n\x00\n 8 \x0c 9 \n")               # NUL, VT and their kin are whitespace


def test_line_ends_and_skipped_lines(W):
    same(W, b"1 2\r3 4\n5 6\r\n7 8\n\r9 10\r\r11 12\n\n13 14\r\n\r\n15 16")
    same(W, b"#a\n1 2\r#b 3 4\r\n#c 5 6\n\n#\r\r# 7 8\r\n1 3")                         # a '#' behind each kind of break
    same(W, b" #x 1\n\t# 2 3\n1 #\n# 1 2")                                           # only the very first byte of a line opens a comment
    same(W, b"1 2\n3 4")                                                              # a last line without a break
    same(W, b"1 2\n3")
    same(W, b"")
    same(W, b"\n")
    same(W, b"\r\n")
    same(W, b"# only\n# comments\r# here")
    same(W, b"   \n\t\t\n \r\n")


@pytest.mark.parametrize("v", SPECIAL)
def test_special_identifier_values(W, v):
    same(W, b"%d %d\n" % (v, v))                                                      # the only identifier
    same(W, b"%d\n" % v)
    same(W, b"%d 5\n6 7\n7 %d\n" % (v, v))                                            # first
    same(W, b"5 6\n%d 7\n7 %d\n8 9\n" % (v, v))                                       # in the middle
    same(W, b"5 6\n6 %d\n" % v, symmetrize=True)
    same(W, b"5 %d\n%d %d\n%d 5\n" % (v, v, v, v), no_loops=True)
    same(W, lines([(a, b) for a in SPECIAL for b in SPECIAL]) + b"%d %d\n" % (v, v))  # all of them together


def test_registration_rules(W):
    for text in (b"7\n", b"7 X\n", b"X 9\n", b"X 9\n9 1\n", b"5 5\n", b"7 8 9\n", b"7 8 X\n", b"7 X 9\n", b"1 2 3 4 5 6 7 8 9\n2 1\n"):
        for nol in (False, True):
            same(W, text, no_loops=nol)
    with W.parse_scattered_arcs(b"X 9\n") as g:
        assert g.num_nodes() == 0 and g.report["bad_source"] == 1                    # 9 is no node
    with W.parse_scattered_arcs(b"5 5\n", no_loops=True) as g:
        assert (g.num_nodes(), g.num_arcs(), g.ids.tolist(), g.report["dropped_loops"]) == (1, 0, [5], 1)


# ---- the seams of the tiling

def padded(n, tail=b"77 88\n"):
    """A text of exactly n bytes: arcs over a few identifiers, blanks, then `tail`."""
    body = lines([(i % 7 - 3, i % 5) for i in range(n // 5)])[:n - len(tail)]
    body = body[:body.rfind(b"\n") + 1]
    return body + b" " * (n - len(tail) - len(body)) + tail


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192, 12289])
def test_text_sizes_around_the_tile(W, n):
    text = padded(n)
    assert len(text) == n
    same(W, text)
    same(W, text[:-1])                                                                # ... without the last break


@pytest.mark.parametrize("at", [16, 32, 4096, 8192, 4096 + 16])
def test_things_that_straddle_a_boundary(W, at):
    for piece, inside in ((b"-123456789 987654321", 5), (b"12 34\n56 78", 5), (b"12 34\r\n56 78", 6), (b"12 34\r\n#6 78\n1 2", 7), (b"1 2\n#", 4)):
        head = lines([(i % 9, -(i % 4)) for i in range(at // 4)])
        head = head[:head[:at - inside].rfind(b"\n") + 1]
        text = head + b" " * (at - inside - len(head)) + piece + b"\n9 9\n"            # byte `inside` of the piece is byte `at` of the text
        same(W, text)
        same(W, text, symmetrize=True, no_loops=True)


def test_long_comment_then_an_arc(W):
    same(W, b"1 2\n#" + b"x 3 4 " * 1500 + b"\n5 6\n")                                # a comment line longer than two tiles
    same(W, b"#" + b"y" * 9000 + b"\r\n5 6\n7")
    same(W, b"1 " + b"2" * 9000 + b"\n5 6\n")                                          # ... and a token as long


class DeviceBytes:
    """A device buffer through the HIP runtime the library itself is linked against."""
    hip = None

    def __init__(self, data, lead=0):
        if DeviceBytes.hip is None:
            DeviceBytes.hip = C.CDLL("libamdhip64.so")
            DeviceBytes.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            DeviceBytes.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            DeviceBytes.hip.hipFree.argtypes = [C.c_void_p]
        self.host = np.frombuffer(b"\n" * lead + bytes(data), dtype=np.uint8).copy()
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(len(self.host), 1)) == 0
        self.base, self.ptr = p.value, p.value + lead
        assert self.hip.hipMemcpy(self.base, self.host.ctypes.data, len(self.host), 1) == 0

    def get(self):
        assert self.hip.hipMemcpy(self.host.ctypes.data, self.base, len(self.host), 2) == 0
        return self.host

    def free(self):
        self.hip.hipFree(self.base)


@pytest.mark.parametrize("lead", [0, 1, 7])
def test_device_forms(W, lead):
    """Text, given numbering and ids in device memory; a text pointer that is not 16-byte aligned takes Chunk::load's other path."""
    text = padded(9000) + b"X 1\n-5 6 7\n1 500\n"
    known = np.array([-3, 0, 1, 2, 3, 4, 77, 88, -1, -2, 1 << 40], dtype=np.int64)
    d_text, d_known = DeviceBytes(text, lead), DeviceBytes(known.tobytes())
    try:
        same(W, text, parse=lambda t, symmetrize, no_loops, ids: W.parse_scattered_arcs_dev(d_text.ptr, len(text), symmetrize, no_loops))
        want = same(W, text, True, True, ids=known.tolist(),
                    parse=lambda t, symmetrize, no_loops, ids: W.parse_scattered_arcs_dev(d_text.ptr, len(text), symmetrize, no_loops, d_known.ptr, len(known)))
        assert want["report"]["unknown_source"] and want["report"]["unknown_target"]
        L = W.textgraph._scattered_fns()
        with W.parse_scattered_arcs_dev(d_text.ptr, len(text)) as g:
            n = g.num_nodes()
            d_ids = DeviceBytes(np.zeros(n + 1, dtype=np.int64).tobytes())
            try:
                assert L.bvg_scattered_ids_dev(g._h, d_ids.ptr, n - 1) == W.E_CAPACITY and not d_ids.get().any()      # nothing is written
                assert L.bvg_scattered_ids(g._h, d_ids.host.ctypes.data, n - 1) == W.E_CAPACITY
                g.ids_dev(d_ids.ptr, n)
                assert np.array_equal(d_ids.get().view(np.int64)[:n], g.ids)
            finally:
                d_ids.free()
    finally:
        d_text.free(); d_known.free()
    with W.parse_arc_list(b"0 1\n") as plain:                                         # every other producer's handle has no ids
        assert L.bvg_scattered_ids(plain._h, None, 0) == W.E_UNSUPPORTED


# ---- the table

def occurrences_text(rng, distinct, occurrences, pool):
    """`occurrences` identifier occurrences (two a line) over exactly `distinct` identifiers of `pool`."""
    ids = pool[:distinct]
    seq = np.concatenate([ids, ids[rng.integers(0, distinct, occurrences - distinct)]]) if occurrences > distinct else ids
    seq = seq[rng.permutation(len(seq))]
    if len(seq) % 2:
        seq = np.concatenate([seq, seq[:1]])
    return lines(zip(seq[0::2].tolist(), seq[1::2].tolist()))


@pytest.mark.parametrize("distinct", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025])
def test_distinct_counts(W, distinct):
    rng = np.random.default_rng(distinct)
    pools = (np.arange(distinct, dtype=np.int64) + 1000,                              # consecutive
             np.arange(distinct, dtype=np.int64) << 20,                               # multiples of 2^20
             rng.integers(-(1 << 62), 1 << 62, distinct * 2, dtype=np.int64))         # random 63-bit
    for pool in pools:
        pool = np.unique(pool)[:distinct][rng.permutation(distinct)]
        want = same(W, occurrences_text(rng, distinct, max(distinct + 3, 2 * distinct), pool))
        assert want["nodes"] == distinct


def test_load_close_to_the_bound(W):
    rng = np.random.default_rng(3000)
    pool = np.unique(rng.integers(-(1 << 62), 1 << 62, 4000, dtype=np.int64))[:3000]
    want = same(W, occurrences_text(rng, 3000, 4000, pool[rng.permutation(3000)]))
    assert want["nodes"] == 3000 and want["report"]["arcs"] == 2000


def test_hubs_and_orders(W):
    n = 50000
    same(W, lines((12345678901, i) for i in range(n)))                               # one hub as the source of every line
    same(W, lines((i, -77) for i in range(n)))                                       # ... as the target
    same(W, lines((-1, -1) for i in range(n)), no_loops=False)                       # ... the identifier outside the table, both ends
    same(W, b"5 999\n" + lines((i, i + 1) for i in range(10, 400)) + lines((999, i % 50) for i in range(20000)))   # first seen as a target, then a source thousands of times
    same(W, lines((i, i - 1) for i in range(30000, 0, -3)))                          # decreasing: order of appearance against numeric order
    same(W, lines((i // 3, (i * 7919) % 1000) for i in range(70000)), symmetrize=True)   # 70 000 lines: every level of the prefix sums


# ---- switches, duplicates, strict

@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("nol", [False, True])
def test_switches(W, sym, nol):
    rng = np.random.default_rng(5)
    ids = rng.integers(-40, 40, (3000, 2))
    want = same(W, lines(ids.tolist()) + b"7 7\n7 7\n-9 -9 x\n", sym, nol)            # duplicates and loops galore
    assert want["report"]["dropped_loops"] > 0 if nol else want["report"]["dropped_loops"] == 0


def test_strict(W):
    clean = b"# c\n-1 15\n\n15 2 \r\n2 -1\r"
    assert refusal(W, clean) is None
    assert refusal(W, clean + b"1 2 trailing\n") is None                             # TRAILING is a warning
    head = clean + b"\n"
    at, ln = len(head), 6
    for bad, reason, shift in ((b"X 1", "bad_source", 0), (b" 1 X", "bad_target", 3), (b"7", "no_target", 0), (b"\t7 \t", "no_target", 1),
                               (b"9223372036854775808 1", "too_large", 0), (b"1 -9223372036854775809", "too_large", 2), (b"+1 +2", "bad_source", 0)):
        for tail in (b"", b"\n", b"\n3 4\nY Y\n"):
            text = head + bad + tail
            assert refusal(W, text) == (W.E_IO, ln, at + shift, reason), (bad, tail)
            want = M.parse(text)["report"]
            assert (want["first_line"], want["first_byte"], want["first_reason"]) == (ln, at + shift, reason)
    known = [-1, 15, 2]
    assert refusal(W, clean, ids=known) is None
    assert refusal(W, head + b"15 3\n3 15\n", ids=known) == (W.E_IO, ln, at + 3, "unknown_target")
    assert refusal(W, head + b"3 15\n15 3\n", ids=known) == (W.E_IO, ln, at, "unknown_source")
    assert refusal(W, head + b"3 4\n", ids=known) == (W.E_IO, ln, at, "unknown_source")
    try:
        W.parse_scattered_arcs(head + b"X 1\n", strict=True)
        assert False
    except W.IOException as e:
        assert e.report == M.parse(head + b"X 1\n")["report"]                         # the report is filled all the same


# ---- given numbering

def test_given_numbering(W):
    text = b"2 -1\n3 2\n2 3\n7\n-1 -1 x\n40 2\n3 3\n"
    want = same(W, text, ids=[2, -1, 7, 40, 1000])                                    # 7 and 1000: isolated nodes
    assert want["nodes"] == 5 and want["report"]["unknown_source"] == 2 and want["report"]["unknown_target"] == 1
    same(W, text, True, True, ids=[2, -1, 7, 40, 1000])
    same(W, text, ids=[])                                                             # nobody is known
    same(W, text, ids=[5, 6])
    same(W, b"", ids=[5, 6])
    for v in SPECIAL:
        same(W, b"%d 1\n1 %d\n%d %d\n" % (v, v, v, v), ids=[1, v] if v != 1 else [1])
        same(W, b"%d 1\n1 %d\n" % (v, v), ids=[1, 2, 3])
    for dup in ([1, 2, 1], [-1, 3, -1], [0, 0], list(range(500)) + [77]):
        with pytest.raises(W.IllegalArgumentException):
            W.parse_scattered_arcs(text, ids=dup)


def test_second_file_in_the_numbering_of_the_first(W):
    rng = np.random.default_rng(11)
    pool = rng.integers(-(1 << 62), 1 << 62, 300, dtype=np.int64)
    first = lines(pool[rng.integers(0, 250, (2000, 2))].tolist())
    second = lines(pool[rng.integers(100, 300, (2000, 2))].tolist())                  # a later snapshot: some identifiers are new
    with W.parse_scattered_arcs(first) as g:
        ids = g.ids.copy()
    want = same(W, second, ids=ids.tolist())
    assert want["nodes"] == len(ids) and want["report"]["unknown_source"] and want["report"]["arcs"]


# ---- cross-checks with what exists

def test_identity_numbering_is_parse_arc_list(W):
    rng = np.random.default_rng(2)
    src = np.sort(rng.integers(0, 2000, 20000))
    dst = rng.integers(0, 2000, 20000)
    order = np.concatenate([np.stack([np.arange(2000), np.arange(2000)], 1), np.stack([src, dst], 1)])   # x x first: the ids appear as 0, 1, 2, ...
    text = lines(order.tolist(), sep=b"\t")
    for sym in (False, True):
        for nol in (False, True):
            with W.parse_scattered_arcs(text, sym, nol) as a, W.parse_arc_list(text, symmetrize=sym, no_loops=nol) as b:
                assert np.array_equal(a.ids, np.arange(2000))
                for x, y in zip(a.csr(), b.csr()):
                    assert np.array_equal(x, y)


def test_cnr_slice_through_a_random_injection(W, cnr_golden, oracle):
    rows = 30000                                                                      # ~ 300 000 arcs
    lists = cnr_golden[:rows]
    deg = np.array([len(l) for l in lists])
    src, dst = np.repeat(np.arange(rows), deg), np.concatenate(lists)
    nodes = np.unique(np.concatenate([src, dst]))
    rng = np.random.default_rng(2000)
    code = np.unique(rng.integers(-(1 << 61), 1 << 61, 2 * len(nodes), dtype=np.int64))[:len(nodes)][rng.permutation(len(nodes))]   # an injection into 62-bit values
    s, t = code[np.searchsorted(nodes, src)], code[np.searchsorted(nodes, dst)]
    order = rng.permutation(len(s))
    text = lines(zip(s[order].tolist(), t[order].tolist()), sep=b"\t")
    with W.parse_scattered_arcs(text) as g:
        assert g.num_nodes() == len(nodes) and g.num_arcs() == len(src) and g.report["arcs"] == len(src)
        off, adj = g.csr()
        ids = g.ids
        by_code = np.argsort(code)
        back = nodes[by_code[np.searchsorted(code[by_code], ids)]]                    # golden node of every new node
        gsrc, gdst = back[np.repeat(np.arange(len(ids)), np.diff(off.astype(np.int64)))], back[adj]
        o = np.lexsort((gdst, gsrc))
        assert np.array_equal(gsrc[o], src) and np.array_equal(gdst[o], dst)          # rows permuted back: the golden rows
        graph, offsets = g.store()
    p = W.default_params(nodes=len(ids), arcs=len(adj))
    og = oracle.Graph.from_memory(oracle.Params(**p.as_dict()), graph.tobytes(), offsets)
    odeg, osucc = og.decode_range(0, len(ids))
    assert np.array_equal(odeg, np.diff(off.astype(np.int64))) and np.array_equal(osucc, adj)


# ---- files and the command line

def test_files_and_command_line(W, tmp_path, capsys):
    text = b"# My graph\n-1 15\n15 2\n2 -1 warning\nOOPS! error\n-1 2\n900 -1\n"
    want = M.parse(text)
    path = str(tmp_path / "example.arcs.gz")
    with gzip.open(path, "wb") as f:
        f.write(text)
    with W.load_scattered_arcs(path, symmetrize=True) as g:
        assert g.ids.tolist() == want["ids"] and g.num_arcs() == len(M.parse(text, True)["arcs"])
    with pytest.raises(W.IOException):
        W.load_scattered_arcs(str(tmp_path / "none"))
    base = str(tmp_path / "example")
    assert W.scattered_main(["--input", path, "-w", "3", base]) == 0
    err = capsys.readouterr().err
    assert "7 lines, 5 arcs kept, 4 nodes" in err and "bad source: 1 lines" in err and "trailing: 1 lines" in err and "line 5" in err
    ids = W.load_longs(base + ".ids")
    assert ids.tolist() == want["ids"]
    bv = W.BVGraph.load(base)
    try:
        assert bv.params.window_size == 3 and bv.num_nodes() == 4
        deg, succ = bv.decode_range(0, 4)
        got = sorted(zip(ids[np.repeat(np.arange(4), deg)].tolist(), ids[succ].tolist()))
    finally:
        bv.close()
    assert got == sorted({(-1, 15), (15, 2), (2, -1), (-1, 2), (900, -1)})               # the successors mapped through .ids: the text's arcs
    # a second file in the numbering of the first; -z on a gzipped file without the suffix
    second = str(tmp_path / "second.bin")
    with open(second, "wb") as f:
        f.write(gzip.compress(b"15 -1\n2 2\n900 901\n"))
    base2 = str(tmp_path / "second")
    assert W.scattered_main(["-z", "-L", "--ids", base + ".ids", "--input", second, base2]) == 0
    assert "unknown target: 1 lines" in capsys.readouterr().err and not os.path.exists(base2 + ".ids")
    bv = W.BVGraph.load(base2)
    try:
        deg, succ = bv.decode_range(0, bv.num_nodes())
        assert bv.num_nodes() == 4 and deg.tolist() == [0, 1, 0, 0] and succ.tolist() == [0]
    finally:
        bv.close()
    with pytest.raises(W.IOException):
        W.scattered_main(["--strict", "--input", path, base])
