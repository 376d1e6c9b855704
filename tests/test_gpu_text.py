"""GPU: text graphs on the device (bvg_text_*): ASCIIGraph and arc lists, both ways.  The fixture is the yardstick -- the golden
cnr-2000.graph-txt is what ASCIIGraph.store writes and cnr-2000.graph what BVGraph.store writes -- everything else is held against the
plain-Python model (tests/textgraph_model.py), refusals as the whole record (status, line, byte, reason)."""
import ctypes as C
import gzip

import numpy as np
import pytest

import textgraph_model as M
from conftest import CNR

pytestmark = pytest.mark.gpu

N_CNR = 325557


@pytest.fixture(scope="module")
def golden_text():
    with gzip.open(CNR + ".graph-txt.gz", "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def cnr(W):
    g = W.BVGraph.load(CNR)
    yield g
    g.close()


@pytest.fixture(scope="module")
def line_starts(golden_text):
    """Byte offset of the line of every node in the golden text (and of its end)."""
    nl = np.flatnonzero(np.frombuffer(golden_text, dtype=np.uint8) == 10)
    return nl[:N_CNR + 1] + 1


def lib_record(call, *a, **kw):
    """What the library makes of a text: (nodes, adj_off, adj) or the refusal record."""
    import webgraph_big_amd as W
    try:
        g = call(*a, **kw)
    except W.BVGraphError as e:
        return (e.status, e.line, e.byte, e.reason)
    with g:
        off, adj = g.csr()
        assert len(off) == g.num_nodes() + 1 and len(adj) == g.num_arcs() == int(off[-1])
        return (g.num_nodes(), off.tolist(), adj.tolist())


def model_record(call, *a, **kw):
    try:
        n, off, adj = call(*a, **kw)
    except M.Refusal as e:
        return e.record()
    return (n, off.tolist(), adj.tolist())


def same_ascii(W, text):
    got, want = lib_record(W.parse_ascii_graph, text), model_record(M.parse_ascii, text)
    assert got == want, (text[:80], got if len(got) == 4 else got[0], want if len(want) == 4 else want[0])
    return got


def same_arcs(W, text, **kw):
    got, want = lib_record(W.parse_arc_list, text, **kw), model_record(M.parse_arcs, text, **kw)
    assert got == want, (text[:80], kw, got if len(got) == 4 else got[0], want if len(want) == 4 else want[0])
    return got


# ---- the fixture

def test_fixture_export_whole_and_by_arc_ranges(W, cnr, golden_text, tmp_path):
    assert len(golden_text) == 22248688
    assert b"%d\n" % N_CNR + cnr.format_ascii(0, N_CNR) == golden_text
    for ranges in (None, 5):                                                  # the file writer: one range, and bvg_split_by_arcs(5)
        path = cnr.to_ascii_graph(str(tmp_path / ("cnr%s" % ranges)), ranges=ranges)
        assert open(path, "rb").read() == golden_text
    b = cnr.split_by_arcs(5)
    assert len(set(b.tolist())) == 6                                          # five ranges that are not empty


def test_fixture_export_in_small_ranges(cnr, golden_text, line_starts, cnr_csr):
    """Ranges of 1 node and of 7 nodes.  A call costs a few hundred microseconds, so not all 325 557 nodes go one by one: the first and the
    last 100 nodes do (the edges of the graph), then 600 nodes and 600 windows of 7 drawn with a fixed seed over the whole id range, and the
    30 nodes of largest outdegree, each alone and inside a window of 7; each piece must be the golden's bytes of exactly those lines."""
    def golden(lo, hi):
        return golden_text[int(line_starts[lo]):int(line_starts[hi])]
    rng = np.random.default_rng(325557)
    big = np.argsort(cnr_csr[0])[-30:].tolist()
    assert cnr_csr[0][big[-1]] > 1000
    singles = list(range(100)) + list(range(N_CNR - 100, N_CNR)) + rng.integers(0, N_CNR, size=600).tolist() + big
    for x in singles:
        assert cnr.format_ascii(x, x + 1) == golden(x, x + 1), x
    sevens = [0, N_CNR - 7] + rng.integers(0, N_CNR - 6, size=600).tolist() + [max(0, min(x - 3, N_CNR - 7)) for x in big]
    for x in sevens:
        assert cnr.format_ascii(x, x + 7) == golden(x, x + 7), x
    whole = b"".join(cnr.format_ascii(x, min(x + 7, N_CNR)) for x in range(150000, 157000, 7))      # consecutive windows: the pieces abut
    assert whole == golden(150000, 157000)
    assert cnr.format_ascii(5, 5) == b"" and cnr.format_arcs(N_CNR, N_CNR) == b""


def test_fixture_import_reproduces_the_stored_graph(W, golden_text):
    with W.parse_ascii_graph(golden_text) as pg:
        assert (pg.num_nodes(), pg.num_arcs()) == (N_CNR, 3216152)
        p = W.default_params(window_size=7, max_ref_count=3, min_interval_length=3, zeta_k=3)
        graph, offsets = pg.store(p, 0)
    assert graph.tobytes() == open(CNR + ".graph", "rb").read()
    assert np.array_equal(offsets, W.decode_offsets(open(CNR + ".offsets", "rb").read(), N_CNR))
    assert W.coded_gaps(offsets, W.GAMMA) == open(CNR + ".offsets", "rb").read()


def test_fixture_arc_list_round_trip_shuffled(W, cnr, cnr_csr):
    deg, succ = cnr_csr
    text = cnr.format_arcs(0, N_CNR)
    assert text.startswith(b"0\t1\n0\t342\n") and text.count(b"\n") == len(succ)
    lines = np.array(text.split(b"\n")[:-1], dtype=object)
    shuffled = b"\n".join(lines[np.random.default_rng(2000).permutation(len(lines))].tolist()) + b"\n"
    with W.parse_arc_list(shuffled) as pg:
        off, adj = pg.csr()
    assert np.array_equal(adj, succ) and np.array_equal(np.diff(off.astype(np.int64)), deg)


# ---- numbers

NUMBERS = sorted(set([0, 9, 10] + [10 ** k - 1 for k in range(1, 19)] + [10 ** k for k in range(1, 19)]
                     + [2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 53 + 1, 2 ** 63 - 1]))


def test_numbers_format(W):
    """Every digit count and its neighbours, the 32-bit and double edges and 2^63 - 1, as successors and (shifted) as sources."""
    off = np.array([0, len(NUMBERS), len(NUMBERS), len(NUMBERS) + 2], dtype=np.uint64)
    adj = np.array(NUMBERS + [0, 2 ** 63 - 1], dtype=np.int64)
    lists = M.lists_of(off, adj)
    assert W.format_csr(W.TEXT_ASCII, 0, off, adj) == M.format_ascii(lists)
    for first in (0, 9, 10 ** 18 - 2, 2 ** 63 - 4):
        assert W.format_csr(W.TEXT_ARCS, first, off, adj) == M.format_arcs(lists, first)
    small = np.array(NUMBERS[:-1], dtype=np.int64)
    off1 = np.array([0, len(small)], dtype=np.uint64)
    for shift in (1, -0, 7):
        assert W.format_csr(W.TEXT_ARCS, 3, off1, small, shift) == M.format_arcs([small.tolist()], 3, shift)
    assert W.format_csr(W.TEXT_ARCS, 3, off1, small + 1, -1) == M.format_arcs([(small + 1).tolist()], 3, -1)
    for bad_adj, shift in (([2 ** 63 - 1], 1), ([0], -4), ([-1], 0)):         # leaves [0, 2^63 - 1]
        with pytest.raises(W.IllegalArgumentException):
            W.format_csr(W.TEXT_ARCS, 3, [0, 1], bad_adj, shift)
    with pytest.raises(W.IllegalArgumentException):
        W.format_csr(W.TEXT_ASCII, 0, [0, 1], [-5])


def test_numbers_parse(W):
    """Accepted or refused, number by number: as the one successor of a graph of one node every accepted number above 0 is "not a node
    index" and every refused one "too large"; with a shift of minus itself an arc list turns it into node 0; and the numbers that fit a
    graph come back from a round trip."""
    for v in NUMBERS:
        rec = same_ascii(W, b"1\n%d\n" % v)
        assert rec == ((1, [0, 1], [0]) if v == 0 else (M.E_IO, 2, 2, M.NOT_NODE))
        assert same_arcs(W, b"%d\t%d\n" % (v, v), shift=-v) == (1, [0, 1], [0])
    for v in (2 ** 63, 2 ** 63 + 1, 10 ** 19, 10 ** 19 - 1, 2 ** 64 - 1, 2 ** 64, 12345678901234567890, 10 ** 25):
        assert same_ascii(W, b"1\n%d\n" % v) == (M.E_IO, 2, 2, M.TOO_LARGE)
        assert same_arcs(W, b"0 %d\n" % v) == (M.E_IO, 1, 2, M.TOO_LARGE)
        assert same_ascii(W, b"%d\n" % v) == (M.E_IO, 1, 0, M.TOO_LARGE)
    assert same_ascii(W, b"8\n1 007\n" + b"0" * 25 + b"1\n" + b"\n" * 6)[2] == [1, 7, 1]
    assert same_ascii(W, b"0" * 30 + b"2\n" + b"0" * 40 + b"\n\n")[1:] == ([0, 1, 1], [0])
    n = 10 ** 6 + 2                                                          # a round trip of what fits a graph
    vals = [v for v in NUMBERS if v < n]
    off = np.zeros(n + 1, dtype=np.uint64); off[5:] = len(vals)
    text = b"%d\n" % n + W.format_csr(W.TEXT_ASCII, 0, off, vals)
    with W.parse_ascii_graph(text) as pg:
        o, a = pg.csr()
    assert np.array_equal(o, off) and a.tolist() == vals


# ---- tile boundaries and prefix-sum levels

def test_tokens_on_every_tile_residue(W):
    """19-digit tokens 23 bytes apart, 4 600 of them: 23 is odd, so token starts (and ends) fall on every residue of every power-of-two tile
    up to 4 096, and most tokens straddle a lane's 16 bytes.  A shift of -10^18 turns them into small ids."""
    rng = np.random.default_rng(23)
    ids = rng.integers(0, 3000, size=(2300, 2))
    text = b"".join(b"%d\t   %d   \n" % (10 ** 18 + int(s), 10 ** 18 + int(t)) for s, t in ids)
    assert len(text) == 4600 * 23
    got = same_arcs(W, text, shift=-10 ** 18)
    assert got[0] == int(ids.max()) + 1 and len(got[2]) == len(set(map(tuple, ids.tolist())))
    for cut in (1, 22, 23, 24):                                               # the last line loses its break, then its second number
        same_arcs(W, text[:-cut], shift=-10 ** 18)


def test_formatted_lists_on_every_residue(W):
    """Lists of 0..12 successors of 1..18 digits: the byte length of a line walks through every residue of the 4-byte words the text is
    written in, and 3 500 nodes with 21 000 successors make 48 workgroups of the writing pass."""
    rng = np.random.default_rng(7)
    lists = [sorted(set(int(rng.integers(0, 10 ** int(rng.integers(1, 19)))) for _ in range(x % 13))) for x in range(3500)]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    adj = np.array([v for l in lists for v in l], dtype=np.int64)
    assert {len(M.format_ascii([l])) % 4 for l in lists} == {0, 1, 2, 3}
    assert W.format_csr(W.TEXT_ASCII, 0, off, adj) == M.format_ascii(lists)
    assert W.format_csr(W.TEXT_ARCS, 10 ** 17, off, adj, 5) == M.format_arcs(lists, 10 ** 17, 5)
    for lo, hi in ((1, 2), (17, 3000), (3499, 3500), (0, 0)):                # a slice of the arrays: adj_off does not start at 0
        assert W.format_csr(W.TEXT_ASCII, lo, off[lo:hi + 1], adj) == M.format_ascii(lists[lo:hi])
        assert W.format_csr(W.TEXT_ARCS, lo, off[lo:hi + 1], adj) == M.format_arcs(lists[lo:hi], lo)


@pytest.mark.parametrize("count", [255, 256, 257, 65535, 65536, 65537, 70000])
def test_prefix_sum_levels(W, count):
    """`count` lines of one token each (and the header): token and line counts on either side of one tile of the prefix sum and of two levels."""
    vals = np.arange(count, dtype=np.int64)[::-1]
    text = b"%d\n" % count + b"".join(b"%d\n" % v for v in vals)
    with W.parse_ascii_graph(text) as pg:
        off, adj = pg.csr()
    assert np.array_equal(off, np.arange(count + 1)) and np.array_equal(adj, vals)
    arcs = b"".join(b"%d %d\n" % (v, v) for v in vals[:count // 2 + 1])     # the same number of tokens, half the lines
    with W.parse_arc_list(arcs + b"#%d tokens\n" % count) as pg:
        off, adj = pg.csr()
    want = np.sort(vals[:count // 2 + 1])
    assert pg.num_nodes() == count and np.array_equal(adj, want) and np.array_equal(np.diff(off.astype(np.int64)), np.isin(np.arange(count), want).astype(np.int64))


# ---- extreme shapes

def test_extreme_shapes(W, cnr):
    with W.parse_ascii_graph(b"100000\n" + b"\n" * 100000) as pg:
        off, adj = pg.csr()
        assert (pg.num_nodes(), pg.num_arcs()) == (100000, 0) and not off.any() and len(adj) == 0
        assert W.format_csr(W.TEXT_ASCII, 0, off, adj) == b"\n" * 100000
    line = b" ".join(b"%d" % v for v in range(100000)) + b" \n"
    with W.parse_ascii_graph(b"100000\n" + line + b"\r" * 99999) as pg:       # one list of 100 000, then lone '\r' lines
        off, adj = pg.csr()
        assert off[0] == 0 and (off[1:] == 100000).all() and np.array_equal(adj, np.arange(100000))
        assert W.format_csr(W.TEXT_ASCII, 0, off[:2], adj) == line
    for text in (b"0\n", b"0", b"0\r\n", b"1\n\n", b"1\r\n\r\n", b"1\r\r"):
        same_ascii(W, text)
    assert same_ascii(W, b"0\n")[0] == 0 and same_ascii(W, b"1\n\n") == (1, [0, 0], [])
    assert W.format_csr(W.TEXT_ASCII, 0, [0], []) == b"" and W.format_csr(W.TEXT_ARCS, 0, [0, 0, 0], []) == b""
    assert W.format_csr(W.TEXT_ASCII, 0, [0, 0], []) == b"\n"
    assert cnr.format_ascii(0, 0) == b"" and cnr.format_ascii(N_CNR, N_CNR) == b"" and cnr.format_arcs(7, 7, 3) == b""
    with pytest.raises(W.IllegalArgumentException):
        cnr.format_ascii(3, 2)
    with pytest.raises(W.IllegalArgumentException):
        cnr.format_arcs(0, N_CNR + 1)


def test_line_breaks_and_separators(W):
    lists = [[1, 2, 5], [], [0], [3, 4], [], [0, 4]]
    plain = b"6\n" + M.format_ascii(lists)
    want = (6, [0, 3, 3, 4, 6, 6, 8], [1, 2, 5, 0, 3, 4, 0, 4])
    for text in (plain, plain.replace(b"\n", b"\r\n"), plain.replace(b"\n", b"\r"), plain.replace(b" ", b"\t"), plain.replace(b" ", b" \x0b \x01\t"),
                 plain.replace(b" \n", b"\n"), b"6\r" + M.format_ascii(lists).replace(b"\n", b"\r\n"),
                 plain + b"-1 this / is # never . read\xff\n", plain.replace(b"\n", b"\r\n") + b"\nx", plain.replace(b"\n", b"\r") + b"\nx"):
        assert same_ascii(W, text) == want, text
    arcs = M.format_arcs(lists)
    for text in (arcs, arcs.replace(b"\n", b"\r\n"), arcs.replace(b"\n", b"\r"), arcs.replace(b"\t", b" "), arcs.replace(b"\t", b"  \t "), arcs[:-1],
                 arcs.replace(b"\n", b"\n\n\r\n"), b"# head\n" + arcs.replace(b"\n", b"\n#x 1 2 3 -\r\n"), b"\n" + arcs + b"#", b"#\r\n" + arcs + b"#9 9"):
        assert same_arcs(W, text) == want, text


# ---- refusals

ASCII_REFUSALS = [
    (b"3\n0 -1\n\n\n", M.BAD_BYTE), (b"3\n0 1.0\n\n\n", M.BAD_BYTE), (b"3\n0 1 /\n\n\n", M.BAD_BYTE), (b"3\n#\n\n\n", M.BAD_BYTE),
    (b"3\n0 \"1\"\n\n\n", M.BAD_BYTE), (b"3\n0 1'\n\n\n", M.BAD_BYTE), (b"3\nzero\n\n\n", M.BAD_BYTE), (b"3\n0 \xc3\xa9\n\n\n", M.BAD_BYTE), (b"3\n0 \x80\n\n\n", M.BAD_BYTE),
    (b"-3\n\n\n\n", M.BAD_BYTE), (b"3 \n\n\n\n", M.BAD_HEADER), (b"3 4\n\n\n\n", M.BAD_HEADER), (b"\n3\n", M.BAD_HEADER), (b"", M.BAD_HEADER),
    (b"3\n0 1 3\n\n\n", M.NOT_NODE), (b"3\n1 1\n\n\n", M.NOT_INCREASING), (b"3\n0 2 1\n\n\n", M.NOT_INCREASING), (b"3\n\n1 2\n0 0 \n", M.NOT_INCREASING),
    (b"3\n0\n1\n", M.EOF), (b"3\n0\n1\n2", M.EOF), (b"3\n0\n1\n2 ", M.EOF), (b"3", M.EOF), (b"1\n", M.EOF),
    (b"3\n0 1\n2 x\n", M.BAD_BYTE),                                          # two defects: the bad byte comes before the end of the text
    (b"3\n1 1 x\n\n\n", M.NOT_INCREASING), (b"3\n1 x 1\n\n\n", M.BAD_BYTE), (b"3\n\n5 y\n", M.NOT_NODE), (b"3\n2 99999999999999999999 1\n\n\n", M.TOO_LARGE),
]


@pytest.mark.parametrize("text,reason", ASCII_REFUSALS)
def test_ascii_refusals(W, text, reason):
    rec = same_ascii(W, text)
    assert rec[3] == reason and rec[0] == (W.E_ARG if reason == M.NOT_INCREASING else W.E_IO)
    assert same_ascii(W, b"2\n1 \n0 \n") == (2, [0, 1, 2], [1, 0])            # a healthy parse on the same device still works


ARC_REFUSALS = [
    (b"0 1\n2\n3 4\n", {}, M.ARC_FIELDS), (b"0 1\n2", {}, M.ARC_FIELDS), (b"0 1\n2 3 4\n", {}, M.ARC_FIELDS), (b"0 1 2 3", {}, M.ARC_FIELDS),
    (b"5 6\n0 1\n", dict(shift=-1), M.SHIFT_RANGE), (b"1 0\n", dict(shift=-1), M.SHIFT_RANGE), (b"1 9223372036854775807\n", dict(shift=1), M.SHIFT_RANGE),
    (b"0 1\n2 -3\n", {}, M.BAD_BYTE), (b"0 1 #\n", {}, M.BAD_BYTE), (b"0,1\n", {}, M.BAD_BYTE), (b"0 1\n 2 99999999999999999999\n", {}, M.TOO_LARGE),
    (b"0 1\n2\n3 x\n", {}, M.ARC_FIELDS), (b"0 1\n2 x\n3\n", {}, M.BAD_BYTE), (b"1 2 99999999999999999999\n", {}, M.TOO_LARGE),
]


@pytest.mark.parametrize("text,kw,reason", ARC_REFUSALS)
def test_arc_refusals(W, text, kw, reason):
    rec = same_arcs(W, text, **kw)
    assert rec[3] == reason and rec[0] == (W.E_ARG if reason == M.SHIFT_RANGE else W.E_IO)
    assert same_arcs(W, b"1 0\n0 1\n") == (2, [0, 1, 2], [1, 0])


def test_refusal_far_into_a_text(W):
    """The error record of a defect behind several tiles and prefix-sum blocks: the line is counted on the device."""
    n = 30000
    good = b"%d\n" % n + b"".join(b"%d %d \r\n" % (x // 2, x // 2 + 1) if x % 3 else b"\r\n" for x in range(n))
    for at in (len(good) // 2, len(good) - 9):
        cut = good.index(b" ", at)
        assert same_ascii(W, good[:cut] + b"x" + good[cut + 1:])[2:] == (cut, M.BAD_BYTE)
    lines = good.split(b"\r\n")                                              # (the header ends in a bare line feed: lines[0] holds it and the list of node 0)
    lines[20001] = b"7 7 "
    assert same_ascii(W, b"\r\n".join(lines))[1:] == (20003, len(b"\r\n".join(lines[:20001])) + 4, M.NOT_INCREASING)
    arcs = b"".join(b"%d\t%d\n" % (x, x + 1) for x in range(40000))
    cut = arcs.index(b"\n", len(arcs) * 3 // 4)
    assert same_arcs(W, arcs[:cut] + b" 5" + arcs[cut:])[3] == M.ARC_FIELDS
    assert same_arcs(W, arcs[:arcs.rindex(b"\t", 0, cut)] + arcs[cut:])[3] == M.ARC_FIELDS      # a line that lost its second number


# ---- arc-list semantics

def test_arc_list_semantics(W):
    text = b"5\t1\n0\t3\n#a comment 1 2 3\n\n5\t1\n2\t2\r\n0\t1\n   \n5 0\n"
    assert same_arcs(W, text) == (6, [0, 2, 2, 3, 3, 3, 5], [1, 3, 2, 0, 1])
    assert same_arcs(W, text, min_nodes=4)[0] == 6 and same_arcs(W, text, min_nodes=9)[0] == 9
    assert same_arcs(W, text, no_loops=True)[2] == [1, 3, 0, 1]
    assert same_arcs(W, text, symmetrize=True)[2] == [1, 3, 5, 0, 5, 2, 0, 0, 1]
    assert same_arcs(W, text, shift=10)[0] == 16
    assert same_arcs(W, b"") == (0, [0], []) and same_arcs(W, b"", min_nodes=3) == (3, [0, 0, 0, 0], [])
    assert same_arcs(W, b"# nothing\n\n\n", min_nodes=1) == (1, [0, 0], [])
    assert same_arcs(W, b"4 4\n", no_loops=True) == (5, [0] * 6, [])


def test_both_flags_equal_symmetrize_without_loops(W, tools):
    st = tools.synth_store(3000, seed=11)
    g = W.BVGraph.from_memory(st.params, st.graph, st.offsets)
    soff, ssucc = g.symmetrize()
    src = np.repeat(np.arange(3000), np.diff(soff.astype(np.int64)))
    keep = src != ssucc
    text = g.format_arcs(0, 3000)
    g.close()
    with W.parse_arc_list(text, symmetrize=True, no_loops=True) as pg:
        off, adj = pg.csr()
    assert np.array_equal(adj, ssucc[keep]) and np.array_equal(np.diff(off.astype(np.int64)), np.bincount(src[keep], minlength=3000))


# ---- capacity contract, device forms, store

class DeviceBytes:
    """A device buffer through the HIP runtime the library itself is linked against (torch would have to be imported before the library)."""
    hip = None

    def __init__(self, data):
        if DeviceBytes.hip is None:
            DeviceBytes.hip = C.CDLL("libamdhip64.so")
            DeviceBytes.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            DeviceBytes.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            DeviceBytes.hip.hipFree.argtypes = [C.c_void_p]
        self.host = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(len(self.host), 1)) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(self.ptr, self.host.ctypes.data, len(self.host), 1) == 0

    def get(self):
        assert self.hip.hipMemcpy(self.host.ctypes.data, self.ptr, len(self.host), 2) == 0
        return self.host

    def free(self):
        self.hip.hipFree(self.ptr)


def test_capacity_contract_and_device_forms(W, cnr, golden_text, line_starts):
    L = W.textgraph._text_fns()
    lo, hi = 1000, 1600
    want = golden_text[int(line_starts[lo]):int(line_starts[hi])]
    want_arcs = cnr.format_arcs(lo, hi, 2)
    nb = C.c_uint64(0)
    buf = np.full(len(want_arcs) + 8, 0xAA, dtype=np.uint8)
    for fn, extra, text in ((L.bvg_text_format_ascii, (), want), (L.bvg_text_format_arcs, (2,), want_arcs)):
        assert fn(cnr._h, lo, hi, *extra, None, 1 << 40, C.byref(nb)) == W.E_CAPACITY and nb.value == len(text)       # out == NULL: the size
        nb.value = 0
        assert fn(cnr._h, lo, hi, *extra, buf.ctypes.data, len(text) - 1, C.byref(nb)) == W.E_CAPACITY and nb.value == len(text)
        assert (buf == 0xAA).all()                                            # no text was written
        assert fn(cnr._h, lo, hi, *extra, buf.ctypes.data, len(text), C.byref(nb)) == 0 and buf[:len(text)].tobytes() == text
        assert (buf[len(text):] == 0xAA).all()
        buf[:] = 0xAA
    for fn, extra, text in ((L.bvg_text_format_ascii_dev, (), want), (L.bvg_text_format_arcs_dev, (2,), want_arcs)):
        for skew in (0, 1, 2, 3):                                             # a device buffer that does not start on a dword
            d = DeviceBytes(b"\x55" * (len(text) + 16))
            assert fn(cnr._h, lo, hi, *extra, d.ptr + skew, len(text) - 1, C.byref(nb)) == W.E_CAPACITY and nb.value == len(text)
            assert (d.get() == 0x55).all()
            assert fn(cnr._h, lo, hi, *extra, d.ptr + skew, len(text), C.byref(nb)) == 0
            h = d.get()
            assert h[skew:skew + len(text)].tobytes() == text and (h[:skew] == 0x55).all() and (h[skew + len(text):] == 0x55).all()
            d.free()
    off = np.array([0, 2, 2, 3], dtype=np.uint64); adj = np.array([1, 2, 0], dtype=np.int64)
    assert L.bvg_text_format_csr(0, 0, 3, off.ctypes.data, adj.ctypes.data, 0, buf.ctypes.data, 8, C.byref(nb)) == W.E_CAPACITY and nb.value == 9
    assert (buf == 0xAA).all()
    # the parsed CSR: host and device forms of the parse agree, and get / get_dev keep the capacity contract
    first = golden_text[:int(line_starts[5000])].split(b"\n")[1:5001]         # the first 5 000 nodes and the arcs among them
    text = b"5000\n" + b"".join(b"".join(t + b" " for t in l.split() if int(t) < 5000) + b"\n" for l in first)
    with W.parse_ascii_graph(text) as pg:
        o, a = pg.csr()
        n, m = pg.num_nodes(), pg.num_arcs()
        d_text = DeviceBytes(b"x" + text)
        with W.parse_ascii_graph_dev(d_text.ptr + 1, len(text)) as pd:                                                 # (an odd address)
            o2, a2 = pd.csr()
        d_text.free()
        assert np.array_equal(o, o2) and np.array_equal(a, a2) and n == 5000 and m == len(a) > 1000
        ob = np.full(n + 1, 77, dtype=np.uint64); ab = np.full(m, 77, dtype=np.int64)
        assert L.bvg_text_get(pg._h, ob.ctypes.data, n, ab.ctypes.data, m) == W.E_CAPACITY
        assert L.bvg_text_get(pg._h, ob.ctypes.data, n + 1, ab.ctypes.data, m - 1) == W.E_CAPACITY
        assert (ob == 77).all() and (ab == 77).all()
        assert L.bvg_text_get(pg._h, None, 0, ab.ctypes.data, m) == 0 and np.array_equal(ab, a)
        do, da = DeviceBytes(bytes(8 * (n + 1))), DeviceBytes(bytes(8 * m))
        assert L.bvg_text_get_dev(pg._h, do.ptr, n, da.ptr, m) == W.E_CAPACITY and not do.get().any() and not da.get().any()
        pg.csr_dev(do.ptr, n + 1, da.ptr, m)
        assert np.array_equal(do.get().view(np.uint64), o) and np.array_equal(da.get().view(np.int64), a)
        do.free(); da.free()
        # ParsedGraph.store == bvg_store on csr(), single range and chunked
        for chunk in (0, 700):
            g1, f1 = pg.store(None, chunk)
            g2, f2 = W.store((o, a), None, chunk)
            assert g1.tobytes() == g2.tobytes() and np.array_equal(f1, f2)
    arcs = M.format_arcs(M.lists_of(o, a))
    d_arcs = DeviceBytes(arcs)
    with W.parse_arc_list_dev(d_arcs.ptr, len(arcs), min_nodes=5000) as pd:
        o3, a3 = pd.csr()
    d_arcs.free()
    assert np.array_equal(o, o3) and np.array_equal(a, a3)


def test_host_csr_writers_do_not_depend_on_their_ranges(W, tmp_path):
    """ParsedGraph / EFGraph .to_ascii_graph and .to_arc_list go through an adjacency in host memory, range after range: ranges of 1 item
    (every node alone), of 50 and of 1 000 items must write what one range writes."""
    rng = np.random.default_rng(9)
    lists = [np.flatnonzero(rng.random(400) < (0.5 if x % 50 == 7 else 0.02)).tolist() for x in range(400)]
    text = b"400\n" + M.format_ascii(lists)
    with W.parse_ascii_graph(text) as pg:
        for per in (None, 1, 50, 1000):
            assert open(pg.to_ascii_graph(str(tmp_path / ("p%s" % per)), range_items=per), "rb").read() == text, per
            assert open(pg.to_arc_list(str(tmp_path / ("a%s" % per)), 3, range_items=per), "rb").read() == M.format_arcs(lists, 0, 3), per
        W.write_bvgraph(str(tmp_path / "bv"), pg)
    g = W.BVGraph.load(str(tmp_path / "bv"))
    ef = W.BVGraph.to_efgraph(g)
    for per in (None, 1, 50, 1000):
        assert open(ef.to_ascii_graph(str(tmp_path / ("e%s" % per)), range_items=per), "rb").read() == text, per
        assert open(ef.to_arc_list(str(tmp_path / ("f%s" % per)), 3, range_items=per), "rb").read() == M.format_arcs(lists, 0, 3), per
    for ranges in (1, 3, 400):
        assert open(g.to_ascii_graph(str(tmp_path / ("g%d" % ranges)), ranges=ranges), "rb").read() == text, ranges
        assert open(g.to_arc_list(str(tmp_path / ("h%d" % ranges)), 3, ranges=ranges), "rb").read() == M.format_arcs(lists, 0, 3), ranges
    ef.close(); g.close()
    L = W.textgraph._text_fns()
    nb = C.c_uint64(0); h = C.c_void_p(); err = W.TextError()
    assert L.bvg_text_parse_arcs(b"0 1\n", 4, -2 ** 63, 0, 0, 0, C.byref(h), C.byref(err)) == W.E_ARG             # -shift does not exist
    off = np.array([0, 1], dtype=np.uint64); adj = np.zeros(1, dtype=np.int64)
    assert L.bvg_text_format_csr(1, 0, 1, off.ctypes.data, adj.ctypes.data, -2 ** 63, None, 0, C.byref(nb)) == W.E_ARG


# ---- files and command lines

def test_files_and_mains(W, tmp_path):
    lists = [[1, 2, 5], [], [0], [3, 4], [], [0, 4], [6]]
    src = str(tmp_path / "small")
    open(src + ".graph-txt", "wb").write(b"7\n" + M.format_ascii(lists))
    assert W.bvgraph_main(["-g", "ASCIIGraph", "-w", "3", "-i", "2", src, str(tmp_path / "bv")]) == 0
    g = W.BVGraph.load(str(tmp_path / "bv"))
    deg, succ = g.decode_range(0, 7)
    assert g.window_size() == 3 and g.num_arcs() == 9 and deg.tolist() == [len(l) for l in lists] and succ.tolist() == [v for l in lists for v in l]
    g.close()
    assert W.asciigraph_main([str(tmp_path / "bv"), str(tmp_path / "back")]) == 0
    assert open(str(tmp_path / "back.graph-txt"), "rb").read() == open(src + ".graph-txt", "rb").read()
    assert W.arclist_main(["-S", "1", str(tmp_path / "bv"), str(tmp_path / "arcs.txt")]) == 0
    assert open(str(tmp_path / "arcs.txt"), "rb").read() == M.format_arcs(lists, 0, 1)
    assert W.bvgraph_main(["-g", "ArcListASCIIGraph", str(tmp_path / "arcs.txt"), str(tmp_path / "bv2")]) == 0     # (ids one up: node 0 is there, without arcs)
    g = W.BVGraph.load(str(tmp_path / "bv2"))
    assert g.num_nodes() == 8 and g.decode_range(0, 8)[1].tolist() == [v + 1 for l in lists for v in l]
    # the same through an EFGraph, and a gzip'ed source
    ef = W.BVGraph.to_efgraph(g, basename=str(tmp_path / "ef"))
    assert open(ef.to_ascii_graph(str(tmp_path / "ef_txt")), "rb").read() == open(g.to_ascii_graph(str(tmp_path / "bv2_txt")), "rb").read()
    assert open(ef.to_arc_list(str(tmp_path / "ef_arcs"), 3), "rb").read() == open(g.to_arc_list(str(tmp_path / "bv2_arcs"), 3), "rb").read()
    ef.close(); g.close()
    assert W.asciigraph_main(["-g", "EFGraph", str(tmp_path / "ef"), str(tmp_path / "ef_back")]) == 0
    assert open(str(tmp_path / "ef_back.graph-txt"), "rb").read() == open(str(tmp_path / "bv2_txt.graph-txt"), "rb").read()
    with gzip.open(str(tmp_path / "z.graph-txt.gz"), "wb") as f:
        f.write(b"7\n" + M.format_ascii(lists))
    for name in ("z", "z.graph-txt.gz"):
        with W.load_ascii_graph(str(tmp_path / name)) as pg:
            assert M.lists_of(*pg.csr()) == lists
    with W.load_arc_list(str(tmp_path / "arcs.txt"), shift=-1) as pg:
        assert M.lists_of(*pg.csr()) == lists
        W.write_bvgraph(str(tmp_path / "bv3"), pg, W.default_params(offset_coding=W.DELTA, residual_coding=W.GAMMA))
    g = W.BVGraph.load(str(tmp_path / "bv3"))
    assert g.decode_range(0, 7)[1].tolist() == [v for l in lists for v in l] and g.params.residual_coding == W.GAMMA
    g.close()
    W.write_bvgraph(str(tmp_path / "bv4"), lists)
    g = W.BVGraph.load(str(tmp_path / "bv4"))
    assert g.format_ascii(0, 7) == M.format_ascii(lists)
    g.close()
