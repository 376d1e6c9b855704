"""CPU: the model of the text formats (tests/textgraph_model.py) held against the reference's own expected answer -- the golden
cnr-2000.graph-txt is byte for byte what ASCIIGraph.store writes, and the oracle decodes cnr-2000.graph -- and against the refusal
rules on hand-made texts."""
import gzip

import numpy as np
import pytest

import textgraph_model as M
from conftest import CNR


@pytest.fixture(scope="module")
def golden_text():
    with gzip.open(CNR + ".graph-txt.gz", "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def oracle_csr(oracle):
    og = oracle.Graph.load(CNR)
    deg, succ = og.decode_range(0, og.num_nodes())
    return np.asarray(deg, dtype=np.int64), np.asarray(succ, dtype=np.int64)


def test_formatting_the_decoded_fixture_gives_the_golden_text(golden_text, oracle_csr):
    deg, succ = oracle_csr
    off = np.concatenate([[0], np.cumsum(deg)])
    text = b"%d\n" % len(deg) + M.format_ascii(M.lists_of(off, succ))
    assert len(golden_text) == 22248688 and text == golden_text


def test_parsing_the_golden_text_gives_the_decoded_fixture(golden_text, oracle_csr):
    deg, succ = oracle_csr
    n, off, adj = M.parse_ascii(golden_text)
    assert n == len(deg) == 325557 and np.array_equal(np.diff(off.astype(np.int64)), deg) and np.array_equal(adj, succ)


def test_arc_list_model_round_trip():
    lists = [[1, 2, 5], [], [0], [3], [], [0, 4]]
    text = M.format_arcs(lists, 0, 3)
    assert text.startswith(b"3\t4\n3\t5\n3\t8\n5\t3\n")
    n, off, adj = M.parse_arcs(text, shift=-3)
    assert n == 6 and M.lists_of(off, adj) == lists
    lines = text.split(b"\n")[:-1]
    n, off, adj = M.parse_arcs(b"\r\n".join(reversed(lines)) + b"\r# a comment\r\r" + lines[0], shift=-3, min_nodes=9)     # any order, a duplicate, no final break
    assert n == 9 and M.lists_of(off, adj) == lists + [[], [], []]
    n, off, adj = M.parse_arcs(text, shift=-3, symmetrize=True, no_loops=True)
    assert M.lists_of(off, adj) == [[1, 2, 5], [0], [0], [], [5], [0, 4]]
    assert M.parse_arcs(b"", min_nodes=2)[0] == 2 and M.parse_arcs(b"7 7\n", no_loops=True)[0] == 8


@pytest.mark.parametrize("text,record", [
    (b"", (M.E_IO, 1, 0, M.BAD_HEADER)),
    (b"\n", (M.E_IO, 1, 0, M.BAD_HEADER)),
    (b"3 \n\n\n\n", (M.E_IO, 1, 1, M.BAD_HEADER)),
    (b"+3\n\n\n\n", (M.E_IO, 1, 0, M.BAD_BYTE)),
    (b"9223372036854775808\n", (M.E_IO, 1, 0, M.TOO_LARGE)),
    (b"2\n1 x\n\n", (M.E_IO, 2, 4, M.BAD_BYTE)),
    (b"2\n0 1.0\n\n", (M.E_IO, 2, 5, M.BAD_BYTE)),
    (b"2\n\n2\n", (M.E_IO, 3, 3, M.NOT_NODE)),
    (b"3\n1 1\n\n\n", (M.E_ARG, 2, 4, M.NOT_INCREASING)),
    (b"3\n2 1\n\n\n", (M.E_ARG, 2, 4, M.NOT_INCREASING)),
    (b"3\n\n\n", (M.E_IO, 4, 4, M.EOF)),                                 # n - 1 complete lines: the text ends where line 4 would start
    (b"2\n\n0", (M.E_IO, 3, 4, M.EOF)),
    (b"2\n1 1\n0 x", (M.E_ARG, 2, 4, M.NOT_INCREASING)),                     # two defects: the earlier one
    (b"1\n00000000000000000000000018446744073709551616\n", (M.E_IO, 2, 2, M.TOO_LARGE)),
])
def test_ascii_refusals(text, record):
    with pytest.raises(M.Refusal) as e:
        M.parse_ascii(text)
    assert e.value.record() == record


@pytest.mark.parametrize("text,kw,record", [
    (b"1\n", {}, (M.E_IO, 1, 1, M.ARC_FIELDS)),
    (b"0 1\n1", {}, (M.E_IO, 2, 5, M.ARC_FIELDS)),
    (b"0 1 2\n", {}, (M.E_IO, 1, 4, M.ARC_FIELDS)),
    (b"0 1\n", dict(shift=-1), (M.E_ARG, 1, 0, M.SHIFT_RANGE)),
    (b"0 9223372036854775807\n", dict(shift=1), (M.E_ARG, 1, 2, M.SHIFT_RANGE)),
    (b"0 1 #\n", {}, (M.E_IO, 1, 4, M.BAD_BYTE)),
    (b"0\t-1\n", {}, (M.E_IO, 1, 2, M.BAD_BYTE)),
])
def test_arc_refusals(text, kw, record):
    with pytest.raises(M.Refusal) as e:
        M.parse_arcs(text, **kw)
    assert e.value.record() == record


def test_accepted_oddities():
    n, off, adj = M.parse_ascii(b"8\r\n\t1  007\x0b\r\n0000000000000000000000001\r\n" + b"\r\n" * 6 + b"this is never read: -1.5e3 /")
    assert (n, M.lists_of(off, adj)) == (8, [[1, 7], [1]] + [[]] * 6)
    n, off, adj = M.parse_ascii(b"3\r0 1\r\n2\r\r\n")                      # a lone '\r', "\r\n", and a '\r' right before a "\r\n"
    assert (n, M.lists_of(off, adj)) == (3, [[0, 1], [2], []])
    assert M.parse_ascii(b"0")[0] == 0 and M.parse_ascii(b"0\n-")[0] == 0     # no list is asked for: not even the header's line break
    assert M.lists_of(*M.parse_ascii(b"1\n\n")[1:]) == [[]]
