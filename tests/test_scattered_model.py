"""CPU: the model of the scattered arc list contract (tests/scattered_model.py) against the reference's own expectations
(tests/scattered_cases.py) and against the contract's fine print, so that the GPU tests compare the device with something that was
itself checked."""
import pytest

import scattered_model as M
from scattered_cases import EXAMPLE_ARCS, REFERENCE_CASES


@pytest.mark.parametrize("case", range(len(REFERENCE_CASES)))
def test_reference_expectations(case):
    text, sym, nol, arcs, ids = REFERENCE_CASES[case]
    r = M.parse(text, sym, nol)
    assert (r["ids"], r["arcs"], r["nodes"]) == (ids, sorted(arcs), len(ids))


def test_example_report():
    rep = M.parse(EXAMPLE_ARCS)["report"]
    assert (rep["lines"], rep["arcs"], rep["trailing"], rep["bad_source"]) == (6, 4, 1, 1)
    assert (rep["first_reason"], rep["first_line"], rep["first_byte"]) == ("bad_source", 5, EXAMPLE_ARCS.index(b"OOPS"))


@pytest.mark.parametrize("tok,want", [(b"-", 0), (b"-0", 0), (b"007", 7), (b"-007", -7), (b"9223372036854775807", M.INT64_MAX), (b"-9223372036854775808", M.INT64_MIN),
                                      (b"0" * 40 + b"12", 12), (b"+1", "bad"), (b"--1", "bad"), (b"1-", "bad"), (b"1x", "bad"), (b"\xc3\xa9", "bad"), (b"1\x80", "bad"),
                                      (b"9223372036854775808", "big"), (b"-9223372036854775809", "big"), (b"1234567890123456789012345", "big"),
                                      (b"12345678901234567890x", "big"), (b"1234567890123456789x", "bad")])
def test_identifiers(tok, want):
    kind, v = M.identifier(tok)
    assert (v if kind == "ok" else kind) == want


def test_lines_and_tokens():
    assert [l for _, l in M.lines_of(b"a\rb\nc\r\nd\n\re")] == [b"a", b"b", b"c", b"d", b"", b"e"]
    assert M.lines_of(b"") == [] and M.lines_of(b"\r\n") == [(0, b"")] and [o for o, _ in M.lines_of(b"x\r\n\ny")] == [0, 3, 4]
    assert M.tokens_of(b" \x00a\x0bb\x80 \t#c ") == [(2, b"a"), (4, b"b\x80"), (8, b"#c")]


def test_registration_rules():
    assert M.parse(b"7\n")["ids"] == [7] and M.parse(b"7\n")["report"]["no_target"] == 1
    assert M.parse(b"7 X\n")["ids"] == [7] and M.parse(b"7 X\n")["report"]["bad_target"] == 1
    r = M.parse(b"X 9\n")
    assert r["ids"] == [] and r["report"]["bad_source"] == 1 and r["report"]["first_byte"] == 0
    assert M.parse(b"5 5\n")["arcs"] == [(0, 0)]
    r = M.parse(b"5 5\n", no_loops=True)
    assert (r["ids"], r["arcs"], r["report"]["dropped_loops"], r["report"]["arcs"]) == ([5], [], 1, 0)
    r = M.parse(b" #x 1\n#x 1\n1 2 #")
    assert (r["ids"], r["report"]["bad_source"], r["report"]["trailing"], r["report"]["lines"]) == ([1, 2], 1, 1, 3)
    r = M.parse(b"99999999999999999999 1\n1 99999999999999999999\n")
    assert (r["ids"], r["report"]["too_large"], r["report"]["first_reason"]) == ([1], 2, "too_large")


def test_given_numbering():
    r = M.parse(b"2 -1\n3 2\n2 3\n7\n-1 -1 x\n", ids=[2, -1, 7, 40])
    assert (r["nodes"], r["ids"], r["arcs"]) == (4, [2, -1, 7, 40], [(0, 1), (1, 1)])
    rep = r["report"]
    assert (rep["unknown_source"], rep["unknown_target"], rep["no_target"], rep["trailing"], rep["arcs"]) == (1, 1, 1, 1, 2)
    assert (rep["first_reason"], rep["first_line"], rep["first_byte"]) == ("unknown_source", 2, 5)
    with pytest.raises(ValueError):
        M.parse(b"", ids=[1, 2, 1])
