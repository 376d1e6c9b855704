"""CPU model of the text graph formats (include/bvgraph_hip.h, "text graphs"): ASCIIGraph and arc lists, parsed and formatted in plain
Python, line by line -- written from the format description, sharing no code with the library.  A refusal is the error record the library
must report: the status, the 1-based line, the byte offset and the reason of the FIRST offending byte."""
import re

import numpy as np

E_ARG, E_IO = -1, -4
BAD_BYTE, BAD_HEADER, TOO_LARGE, NOT_NODE, NOT_INCREASING, SHIFT_RANGE, ARC_FIELDS, EOF = (
    "bad_byte", "bad_header", "too_large", "not_node", "not_increasing", "shift_range", "arc_fields", "eof")
_STATUS = {NOT_INCREASING: E_ARG, SHIFT_RANGE: E_ARG}
MAX = (1 << 63) - 1

_BREAK = re.compile(rb"\r\n|\r|\n")                  # a '\r' always ends a line; a '\n' does unless it follows a '\r'
_PIECE = re.compile(rb"[0-9]+|[^\x00-\x20]")         # a number, or one byte that is neither digit nor separator
_DIGITS = bytes(range(48, 58))
_SEPARATORS = bytes(range(33))
_TO_SPACE = bytes(32 if c < 33 else c for c in range(256))


class Refusal(Exception):
    def __init__(self, reason, line, byte):
        self.status, self.reason, self.line, self.byte = _STATUS.get(reason, E_IO), reason, line, byte
        super().__init__("%s at line %d, byte %d" % (reason, line, byte))

    def record(self):
        return (self.status, self.line, self.byte, self.reason)


def _lines(data, pos=0):
    """(start, end, terminated) of every line from pos on; the last one is unterminated (and may be empty)."""
    while True:
        m = _BREAK.search(data, pos)
        if m is None:
            yield pos, len(data), False
            return
        yield pos, m.start(), True
        pos = m.end()


def parse_ascii(data):
    """-> (n, adj_off uint64[n + 1], adj int64[m]); raises Refusal."""
    data = bytes(data)
    lines = _lines(data)
    s, e, terminated = next(lines)
    for i in range(s, e):
        if data[i] not in _DIGITS:
            raise Refusal(BAD_BYTE if data[i] > 32 else BAD_HEADER, 1, i)
    if e == s:
        raise Refusal(BAD_HEADER, 1, 0)
    n = int(data[s:e])
    if n > MAX:
        raise Refusal(TOO_LARGE, 1, 0)
    if n and not terminated:                          # the text ends inside the header's line
        raise Refusal(EOF, 1, len(data))
    off, adj = [0], []
    for x in range(n):
        lineno = x + 2
        s, e, terminated = next(lines)
        line = data[s:e]
        good = None
        if not line.translate(None, _DIGITS + _SEPARATORS):            # nothing but digits and separators: usually all there is to it
            vals = [int(t) for t in line.translate(_TO_SPACE).split()]
            if all(a < b for a, b in zip(vals, vals[1:])) and (not vals or vals[-1] < n):
                good = vals
        if good is None:
            prev = -1
            good = []
            for m in _PIECE.finditer(line):
                at = s + m.start()
                if not m.group()[0:1].isdigit():
                    raise Refusal(BAD_BYTE, lineno, at)
                v = int(m.group())
                if v > MAX:
                    raise Refusal(TOO_LARGE, lineno, at)
                if v >= n:
                    raise Refusal(NOT_NODE, lineno, at)
                if v <= prev:
                    raise Refusal(NOT_INCREASING, lineno, at)
                prev = v
                good.append(v)
        if not terminated:                            # the reference meets EOF inside this line
            raise Refusal(EOF, lineno, len(data))
        adj.extend(good)
        off.append(len(adj))
    return n, np.array(off, dtype=np.uint64), np.array(adj, dtype=np.int64)


def parse_arcs(data, shift=0, symmetrize=False, no_loops=False, min_nodes=0):
    """-> (nodes, adj_off, adj); raises Refusal."""
    data = bytes(data)
    pairs = []
    for lineno, (s, e, terminated) in enumerate(_lines(data), 1):
        line = data[s:e]
        if line[:1] == b"#":
            continue
        ids = []
        for m in _PIECE.finditer(line):
            at = s + m.start()
            if not m.group()[0:1].isdigit():
                raise Refusal(BAD_BYTE, lineno, at)
            v = int(m.group())
            if v > MAX:
                raise Refusal(TOO_LARGE, lineno, at)
            if not 0 <= v + shift <= MAX:
                raise Refusal(SHIFT_RANGE, lineno, at)
            if len(ids) == 2:
                raise Refusal(ARC_FIELDS, lineno, at)
            ids.append(v + shift)
        if len(ids) == 1:
            raise Refusal(ARC_FIELDS, lineno, e)      # at the line break (at the end of the text when there is none)
        if ids:
            pairs.append(tuple(ids))
    # the largest id counts even when its arc is a dropped loop: the graph is sized by the ids of the text
    nodes = max(max(max(p) for p in pairs) + 1 if pairs else 0, min_nodes)
    if symmetrize:
        pairs += [(t, s) for s, t in pairs]
    if no_loops:
        pairs = [(s, t) for s, t in pairs if s != t]
    return (nodes,) + csr_of_pairs(nodes, pairs)


def csr_of_pairs(nodes, pairs):
    uniq = sorted(set(pairs))
    off = np.zeros(nodes + 1, dtype=np.uint64)
    for s, _ in uniq:
        off[s + 1] += 1
    return np.cumsum(off, dtype=np.uint64), np.array([t for _, t in uniq], dtype=np.int64)


def format_ascii(lists):
    """ASCIIGraph.store without its header line: every successor followed by one space, then a line feed."""
    return b"".join((" ".join(map(str, l)) + " \n").encode() if len(l) else b"\n" for l in lists)


def format_arcs(lists, first_node=0, shift=0):
    return b"".join(b"%d\t%d\n" % (first_node + x + shift, int(t) + shift) for x, l in enumerate(lists) for t in l)


def lists_of(off, adj):
    off = [int(v) for v in off]
    return [adj[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
