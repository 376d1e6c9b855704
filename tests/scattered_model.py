"""A plain restatement of the scattered arc list contract (include/bvgraph_hip.h, "scattered arc lists"): line by line, with a dict.
Written from the contract, not from any implementation; the GPU tests hold the device against it."""
import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
REASONS = ("bad_source", "bad_target", "no_target", "too_large", "trailing", "unknown_source", "unknown_target")
COUNTS = ("lines", "arcs") + REASONS + ("dropped_loops",)


def lines_of(data):
    """[(offset of the line's first byte, its bytes)]: lines end at \\r, \\n or \\r\\n; a last line without a terminator counts when it has bytes."""
    out, start, i, n = [], 0, 0, len(data)
    while i < n:
        c = data[i]
        if c == 13 or c == 10:
            out.append((start, data[start:i]))
            i += 2 if c == 13 and i + 1 < n and data[i + 1] == 10 else 1
            start = i
        else:
            i += 1
    if start < n:
        out.append((start, data[start:]))
    return out


def tokens_of(line):
    """[(offset in the line, bytes)]: maximal runs of bytes above 32."""
    out, i, n = [], 0, len(line)
    while i < n:
        if line[i] <= 32:
            i += 1
            continue
        j = i
        while j < n and line[j] > 32:
            j += 1
        out.append((i, line[i:j]))
        i = j
    return out


def identifier(tok):
    """("ok", value), ("bad", None) or ("big", None): an optional '-', then digits, read from left to right -- the first thing wrong decides."""
    neg = tok[:1] == b"-"
    m, sig = 0, 0
    for c in tok[1:] if neg else tok:
        if not 48 <= c <= 57:
            return "bad", None
        if sig == 0 and c == 48:
            continue
        sig += 1
        if sig > 19:
            return "big", None
        m = m * 10 + (c - 48)
    v = -m if neg else m
    if not INT64_MIN <= v <= INT64_MAX:
        return "big", None
    return "ok", v


def parse(data, symmetrize=False, no_loops=False, ids=None):
    """-> dict(nodes, ids (list), arcs (sorted list of distinct (source, target) node pairs), report (dict))."""
    if isinstance(data, str):
        data = data.encode("latin-1")
    data = bytes(data)
    given = ids is not None
    number = {}
    if given:
        for i, v in enumerate(ids):
            if int(v) in number:
                raise ValueError("a value occurs twice in ids")
            number[int(v)] = i
    rep = dict.fromkeys(COUNTS, 0)
    rep.update(first_byte=0, first_line=0, first_reason=None)
    arcs = set()

    def offend(reason, byte, line):
        rep[reason] += 1
        if rep["first_reason"] is None:                    # the lines come in the order of their offsets, and a line offends once
            rep.update(first_byte=byte, first_line=line, first_reason=reason)

    def node(v):
        if given:
            return number.get(v)
        return number.setdefault(v, len(number))

    for ln, (start, line) in enumerate(lines_of(data), 1):
        rep["lines"] += 1
        if line[:1] == b"#":
            continue
        toks = tokens_of(line)
        if not toks:
            continue
        (so, st), tgt = toks[0], toks[1] if len(toks) > 1 else None
        kind, s = identifier(st)
        if kind != "ok":
            offend("too_large" if kind == "big" else "bad_source", start + so, ln)
            continue
        if tgt is not None:
            tkind, t = identifier(tgt[1])
            if tkind == "ok" and len(toks) > 2:
                rep["trailing"] += 1
        x = node(s)                                            # a good source is registered whatever follows
        if tgt is None:
            offend("no_target", start + so, ln)
            continue
        if tkind != "ok":
            offend("too_large" if tkind == "big" else "bad_target", start + tgt[0], ln)
            continue
        if given and x is None:
            offend("unknown_source", start + so, ln)
            continue
        y = node(t)
        if given and y is None:
            offend("unknown_target", start + tgt[0], ln)
            continue
        if no_loops and x == y:
            rep["dropped_loops"] += 1
            continue
        rep["arcs"] += 1
        arcs.add((x, y))
        if symmetrize:
            arcs.add((y, x))
    if given:
        out_ids = [int(v) for v in ids]
    else:
        out_ids = [None] * len(number)
        for v, i in number.items():
            out_ids[i] = v
    return {"nodes": len(out_ids), "ids": out_ids, "arcs": sorted(arcs), "report": rep}


def csr(nodes, arcs):
    """(adj_off uint64[nodes + 1], adj int64[len(arcs)]) of sorted distinct arcs."""
    off = np.zeros(nodes + 1, dtype=np.uint64)
    for s, _ in arcs:
        off[s + 1] += 1
    return np.cumsum(off).astype(np.uint64), np.array([t for _, t in arcs], dtype=np.int64)
