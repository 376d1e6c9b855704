"""The plain reference of the arc-label decode (csrc/bvg_labels.hip): a bit reader over arbitrary-precision ints, written from the
description of the format alone (labelling/BitStreamArcLabelledImmutableGraph.java:75-84 and the four label classes' fromBitStream).  It
shares no code with the oracle (oracle/bvg_oracle.c), the tooling writer (tooling/bvg_store.cpp) or the device.

The stream is read MSB first.  unary = zeros before a one; gamma(x) = unary(msb) then the msb low bits of x + 1, as an unbounded int;
readInt(width) / readLong(width) = `width` bits.  The int32 / int64 wrap of the element types is applied to the finished arrays only.

A decode of nodes [frm, to) ends in one of two things:
  * Decoded: .labels (scalar classes) or .list_off + .values (list classes; .values is None when there are more than VALUES_LIMIT
    elements: the lengths alone say how many, test code never builds such an array);
  * Defect: .name is
      "overrun"      a read past the node's run (the file's end included: behind it the stream reads as zeros for ever),
      "short"        a run that is longer than what its node's labels take,
      "gamma_range"  a gamma-coded label or list length of 2^31 or more (readGamma() is an int),
    and, for the list classes, .list_off: the prefix of the lengths in which every list that cannot be read inside its run counts as
    empty, along with the rest of its node (what bvg_labels_decode_range_lists[64] leave in list_off next to BVG_E_EOF).
check_offsets() names the fourth defect, "offsets" (non-monotone, or past the file), which the open refuses before anything is decoded."""
import numpy as np

GAMMA, FIXED, LIST, LONG_LIST = 1, 2, 3, 4
VALUES_LIMIT = 1 << 22


class Decoded:
    def __init__(self, labels=None, list_off=None, values=None, total=0):
        self.labels, self.list_off, self.values, self.total = labels, list_off, values, total
    ok = True


class Defect:
    def __init__(self, name, node, list_off=None):
        self.name, self.node, self.list_off = name, node, list_off
    ok = False

    def __repr__(self):
        return "Defect(%s at node %d)" % (self.name, self.node)


class Bits:
    """bits [0, 8 * len(stream)) of the stream, zeros behind them"""

    def __init__(self, stream):
        self.s = bytes(stream)
        self.n = 8 * len(self.s)

    def read(self, pos, width):
        """`width` bits from bit `pos` on"""
        if width == 0:
            return 0
        end = pos + width
        chunk = self.s[pos >> 3:(end + 7) >> 3]                                  # (a slice behind the stream is short or empty ...)
        v = int.from_bytes(chunk, "big") << (8 * (((end + 7) >> 3) - (pos >> 3) - len(chunk)))   # (... and stands for zeros)
        return (v >> (-end % 8)) & ((1 << width) - 1)

    def zeros(self, pos):
        """the number of zeros from `pos` to the next one, None when no one follows"""
        at = pos
        while at < self.n:
            step = 128 - (at & 7)                                              # to a byte boundary, then 16 bytes at a time
            v = self.read(at, step)
            if v:
                z = at + step - v.bit_length() - pos
                return z if pos + z < self.n else None
            at += step
        return None


class _Stop(Exception):
    def __init__(self, name):
        self.name = name


def _gamma(b, pos, end):
    """(value, position behind the code); the code must lie inside [pos, end)"""
    z = b.zeros(pos)
    if z is None or pos + 2 * z + 1 > end:
        raise _Stop("overrun")
    return ((1 << z) | b.read(pos + z + 1, z)) - 1, pos + 2 * z + 1


def check_offsets(nbytes, offsets):
    """None, or the reason the open refuses the offsets: "past_file" (the last one lies behind the stream) before "non_monotone"."""
    offsets = [int(o) for o in offsets]
    if offsets[-1] > 8 * nbytes:
        return "past_file"
    if any(a > b for a, b in zip(offsets, offsets[1:])):
        return "non_monotone"
    return None


def decode(kind, width, stream, offsets, frm, to, deg):
    """deg[to - frm]: the outdegrees of nodes [frm, to)."""
    assert check_offsets(len(bytes(stream)), offsets) is None
    b = Bits(stream)
    first = None
    labels, lens, values = [], [], []
    for x in range(frm, to):
        pos, end, d = int(offsets[x]), int(offsets[x + 1]), int(deg[x - frm])
        try:
            if kind in (GAMMA, FIXED):
                for j in range(d):
                    if kind == GAMMA:
                        v, pos = _gamma(b, pos, end)
                        if v >= 1 << 31:
                            raise _Stop("gamma_range")
                    else:
                        if pos + width > end:
                            raise _Stop("overrun")
                        v, pos = b.read(pos, width), pos + width
                    labels.append(v)
            else:
                for j in range(d):
                    try:
                        n, pos = _gamma(b, pos, end)
                        if n >= 1 << 31:
                            raise _Stop("gamma_range")
                        if pos + n * width > end:
                            raise _Stop("overrun")
                    except _Stop:
                        lens.extend([0] * (d - j))
                        raise
                    lens.append(n)
                    if first is None and len(values) <= VALUES_LIMIT:
                        if n > VALUES_LIMIT:
                            values.extend([0] * (VALUES_LIMIT + 1))                  # (over the limit: never looked at)
                        else:
                            values.extend(b.read(pos + t * width, width) for t in range(n))
                    pos += n * width
            if pos != end:
                raise _Stop("short")
        except _Stop as s:
            if first is None:
                first = Defect(s.name, x)
            if kind in (GAMMA, FIXED):
                return first
    if kind in (GAMMA, FIXED):
        return Decoded(labels=np.array(labels, dtype=np.uint64).astype(np.uint32).view(np.int32), total=len(labels))
    list_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    if lens:
        list_off[1:] = np.cumsum(np.array(lens, dtype=np.uint64))
    if first is not None:
        first.list_off = list_off
        return first
    total = int(list_off[-1])
    if total > VALUES_LIMIT:
        return Decoded(list_off=list_off, values=None, total=total)
    v = np.array(values, dtype=np.uint64)
    return Decoded(list_off=list_off, values=v.astype(np.uint32).view(np.int32) if kind == LIST else v.view(np.int64), total=total)
