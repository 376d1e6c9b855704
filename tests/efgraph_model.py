"""A plain model of EFGraph (src/it/unimi/dsi/big/webgraph/EFGraph.java), for the tests: no product import.

The writer follows Accumulator.init / add / dump (:476-532) and LongWordOutputBitStream (:294-414) step by step -- it keeps the three
bit caches, writes unary gaps and runs the pointer loop of :511-513 -- and never uses the closed form of a record's layout, which is
what the product computes.  The reader follows LongWordBitReader (:852-990) and EliasFanoSuccessorReader (:1055-1160): next and skip_to.
"""
import numpy as np

M64 = (1 << 64) - 1
SKIPPING_THRESHOLD = 8
END_OF_LIST = (1 << 63) - 1


def msb(x):
    return x.bit_length() - 1                     # Fast.mostSignificantBit: -1 for 0


def ceil_log2(x):
    return (x - 1).bit_length() if x >= 1 else -1                # Fast.ceilLog2 (x <= 2 ? x - 1 : 64 - nlz(x - 1))


def lower_bits(length, upper_bound):              # :140-142
    return 0 if length == 0 else max(0, msb(upper_bound // length))


def pointer_size(length, upper_bound):            # :152-154
    return max(0, ceil_log2(length + (upper_bound >> lower_bits(length, upper_bound))))


def number_of_pointers(length, upper_bound, log2_quantum):   # :165-168
    if length == 0:
        return 0
    return (upper_bound >> lower_bits(length, upper_bound)) >> log2_quantum


class BitCache:
    """LongWordCache as far as the writer needs it: an append-only run of bits, least significant bit first."""

    def __init__(self):
        self.value = 0
        self.length = 0

    def append(self, value, width):
        assert width == 64 or value >> width == 0
        self.value |= value << self.length
        self.length += width

    def write_unary(self, k):
        self.length += k
        self.value |= 1 << self.length
        self.length += 1


class LongWordOutputBitStream:
    """:294-414: a 64-bit buffer whose upper `free` bits are empty; full words go out, close() writes the current one always."""

    def __init__(self):
        self.words = []
        self.buffer = 0
        self.free = 64

    def append(self, value, width):
        self.buffer |= (value << (64 - self.free)) & M64               # value << -free: free is strictly positive
        if width < self.free:
            self.free -= width
        else:
            self.words.append(self.buffer)
            if width == self.free:
                self.buffer = 0
                self.free = 64
            else:
                self.buffer = value >> self.free
                self.free = 64 - width + self.free
        return width

    def append_cache(self, cache):
        left, v = cache.length, cache.value
        while left > 0:
            width = min(left, 64)
            self.append(v & ((1 << width) - 1), width)
            v >>= width
            left -= width
        return cache.length

    def write_gamma(self, value):                 # :394-406
        value += 1
        m = msb(value)
        unary = 1 << m
        self.append(unary, m + 1)
        self.append(value ^ unary, m)
        return 2 * m + 1

    def close(self):
        self.words.append(self.buffer)
        return self.words


class Accumulator:
    """:416-540 with strict = false, indexZeroes = true, as store() calls it (:803)."""

    def init(self, length, upper_bound, log2_quantum):
        self.log2_quantum = log2_quantum
        self.length = length
        self.quantum = 1 << log2_quantum
        self.successors, self.lower, self.upper = BitCache(), BitCache(), BitCache()
        self.corrected_upper_bound = upper_bound
        corrected_length = length + 1
        self.current_prefix_sum = 0
        self.current_length = 0
        self.last_one_position = -1
        self.l = lower_bits(corrected_length, upper_bound)
        self.lower_mask = (1 << self.l) - 1
        self.pointer_size = pointer_size(corrected_length, upper_bound)
        self.expected_pointers = number_of_pointers(corrected_length, upper_bound, log2_quantum)

    def add(self, x):
        if self.current_length != 0 and x == 0:
            raise ValueError("duplicate")
        self.current_prefix_sum += x
        if self.current_prefix_sum > self.corrected_upper_bound:
            raise ValueError("too large a prefix sum")
        if self.l != 0:
            self.lower.append(self.current_prefix_sum & self.lower_mask, self.l)
        one_position = (self.current_prefix_sum >> self.l) + self.current_length
        self.upper.write_unary(one_position - self.last_one_position - 1)
        zeroes_before = self.last_one_position - self.current_length + 1
        position = self.last_one_position + (zeroes_before & -self.quantum) + self.quantum - zeroes_before
        while position < one_position:
            self.successors.append(position + 1, self.pointer_size)
            position += self.quantum
            zeroes_before += self.quantum
        self.last_one_position = one_position
        self.current_length += 1

    def dump(self, out):
        assert self.current_length == self.length
        self.add(self.corrected_upper_bound - self.current_prefix_sum)
        assert self.pointer_size == 0 or self.successors.length // self.pointer_size == self.expected_pointers
        return out.append_cache(self.successors) + out.append_cache(self.lower) + out.append_cache(self.upper)


def words_to_bytes(words, byteorder="LITTLE_ENDIAN"):
    return np.array(words, dtype=np.uint64).astype("<u8" if byteorder == "LITTLE_ENDIAN" else ">u8").tobytes()


def bytes_to_words(data, byteorder="LITTLE_ENDIAN"):
    return [int(w) for w in np.frombuffer(bytes(data), dtype="<u8" if byteorder == "LITTLE_ENDIAN" else ">u8")]


def store(lists, upper_bound=None, log2_quantum=8, byteorder="LITTLE_ENDIAN"):
    """EFGraph.store (:773-820): (graph bytes, offsets[n + 1], {bitsforoutdegrees, bitsforsuccessors, arcs})."""
    n = len(lists)
    upper_bound = n if upper_bound is None else upper_bound
    out = LongWordOutputBitStream()
    acc = Accumulator()
    offsets = [0]
    bits_deg = bits_succ = arcs = 0
    for succ in lists:
        d = len(succ)
        arcs += d
        last = 0
        gb = out.write_gamma(d)
        bits_deg += gb
        acc.init(d, upper_bound, log2_quantum)
        for s in succ:
            acc.add(int(s) - last)
            last = int(s)
        sb = acc.dump(out)
        bits_succ += sb
        offsets.append(offsets[-1] + gb + sb)
    words = out.close()
    return words_to_bytes(words, byteorder), np.array(offsets, dtype=np.uint64), {"bitsforoutdegrees": bits_deg, "bitsforsuccessors": bits_succ, "arcs": arcs}


def write_delta_offsets(offsets):
    """basename.offsets: the delta-coded gaps, MSB first, the first being 0 (:785, :812; OutputBitStream.writeLongDelta)."""
    bits = []

    def gamma(x):
        x += 1
        m = msb(x)
        bits.extend([0] * m + [1] + [(x >> i) & 1 for i in range(m - 1, -1, -1)])

    def delta(x):
        x += 1
        m = msb(x)
        gamma(m)
        bits.extend([(x >> i) & 1 for i in range(m - 1, -1, -1)])

    prev = 0
    delta(0)
    for o in offsets[1:]:
        delta(int(o) - prev)
        prev = int(o)
    bits.extend([0] * (-len(bits) % 8))
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


class LongWordBitReader:
    """:852-990."""

    def __init__(self, words, l):
        self.words, self.l = words, l
        self.mask = (1 << l) - 1
        self.buffer = self.filled = 0
        self.curr = -1

    def position(self, position):
        self.curr = position >> 6
        self.buffer = self.words[self.curr] >> (position & 63)
        self.filled = 64 - (position & 63)
        return self

    def tell(self):
        return self.curr * 64 + 64 - self.filled

    def extract_internal(self, width):
        if width <= self.filled:
            r = self.buffer & ((1 << width) - 1)
            self.filled -= width
            self.buffer >>= width
            return r
        r = self.buffer
        self.curr += 1
        self.buffer = self.words[self.curr]
        rem = width - self.filled
        r |= (self.buffer & ((1 << rem) - 1)) << self.filled
        self.buffer >>= rem
        self.filled = 64 - rem
        return r

    def extract(self):
        return self.extract_internal(self.l)

    def extract_at(self, position):
        self.position(position)
        return self.extract_internal(self.l)

    def read_unary(self):
        acc = 0
        while True:
            if self.buffer != 0:
                t = (self.buffer & -self.buffer).bit_length() - 1
                self.filled -= t + 1
                self.buffer >>= t + 1
                return t + acc
            acc += self.filled
            self.curr += 1
            self.buffer = self.words[self.curr]
            self.filled = 64

    def read_gamma(self):
        m = self.read_unary()
        return (self.extract_internal(m) | (1 << m)) - 1


class SuccessorReader:
    """EliasFanoSuccessorReader (:1017-1166)."""

    def __init__(self, n, upper_bound, words, outdegree, skip_pointers_start, log2_quantum, use_pointers=True):
        self.n, self.words, self.outdegree, self.log2_quantum = n, words, outdegree, log2_quantum
        self.quantum = 1 << log2_quantum
        self.skip_pointers_start = skip_pointers_start
        self.l = lower_bits(outdegree + 1, upper_bound)
        self.number_of_pointers = number_of_pointers(outdegree + 1, upper_bound, log2_quantum)
        self.pointer_size = pointer_size(outdegree + 1, upper_bound)
        self.lower_bits_start = skip_pointers_start + self.pointer_size * self.number_of_pointers
        self.upper_bits_start = self.lower_bits_start + self.l * (outdegree + 1)
        self.skip_pointers = LongWordBitReader(words, self.pointer_size) if self.number_of_pointers and use_pointers else None
        self.lower = LongWordBitReader(words, self.l).position(self.lower_bits_start)
        self.current_index = 0
        self._position(self.upper_bits_start)
        self.last = None                          # Long.MIN_VALUE

    def _position(self, position):
        self.curr = position >> 6
        self.window = self.words[self.curr] & (M64 << (position & 63)) & M64

    def _next_upper(self):
        while self.window == 0:
            self.curr += 1
            self.window = self.words[self.curr]
        t = (self.window & -self.window).bit_length() - 1
        upper = self.curr * 64 + t - self.current_index - self.upper_bits_start
        self.current_index += 1
        self.window &= self.window - 1
        return upper

    def next(self):
        if self.current_index >= self.outdegree:
            self.last = END_OF_LIST
            return -1
        self.last = self._next_upper() << self.l | self.lower.extract()
        return self.last

    def skip_to(self, lower_bound):
        """:1098-1160; the result is defined on the d real successors only: the smallest one >= lower_bound, or -1 (the reference
        compares the terminator with n, :1106, :1157, and so hands out a terminator upper_bound != n as if it were a successor)."""
        if self.last is not None and lower_bound <= self.last:
            return -1 if self.last == END_OF_LIST else self.last
        zeroes_to_skip = lower_bound >> self.l
        delta = zeroes_to_skip - ((0 if self.last is None else self.last) >> self.l)
        assert delta >= 0
        if delta < SKIPPING_THRESHOLD:
            while True:
                self.next()
                if not self.last < lower_bound:
                    break
            return -1 if self.last == END_OF_LIST else self.last
        if delta > self.quantum and self.skip_pointers is not None:
            block = zeroes_to_skip >> self.log2_quantum
            assert 0 < block <= self.number_of_pointers
            skip = self.skip_pointers.extract_at(self.skip_pointers_start + (block - 1) * self.pointer_size)
            assert skip != 0
            self._position(self.upper_bits_start + skip)
            self.current_index = skip - (block << self.log2_quantum)
            delta = zeroes_to_skip - self.curr * 64 + self.current_index + self.upper_bits_start
        assert delta >= 0
        while True:
            bit_count = bin(~self.window & M64).count("1")
            if not bit_count < delta:
                break
            self.curr += 1
            self.window = self.words[self.curr]
            delta -= bit_count
            self.current_index += 64 - bit_count
        if delta != 0:
            delta -= 1
            word, select, seen = ~self.window & M64, 0, 0
            while True:                           # the broadword select of :1132-1146: the position of the delta-th zero (from 0)
                if (word >> select) & 1:
                    if seen == delta:
                        break
                    seen += 1
                select += 1
            self.window &= (M64 << select) & M64
            self.current_index += select - delta
        if self.current_index >= self.outdegree:  # only the terminator is left: no successor is that large
            self.last = END_OF_LIST
            return -1
        lower = self.lower.extract_at(self.lower_bits_start + self.l * self.current_index)
        self.last = self._next_upper() << self.l | lower
        while True:
            if self.last >= lower_bound:
                return -1 if self.last == END_OF_LIST else self.last
            self.next()


class Graph:
    """EFGraph as loaded (:675-750): the words, the offsets, outdegree (:1009-1014) and successors (:1169-1171)."""

    def __init__(self, n, upper_bound, log2_quantum, data, offsets, byteorder="LITTLE_ENDIAN"):
        self.n, self.upper_bound, self.log2_quantum = n, upper_bound, log2_quantum
        self.words = bytes_to_words(data, byteorder) + [0, 0]
        self.offsets = [int(o) for o in offsets]

    def reader(self, x, use_pointers=True):
        r = LongWordBitReader(self.words, 0).position(self.offsets[x])
        d = r.read_gamma()
        return SuccessorReader(self.n, self.upper_bound, self.words, d, r.tell(), self.log2_quantum, use_pointers)

    def outdegree(self, x):
        return self.reader(x).outdegree

    def successors(self, x):
        r, out = self.reader(x), []
        while True:
            s = r.next()
            if s == -1:
                return out
            out.append(s)

    def skip_to(self, x, bound, use_pointers=True):
        return self.reader(x, use_pointers).skip_to(bound)


def record_bits(d, upper_bound, log2_quantum):
    """The closed form the product uses (kept apart from the writer above, which the tests hold it against)."""
    L = d + 1
    l = lower_bits(L, upper_bound)
    return 2 * msb(d + 1) + 1 + number_of_pointers(L, upper_bound, log2_quantum) * pointer_size(L, upper_bound) + L * l + (upper_bound >> l) + d + 1


def arc_mix(x, y):
    """bvg_arc_mix (include/bvgraph_hip.h)."""
    m32 = 0xFFFFFFFF
    h = ((x & m32) * 0x9E3779B1 + (x >> 32) * 0x85EBCA77) & m32
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & m32
    h ^= h >> 12
    k1 = h | 1
    k0 = (h * 0x297A2D39) & m32
    k0 ^= k0 >> 15
    return (k1 * y + k0) & M64


def scan_checksum(lists):
    return sum(arc_mix(x, int(y)) for x, l in enumerate(lists) for y in l) & M64


def random_lists(n, arcs, seed, degrees=()):
    """n sorted duplicate-free lists over [0, n) with about `arcs` arcs; degrees: outdegrees forced onto the first nodes."""
    rng = np.random.default_rng(seed)
    out = []
    for x in range(n):
        d = degrees[x] if x < len(degrees) else int(rng.poisson(arcs / max(n, 1)))
        d = min(d, n)
        out.append(np.sort(rng.choice(n, size=d, replace=False)).astype(np.int64) if d else np.empty(0, np.int64))
    return out
