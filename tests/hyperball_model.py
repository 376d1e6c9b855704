"""A numpy model of HyperBall's standard (non-systolic, in-memory) iterations with this library's hash: what the device code is compared
against.  It restates include/bvgraph_hip.h: counters of m = 2^log2m one-byte registers, init adds node i to counter i, an iteration takes
the register-wise maximum over the successors modified by the previous one, counts, and accumulates the float32 centralities."""
import numpy as np

MASK = (1 << 64) - 1
BETA = {4: 1.106, 5: 1.070, 6: 1.054, 7: 1.046}


def relative_standard_deviation(log2m):
    return BETA.get(log2m, 1.04) / np.sqrt(float(1 << log2m))


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def hash_node(v, seed, log2m):
    """(register index, register value) of node v."""
    x = mix64((v + (seed + 1) * 0x9E3779B97F4A7C15) & MASK)
    y = (x >> log2m) | (1 << (64 - log2m))
    return x & ((1 << log2m) - 1), (y & -y).bit_length()          # ctz(y) + 1


def alpha_mm(log2m):
    m = float(1 << log2m)
    alpha = {4: 0.673, 5: 0.697, 6: 0.709}.get(log2m, 0.7213 / (1 + 1.079 / m))
    return alpha * m * m


def count(regs, log2m):
    """The HyperLogLog estimate of every row of regs (uint8[k, m]): the sum of 2^-register from a histogram of the register values, added
    from the largest value down, in double."""
    regs = np.atleast_2d(regs)
    m = float(1 << log2m)
    s = np.zeros(len(regs), dtype=np.float64)
    zeroes = np.zeros(len(regs), dtype=np.float64)
    for v in range(int(regs.max()) if regs.size else 0, -1, -1):
        h = (regs == v).sum(axis=1).astype(np.float64)
        s += h * 2.0 ** -v
        if v == 0:
            zeroes = h
    e = alpha_mm(log2m) / s
    small = (zeroes > 0) & (e < 2.5 * m)
    with np.errstate(divide="ignore"):
        e[small] = m * np.log(m / zeroes[small])
    return e


def adjacency(lists, n=None):
    """(off uint64[n + 1], succ int64[arcs]) of a list of successor lists."""
    n = len(lists) if n is None else n
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
    succ = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if n and off[-1] else np.empty(0, np.int64)
    return off, succ


class HyperBallModel:
    def __init__(self, off, succ, log2m, seed=0, sum_of_distances=False, harmonic=False, chunk=1 << 18):
        self.n = len(off) - 1
        self.log2m, self.m, self.seed = log2m, 1 << log2m, seed
        deg = np.diff(np.asarray(off, dtype=np.int64))
        self.src = np.repeat(np.arange(self.n, dtype=np.int64), deg)
        self.dst = np.asarray(succ, dtype=np.int64)
        self.do_sod, self.do_sid = sum_of_distances, harmonic
        self.chunk = chunk
        self.inited = False

    def init(self, seed=None):
        self.seed = self.seed if seed is None else seed
        self.regs = np.zeros((self.n, self.m), dtype=np.uint8)
        for v in range(self.n):
            j, r = hash_node(v, self.seed, self.log2m)
            self.regs[v, j] = max(self.regs[v, j], r)
        self.mod = np.ones(self.n, dtype=bool)
        self.iteration, self.modified, self.relative_increment = -1, self.n, 0.0
        self.nf = [float(self.n)]
        self.sod = np.zeros(self.n, dtype=np.float32)
        self.sid = np.zeros(self.n, dtype=np.float32)
        self.passed = 0
        self.inited = True

    def iterate(self):
        assert self.inited
        self.iteration += 1
        cur = self.regs
        keep = (self.dst != self.src) & self.mod[self.dst]
        src, dst = self.src[keep], self.dst[keep]
        self.passed = int(keep.sum())
        t = cur.copy()
        for a in range(0, len(src), self.chunk):
            s, d = src[a:a + self.chunk], dst[a:a + self.chunk]
            heads = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
            red = np.maximum.reduceat(cur[d], heads, axis=0)
            t[s[heads]] = np.maximum(t[s[heads]], red)
        changed = (t != cur).any(axis=1)
        post = count(t, self.log2m) if self.n else np.zeros(0)
        if (self.do_sod or self.do_sid) and changed.any():
            idx = np.flatnonzero(changed)
            delta = post[idx] - count(cur[idx], self.log2m)
            pos = delta > 0
            idx, delta = idx[pos], delta[pos]
            k = float(self.iteration + 1)
            if self.do_sod:
                self.sod[idx] = self.sod[idx] + (delta * k).astype(np.float32)
            if self.do_sid:
                self.sid[idx] = self.sid[idx] + (delta / k).astype(np.float32)
        self.regs, self.mod, self.modified = t, changed, int(changed.sum())
        self.post = post
        current = float(np.sum(post)) if self.n else 0.0
        last = self.nf[-1]
        if current < last:
            current = last
        self.relative_increment = current / last if last else float("nan")
        self.nf.append(current)

    def run(self, upper_bound=-1, threshold=-1.0):
        ub = self.n if upper_bound < 0 else min(upper_bound, self.n)
        self.init()
        for i in range(ub):
            self.iterate()
            if self.modified == 0:
                break
            if i > 3 and self.relative_increment < 1 + threshold:
                break

    def counts(self):
        return count(self.regs, self.log2m)

    # the centralities of the reference's main
    def closeness(self):
        with np.errstate(divide="ignore"):
            return np.where(self.sod == 0, np.float32(0), np.float32(1) / self.sod).astype(np.float32)

    def lin(self):
        c = self.counts()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.sod == 0, np.float32(1), (c * c / self.sod.astype(np.float64)).astype(np.float32)).astype(np.float32)

    def nieminen(self):
        c = self.counts()
        return (c * c - self.sod.astype(np.float64)).astype(np.float32)

    def reachable(self):
        return self.counts().astype(np.float32)


def exact_neighbourhood_function(lists):
    """N(t) = the pairs (x, y) with d(x, y) <= t, for t = 0 .. the largest finite distance, by one breadth-first visit per node."""
    n = len(lists)
    per_dist = np.zeros(n + 1, dtype=np.int64)
    for x in range(n):
        dist = {x: 0}
        frontier = [x]
        d = 0
        while frontier:
            per_dist[d] += len(frontier)
            d += 1
            nxt = []
            for u in frontier:
                for v in lists[u]:
                    v = int(v)
                    if v not in dist:
                        dist[v] = d
                        nxt.append(v)
            frontier = nxt
    last = int(np.flatnonzero(per_dist)[-1]) if n else 0
    return np.cumsum(per_dist[:last + 1]).astype(np.float64)


# ---- the small graphs of the tests
def clique(n):
    return [[y for y in range(n) if y != x] for x in range(n)]


def cycle(n):
    return [[(x + 1) % n] for x in range(n)]


def line(n):
    return [[x + 1] if x + 1 < n else [] for x in range(n)]


def out_tree(n):
    return [[c for c in (2 * x + 1, 2 * x + 2) if c < n] for x in range(n)]


def random_graph(n, avg, seed):
    rng = np.random.RandomState(seed)
    return [sorted(set(int(y) for y in rng.randint(0, n, rng.poisson(avg)))) for _ in range(n)]
