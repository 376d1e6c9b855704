"""Text graph rates (reported, not gated), on cnr-2000 tiled on the device (argument: copies, default 8): format of an ASCIIGraph text and
of an arc list, parse of both from host memory (upload included), and the store of the parsed graph.  The arc list is parsed as written
(sources and targets in order) and with its lines shuffled: BOTH run the two radix sorts, the pair shows what the order of the input is
worth to them, not the cost of the sort; the ASCIIGraph parse is the same token pass without any sort.
The host baseline is CONSTRUCTED HERE: the repository holds no text reader outside the test suite (tooling/ takes adjacencies, not text),
so the last line times what tests/conftest.py does to get an adjacency -- one process splitting the lines and converting the numbers."""
import os, sys, time
sys.path.insert(0, '.')
import numpy as np
import webgraph_big_amd as W

copies = int(sys.argv[1]) if len(sys.argv) > 1 else 8
base = W.BVGraph.load(os.path.join('tests', 'golden', 'cnr-2000'))
g = base.tile(copies)
n, arcs = g.num_nodes(), g.num_arcs()


def best(f, reps=3):
    out, dt = None, 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); out = f(); dt = min(dt, time.perf_counter() - t0)
    return out, dt


def line(what, nbytes, dt):
    print('%-34s %8.1f MB %8.2f ms %7.2f GB/s %8.1f M arcs/s' % (what, nbytes / 1e6, dt * 1e3, nbytes / dt / 1e9, arcs / dt / 1e6))


ascii_text, dt = best(lambda: g.format_ascii(0, n)); line('format ASCIIGraph (to host)', len(ascii_text), dt)
arc_text, dt = best(lambda: g.format_arcs(0, n)); line('format arc list (to host)', len(arc_text), dt)
text = b'%d\n' % n + ascii_text
_, dt = best(lambda: W.parse_ascii_graph(text).close()); line('parse ASCIIGraph (from host)', len(text), dt)
_, dt = best(lambda: W.parse_arc_list(arc_text).close()); line('parse arc list, input in order', len(arc_text), dt)
lines = np.array(arc_text.split(b'\n')[:-1], dtype=object)
shuffled = b'\n'.join(lines[np.random.default_rng(0).permutation(len(lines))].tolist()) + b'\n'
_, dt = best(lambda: W.parse_arc_list(shuffled).close()); line('parse arc list, lines shuffled', len(shuffled), dt)
with W.parse_ascii_graph(text) as pg:
    _, dt = best(lambda: pg.store(None, 1 << 16), 1); line('store parsed graph (BVGraph)', len(text), dt)


def host_route():
    rows = text.split(b'\n')
    return [np.array(l.split(), dtype=np.int64) for l in rows[1:int(rows[0]) + 1]]


_, dt = best(host_route, 1); line('host (built here): split, int64', len(text), dt)
