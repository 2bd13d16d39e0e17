"""Inputs the rtc_leiden tests share (tests/test_cpu_leiden_refine.py, tests/test_gpu_leiden_refine.py): hand graphs small enough
to check on paper, and one set of about 2 500 vertices whose rows take every kernel path."""
import numpy as np

ONE = 1 << 20


def clique(vs, q):
    vs = list(vs)
    return [(a, b, q) for i, a in enumerate(vs) for b in vs[i + 1:]]


def two_cliques():
    """two 4-cliques of unit weights joined by one light edge"""
    return 8, clique(range(4), ONE) + clique(range(4, 8), ONE) + [(3, 4, ONE // 64)]


def path(n=9):
    """a path of equal weights"""
    return n, [(i, i + 1, ONE) for i in range(n - 1)]


def pendant():
    """a 5-clique of unit weights and vertex 5 hanging on vertex 0 by an edge of half a unit.  CPM at resolution 0.25: in round 0
    every vertex joins community 0 (vertex 5 gains 0.5 - 0.25); in the refinement vertex 5 holds 0.5 towards a community of
    5 others, below 0.25 * 5, and is not eligible, so the clique merges without it"""
    return 6, clique(range(5), ONE) + [(0, 5, ONE // 2)]


def hand_graphs():
    return {"two_cliques": two_cliques(), "path": path(), "pendant": pendant()}


_BIG = {}


def paths_set():
    """About 2 500 vertices.  Cliques of 5..40 members (rows of one wave), light bridges between consecutive cliques, three
    vertices tied to 150..700 others (rows of 129..2 048 entries: the workgroup's table in LDS) and one hub tied to 2 150 (the
    table in global memory)."""
    if not _BIG:
        rng = np.random.default_rng(4242)
        edges = []
        first = []
        n = 0
        while n < 2400:
            size = int(rng.integers(5, 41))
            first.append(n)
            for a in range(n, n + size):
                for b in range(a + 1, n + size):
                    edges.append((a, b, int(rng.integers(ONE // 2, ONE))))
            n += size
        for a, b in zip(first, first[1:]):
            edges.append((a + 1, b, int(rng.integers(ONE // 64, ONE // 16))))
        for deg in (150, 400, 700):
            for y in rng.choice(n, size=deg, replace=False).tolist():
                edges.append((n, y, int(rng.integers(ONE // 512, ONE // 128))))
            n += 1
        for y in rng.choice(n, size=2150, replace=False).tolist():
            edges.append((n, y, int(rng.integers(ONE // 2048, ONE // 512))))
        n += 1
        _BIG["n"], _BIG["edges"] = n, edges
    return _BIG["n"], _BIG["edges"]


_RANDOM = {}


def random_graph():
    """300 vertices in 20 planted blocks by residue: about 2 300 distinct pairs, no self record, every weight at most one unit
    (so CPM at resolution 1 or above moves nothing)"""
    if not _RANDOM:
        rng = np.random.default_rng(78)
        n, m = 300, 5000
        u = rng.integers(0, n, size=m)
        v = np.where(rng.random(m) < 0.9, u % 20 + 20 * rng.integers(0, 15, size=m), rng.integers(0, n, size=m))
        q = rng.integers(ONE // 2, ONE + 1, size=m)
        seen = {}
        for a, b, w in zip(u.tolist(), v.tolist(), q.tolist()):
            if a != b:
                seen.setdefault((min(a, b), max(a, b)), w)
        _RANDOM["n"], _RANDOM["edges"] = n, [(a, b, w) for (a, b), w in seen.items()]
    return _RANDOM["n"], _RANDOM["edges"]
