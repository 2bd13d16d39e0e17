"""Plain-Python restatement of rtc_dbscan_update's two-stage rule (include/rtclust.h): a clustered set of n_old
points, labels and core flags as the full run gives them, and points [n_old, n) added.  The neighbour relation comes as a
function nbr(p, q) of two indices and is evaluated ONLY for the rows of stage 1 (the new points against everything below
them) and of stage 2 (T u B against the old points); `update` returns those row sets with the result, and the events the crafted
sets of the tests are built for.  kssd_relation / mash_relation are the two kinds' relations, one pair at a time, restated
from tests/refdbscan.py and tests/refdbscan_mash.py; graph_sketches builds sketches whose relation is a given graph."""
import math

import numpy as np

from tests import refdbscan as R
from tests import refdbscan_mash as M


def kssd_relation(sketches, eps, kmer_size, use64):
    """findNeighborsKSSDWithIndex's test of candidate q for reference point p (tests/refdbscan.neighbour_lists): the u64 brute
    force has no emptiness test, the u32 index never lists a pair without a common hash and saturates the count at 65 535."""
    t = R.jaccard_min(eps, kmer_size)
    sets = [set(np.asarray(s).tolist()) for s in sketches]
    sizes = [len(s) for s in sets]

    def nbr(p, q):
        a, b = sizes[p], sizes[q]
        if not use64 and (a == 0 or b == 0):
            return False
        if b < math.floor(t * a) or b > math.ceil(float(a) / t):
            return False
        common = len(sets[p] & sets[q])
        if not use64:
            if common == 0:
                return False
            common = min(common, 65535)
        return not (float(common) * (1.0 + t) + 1e-12 < t * float(a) + t * float(b))
    return nbr


def mash_relation(sketches, sketch_size, eps, kmer_size):
    """findNeighborsMinHash's test: the union-truncated distance <= eps"""
    arrs = [np.asarray(s) for s in sketches]
    sets = [set(a.tolist()) for a in arrs]
    memo = {}

    def nbr(p, q):
        if sets[p].isdisjoint(sets[q]):
            return eps >= 1.0  # no common hash: distance 1
        key = (min(p, q), max(p, q))
        if key not in memo:
            memo[key] = M.distance(*M.mash_counts_sets(arrs[key[0]], arrs[key[1]], sketch_size), kmer_size) <= eps
        return memo[key]
    return nbr


def need_of(min_pts, minhash):
    """the neighbours a core point has at least: KssdDBSCAN counts the point itself, MinHashDBSCAN does not"""
    return max(min_pts, 0) if minhash else min_pts - 1


def update(n_old, n, nbr, labels_old, core_old, need):
    """-> (labels, core, info): info['rows1'] / info['rows2'] the rows of the two stages, info['events'] what happened."""
    labels_old = [int(x) for x in labels_old]
    core_old = [bool(x) for x in core_old]
    edges = set()
    # ---- stage 1: the new points against everything below them ----
    rows1 = list(range(n_old, n))
    for p in rows1:
        for q in range(p):
            if nbr(p, q):
                edges.add((p, q))
    T = {q for (p, q) in edges if q < n_old and labels_old[q] < 0}
    B = {v for v in range(n_old) if not core_old[v] and labels_old[v] >= 0}
    rows2 = sorted(T | B)
    # ---- stage 2: T u B against the old points, every unordered pair once ----
    in2 = set(rows2)
    for p in rows2:
        for q in range(n_old):
            if q == p or (q in in2 and q > p):
                continue
            if nbr(p, q):
                edges.add((max(p, q), min(p, q)))
    # ---- core flags: the old ones, or the count rule where the count is complete ----
    deg = [0] * n
    for p, q in edges:
        deg[p] += 1
        deg[q] += 1
    counted = set(rows1) | in2
    core = [(v < n_old and core_old[v]) or (v in counted and deg[v] >= need) for v in range(n)]
    # ---- components over the seeds and the kept core-core edges ----
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    first = {}
    for v in range(n_old):
        if core_old[v]:
            first.setdefault(labels_old[v], v)
            union(v, first[labels_old[v]])
    for p, q in edges:
        if core[p] and core[q]:
            union(p, q)
    cid, labels = {}, [-1] * n
    for v in range(n):  # in index order: a cluster's number is the rank of its smallest core index
        if core[v]:
            r = find(v)
            if r not in cid:
                cid[r] = len(cid)
            labels[v] = cid[r]
    for p, q in edges:
        for a, b in ((p, q), (q, p)):
            if core[a] and not core[b]:
                labels[b] = labels[a] if labels[b] < 0 else min(labels[b], labels[a])
    # ---- what happened ----
    now_of_old = {labels_old[v]: labels[v] for v in range(n_old) if core_old[v]}  # old cluster -> its number now
    ev = set()
    if any(core[v] for v in T):
        ev.add("noise promoted")
    if any(core[v] for v in B):
        ev.add("border promoted")
    if len(set(now_of_old.values())) < len(now_of_old):
        ev.add("clusters merged")
    if any(not core[v] and labels[v] != now_of_old[labels_old[v]] for v in B) and any(core[v] for v in T | B):
        ev.add("border relabelled")
    if set(labels[v] for v in range(n_old, n) if core[v]) - set(labels[v] for v in range(n_old) if core[v]):
        ev.add("new cluster")
    info = {"rows1": rows1, "rows2": rows2, "events": ev, "promoted": sum(core[v] and not core_old[v] for v in range(n_old)),
            "merged": len(now_of_old) - len(set(now_of_old.values())), "kept": len(edges)}
    return np.array(labels, dtype=np.int32), np.array(core, dtype=bool), info


def graph_sketches(n, edges, rng, size=40, shared=8, use64=False, everywhere=0):
    """Sketches of `size` hashes whose neighbour relation at GRAPH_EPS (k 21, either kind, estimator size >= 2 * size) is exactly
    the graph: the two ends of an edge share a block of `shared` hashes that nothing else holds (jaccard 8 / 72 = 0.111 against
    jaccard_min 0.1), everything else is a sketch's own.  A vertex has at most (size - everywhere) // shared edges.
    everywhere: that many hashes (at most 2) in EVERY sketch, so that every pair is a candidate of the pair phase and none a
    neighbour by them (jaccard 2 / 78)."""
    assert everywhere <= 2
    nxt = int(rng.integers(1 << 20, 1 << 24))
    blocks = [list(range(nxt, nxt + everywhere)) for _ in range(n)]
    nxt += everywhere + 1
    for u, v in edges:
        blk = list(range(nxt, nxt + shared))
        nxt += shared + int(rng.integers(1, 50))
        blocks[u] += blk
        blocks[v] += blk
    out = []
    for v in range(n):
        assert len(blocks[v]) <= size, "vertex %d has too many edges" % v
        own = list(range(nxt, nxt + size - len(blocks[v])))
        nxt += size + int(rng.integers(1, 50))
        out.append(np.array(sorted(blocks[v] + own), dtype=np.uint64 if use64 else np.uint32))
    return out


GRAPH_K = 21
# jaccard_min t = x / (2 - x) with x = exp(-eps k): t = 0.1 at x = 2 / 11.  A little above that eps: t = 0.0993 < 8 / 72
GRAPH_EPS = -math.log(2.0 / 11.0) / GRAPH_K + 0.0005
GRAPH_SKETCH_SIZE = 1000

# ---- crafted sets: (n_old, n, edges, min_pts of the KSSD rule), each built for one event.  The MinHash rule counts the
# neighbours alone, so its min_pts is one less for the same core flags. ----
CRAFTED = {
    # 0-1-2 a path of noise (min_pts 4: a core point needs 3 neighbours); 3, 4 arrive next to 1: 1 becomes a core point
    "noise promoted": (3, 5, [(0, 1), (1, 2), (3, 1), (4, 1)], 4),
    # 0 the centre of a star 1 2 3 (core), 3 a border point with the further neighbour 4 (noise); 5 arrives next to 3
    "border promoted": (5, 6, [(0, 1), (0, 2), (0, 3), (3, 4), (5, 3)], 4),
    # two triangles, 6 arrives next to a point of each and to 7, 8 (arriving too): a core point that joins the clusters
    "clusters merged": (6, 9, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (6, 0), (6, 3), (6, 7), (6, 8)], 3),
    # three new points, a triangle, next to nothing old
    "new cluster": (4, 7, [(0, 1), (4, 5), (4, 6), (5, 6)], 3),
}


def _relabel_case():
    """min_pts 4 (three neighbours make a core point).  Old: star A with centre 4 over 5 6 7, star B with centre 8 over 9 10 7:
    7 is a border point of both and carries A's number 0 (centre 4 < centre 8).  0 is noise with the neighbours 1 (noise) and 9;
    9 is a border point of B; 2 and 3 are alone.  11 arrives next to 0 and 12 next to 9: both become core points, 0 - 9 - 8 is a
    core chain, B's smallest core index becomes 0 and B is numbered before A: 7 now takes B."""
    edges = [(4, 5), (4, 6), (4, 7), (8, 9), (8, 10), (8, 7), (0, 1), (0, 9), (11, 0), (12, 9)]
    return 11, 13, edges, 4


CRAFTED["border relabelled"] = _relabel_case()


def mostly_core_set(rng, use64=False, cliques=20):
    """(sketches, n_old): `cliques` cliques of five (core points at min_pts 3), four of them with a border point hanging on,
    ten pairs and eight loners (noise); eight new points: next to a point of a pair, to a loner, to a clique member, to a border
    point, and two alone.  Stage 2 has the four border points and the few noise points the new ones touch: far below n_old / 4."""
    edges, v = [], 0
    members = []
    for _ in range(cliques):
        ids = list(range(v, v + 5))
        edges += [(a, b) for a in ids for b in ids if b < a]
        members.append(ids)
        v += 5
    borders = []
    for c in range(4):
        edges.append((v, members[c][0]))
        borders.append(v)
        v += 1
    pairs = []
    for _ in range(10):
        edges.append((v + 1, v))
        pairs.append(v)
        v += 2
    loners = list(range(v, v + 8))
    v += 8
    n_old = v
    for target in (pairs[0], pairs[0], pairs[3], loners[1], members[7][2], borders[1]):
        edges.append((v, target))
        v += 1
    v += 2
    return graph_sketches(v, edges, rng, use64=use64), n_old


def family_sets(seed, use64, n_old=300, n_new=60):
    """(sketches, n_old) in the style of tests/sweep_sets.py, n_old + n_new points in shuffled order: families of eight at four
    substitution rates (sketches of 120 .. 200 hashes), a chain of sliding windows, loners and empty sketches."""
    rng = np.random.default_rng(seed)
    n = n_old + n_new

    def fresh(m):
        return rng.integers(1, (1 << 31) - 1, size=m, dtype=np.int64)
    out = []
    chain0 = int(rng.integers(1 << 20, 1 << 30))
    for i in range(16):
        out.append(np.arange(chain0 + 25 * i, chain0 + 25 * i + 100, dtype=np.int64))
    out += [fresh(150) for _ in range(18)] + [np.zeros(0, dtype=np.int64)] * 6
    f = 0
    while len(out) < n:
        size, rate = 120 + 10 * (f % 9), (0.03, 0.15, 0.35, 0.5)[f % 4]
        base = fresh(size)
        for _ in range(min(8, n - len(out))):
            s = base.copy()
            flip = rng.random(size) < rate
            s[flip] = fresh(int(flip.sum()))
            out.append(s)
        f += 1
    out = [out[i] for i in rng.permutation(n)]
    return [np.unique(s).astype(np.uint64 if use64 else np.uint32) for s in out], n_old
