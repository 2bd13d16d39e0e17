"""Sketch sets for the clust-greedy --order degree tests (tests/refgreedy_degree.py is the yardstick): the eps sweep's families,
MinHash families with short sketches, a path, small graphs that isolate one rule of the definition each, a clique of 4 200 and
a member with more than 4 096 candidate representatives."""
import numpy as np

from tests import sweep_sets

KMER = 21
FAMILY_THRESHOLD = 0.02   # between the sweep families' second and third substitution rate (tests/sweep_sets.py)
GRAPH_THRESHOLD = 0.1     # jaccard_min 0.0652: every pair of graph_sketches that shares hashes is a neighbour (checked by the sets)


def families(seed, use64, n_empty):
    return sweep_sets.family_sets(seed, use64, n_empty=n_empty)


def minhash_families(seed, s=128, n_fam=8, per=6):
    """Genomes as sets of 300 hashes (a family's members replace a share of its base), some with 70 only; a sketch is the s
    smallest, so the short genomes' sketches are shorter than s.  Ordered by genome size, as the command line leaves them."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_fam):
        base = rng.choice(1 << 40, size=300, replace=False)
        for m in range(per):
            g = base.copy()
            flip = rng.random(300) < rng.choice([0.01, 0.05, 0.15, 0.4])
            g[flip] = rng.choice(1 << 40, size=int(flip.sum()), replace=False)
            if (f + m) % 5 == 0:
                g = np.sort(g)[:70]  # a short genome: it keeps the low end, so it still shares hashes with its family
            out.append(np.unique(g))
    out.sort(key=lambda g: -len(g))
    sk = [g[:s].astype(np.uint64) for g in out]
    assert any(len(x) < s for x in sk) and any(len(x) == s for x in sk)
    return sk


def path(n=2000, block=8, dtype=np.uint32):
    """genome i = block i and block i + 1 of `block` private hashes each: only neighbours in the path share hashes, j = 1 / 3"""
    return [np.arange(1000 + block * i, 1000 + block * (i + 2), dtype=dtype) for i in range(n)]


def graph_sketches(n, edges, private=None, dtype=np.uint32):
    """A sketch per vertex: every edge (u, v, c) gives u and v c hashes no other sketch has, private[v] more belong to v alone.
    Vertices that are not joined share nothing."""
    nxt = 1000
    sets = [[] for _ in range(n)]
    for u, v, c in edges:
        sets[u] += range(nxt, nxt + c)
        sets[v] += range(nxt, nxt + c)
        nxt += c
    for v, c in (private or {}).items():
        sets[v] += range(nxt, nxt + c)
        nxt += c
    return [np.array(sorted(s), dtype=dtype) for s in sets]


def star_and_clique():
    """a star (centre 3, leaves 0 1 2 4 5) and a clique (6 .. 10): the centre and the clique's lowest index are the representatives"""
    edges = [(3, v, 4) for v in (0, 1, 2, 4, 5)] + [(u, v, 3) for u in range(6, 11) for v in range(u + 1, 11)]
    return graph_sketches(11, edges), edges


def two_hubs():
    """hubs 2 and 5, neighbours of each other, three leaves each: equal degrees, so 2 is the representative and 5 a member; the
    leaves of 5 then have no representative next to them and become representatives themselves"""
    edges = [(2, 5, 6)] + [(2, v, 3) for v in (0, 1, 3)] + [(5, v, 3) for v in (4, 6, 7)]
    return graph_sketches(8, edges), edges


def tie_in_j():
    """member 2 between representative 1 (degree 4: 2 / 12) and representative 0 (degree 3: 4 / 24): the same j from other counts.
    1 is earlier in the order (the higher degree), though 0 has the lower index and the larger common."""
    edges = [(2, 1, 2), (2, 0, 4)] + [(1, v, 2) for v in (3, 4, 5)] + [(0, v, 2) for v in (6, 7)]
    sk = graph_sketches(8, edges, private={0: 14})
    assert [len(sk[v]) for v in (0, 1, 2)] == [22, 8, 6]
    return sk, edges


def both_sides():
    """member 2 between representatives 0 (2 / 14) and 1 (6 / 12), both of degree 3: it joins 1, the more similar one, though 0
    comes first in the order"""
    edges = [(2, 0, 2), (2, 1, 6)] + [(0, v, 3) for v in (3, 4)] + [(1, v, 2) for v in (5, 6)]
    sk = graph_sketches(7, edges)
    assert [len(sk[v]) for v in (0, 1, 2)] == [8, 10, 8]
    return sk, edges


def clique_4200(n=4200):
    """4 200 sketches of 4 hashes that all share 2 of them: every pair has j = 2 / 6, a clique of 8 817 900 pairs"""
    return [np.array([1, 2, 10 + 2 * i, 11 + 2 * i], dtype=np.uint32) for i in range(n)]


LONG_ROW_LEAVES = 4097
LONG_ROW_THRESHOLD = 0.4  # with k 21: jaccard_min 1.1e-4, below a leaf's 2 / (|hub| + 2) = 2.4e-4


def long_row(leaves=LONG_ROW_LEAVES):
    """A member with more than 4 096 representatives next to it.  A representative r0 of that member m must come before it, so
    degree(r0) >= degree(m) > 4 096, and r0's neighbours are no representatives: no set of fewer than 2 * 4 097 genomes has such
    a row.  Here: hubs 0 and 1, neighbours of each other, with `leaves` leaves each (a leaf shares 2 of its 4 hashes with its
    hub and nothing else).  Equal degrees: 0 is the representative, 1 its member, the leaves of 0 are members with one
    candidate, and the leaves of 1, with no representative next to them, are representatives -- 1 has leaves + 1 candidates."""
    n = 2 + 2 * leaves
    edges = [(0, 1, 64)] + [(0, 2 + i, 2) for i in range(leaves)] + [(1, 2 + leaves + i, 2) for i in range(leaves)]
    sk = graph_sketches(n, edges, private={v: 2 for v in range(2, n)})
    assert all(len(s) == 4 for s in sk[2:]) and len(sk[0]) == len(sk[1]) == 64 + 2 * leaves
    return sk, edges


def dense_candidates(n=600, dtype=np.uint32):
    """every sketch shares one hash with every other (the candidate list is the whole triangle); seven families besides"""
    rng = np.random.default_rng(3)
    sets = []
    for g in range(n):
        body = (100_000 * (g % 7) + np.arange(60))[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, 10_000_000 + 1000 * g + np.arange(5)])).astype(dtype))
    return sets


def edges_to_lists(n, edges):
    nbrs = [[] for _ in range(n)]
    for u, v, _ in edges:
        nbrs[u].append(v)
        nbrs[v].append(u)
    return [sorted(x) for x in nbrs]
