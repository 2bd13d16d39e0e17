"""The matrices of the neighbour-joining tests (tests/test_cpu_nj.py, tests/test_gpu_nj.py)."""
import functools

import numpy as np

from tests import linkage_sets as S

# 2: the one-record case; 3: the last record alone; 4, 5: the first joins; 63, 64: the wave path and its last size; 65: the
# workgroup path's first; 256, 257: one turn of 256 lanes and past it; 300
ADDITIVE_SIZES = (2, 3, 4, 5, 63, 64, 65, 256, 257, 300)
CASE_SIZES = (5, 64, 65, 257, 300)
CASE_NAMES = ("all_equal", "random_ties", "star", "chain", "tie_free")


@functools.lru_cache(maxsize=None)
def additive(m, seed=0):
    """(D, splits): a random unrooted binary tree of m leaves grown by leaf insertion -- leaf t lands on a branch drawn uniformly
    from those present -- with integer branch lengths 1..9, its leaf-to-leaf path lengths as doubles, and its branches as a
    sorted list of (split, length), split the leaf set away from leaf 0 as a bit mask (refnj.splits gives the same of records).
    Every value neighbour joining forms on such a matrix is an integer or a half-integer, so the records are exact on any
    evaluation order and the tree comes back with every length."""
    assert m >= 2
    rng = np.random.default_rng(1000 * m + seed)
    edges = [(0, 1)]
    inner = m
    for t in range(2, m):
        u, v = edges.pop(int(rng.integers(len(edges))))
        edges += [(u, inner), (inner, v), (inner, t)]
        inner += 1
    n_nodes = inner
    length = rng.integers(1, 10, size=len(edges))
    adj = [[] for _ in range(n_nodes)]
    for (u, v), ln in zip(edges, length.tolist()):
        adj[u].append((v, ln))
        adj[v].append((u, ln))
    # nodes outwards from leaf 0; the path lengths to everything seen so far come from the parent's
    parent, plen, seen = {0: None}, {0: 0}, [0]
    for u in seen:
        for v, ln in adj[u]:
            if v not in parent:
                parent[v], plen[v] = u, ln
                seen.append(v)
    dn = np.zeros((n_nodes, n_nodes), dtype=np.float64)
    for at, v in enumerate(seen[1:], 1):
        before = np.asarray(seen[:at])
        dn[v, before] = dn[parent[v], before] + plen[v]
        dn[before, v] = dn[v, before]
    under = [1 << v if v < m else 0 for v in range(n_nodes)]
    for v in reversed(seen[1:]):
        under[parent[v]] |= under[v]
    D = np.ascontiguousarray(dn[:m, :m])
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    return D, sorted((under[v], float(plen[v])) for v in seen[1:])


@functools.lru_cache(maxsize=None)
def case(name, m, kmer_size=21):
    """a key matrix of linkage_sets as distances (rtc_linkage_distance; keys of common 0 or denom 0 at exactly 1.0): all_equal --
    every Q ties; random_ties -- few distinct values; star and chain -- graded values; tie_free; none of them additive, so
    negative branch lengths and inexact sums occur"""
    from rabbittclust_amd import api
    keys = S.CASES[name](m)
    D = np.zeros((m, m), dtype=np.float64)
    memo = {}
    for i in range(m):
        for j in range(i):
            c, d = int(keys[i, j, 0]), int(keys[i, j, 1])
            if (c, d) not in memo:
                memo[(c, d)] = 1.0 if c == 0 or d == 0 else api.linkage_distance(c, d, kmer_size)
            D[i, j] = D[j, i] = memo[(c, d)]
    return D
