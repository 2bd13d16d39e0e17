"""The exact minimum spanning forest of a candidate list, in plain numpy and Python (no project code): what rtc_msf_dev has to
leave in d_sel, record for record.

The forest is unique: the edges are held in one strict total order -- the weight key of the double J = common / denom
(smaller key = more similar), then i, then j -- and Kruskal over a strict order leaves exactly one forest.  `denom` follows
include/rtclust.h and weight_denom of rtc_mst.hip:
    mode 0           |A| + |B| - common
    mode 1           min(|A|, |B|)
    mode 2 | s << 2  min(s, |A| + |B| - common)
J is the float64 quotient (0.0 where denom == 0) and key = 0x4000000000000000 - bits(J).  Where all sizes are below 2^26 two
different rationals never round to one double, so the order of the keys is the order of the exact rationals (forest_exact);
above that the double is the definition, the device forms the same correctly rounded quotient."""
from fractions import Fraction

import numpy as np

KEY_ONE = 0x4000000000000000


def _columns(edges):
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    return e[:, 0], e[:, 1], e[:, 2]


def denoms(edges, lens, wmode):
    i, j, c = _columns(edges)
    lens = np.asarray(lens).astype(np.int64)
    sa, sb = lens[i], lens[j]
    if (wmode & 3) == 1:
        return np.minimum(sa, sb)
    u = sa + sb - c
    if (wmode & 3) == 2:
        return np.minimum(u, np.int64((wmode & 0xffffffff) >> 2))
    return u


def keys(edges, lens, wmode):
    """the u64 weight key of every edge"""
    c = _columns(edges)[2]
    d = denoms(edges, lens, wmode)
    J = np.zeros(len(c), dtype=np.float64)
    nz = d != 0
    J[nz] = c[nz].astype(np.float64) / d[nz].astype(np.float64)
    return (np.uint64(KEY_ONE) - J.view(np.uint64)).astype(np.uint64)


def order(edges, lens, wmode):
    """the permutation that puts the list into (key, i, j) order"""
    i, j, _ = _columns(edges)
    return np.lexsort((j, i, keys(edges, lens, wmode)))


def _kruskal(n, i, j, perm):
    """positions (into the list) of the forest's edges, over the list taken in the order `perm`"""
    parent = list(range(n))
    chosen = []
    left = n - 1
    for p, a, b in zip(perm.tolist(), i[perm].tolist(), j[perm].tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[a] = b
            chosen.append(p)
            left -= 1
            if not left:
                break
    return chosen


def forest(n, edges, lens, wmode):
    """the (i, j, common) records of the forest in (key, i, j) order, int64 [f, 3]"""
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    if n < 2 or not len(e):
        return np.zeros((0, 3), dtype=np.int64)
    chosen = _kruskal(n, e[:, 0], e[:, 1], order(e, lens, wmode))
    return e[np.array(chosen, dtype=np.int64)].reshape(-1, 3)


def sorted_list(edges, lens, wmode):
    """the whole list in (key, i, j) order: the forest of a list that is a forest already"""
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    return e[order(e, lens, wmode)]


def rounds(n, edges, lens, wmode):
    """Boruvka rounds under the same order, as h_rounds counts them: the productive rounds and the one that finds nothing
    (1 for an empty list; rtc_msf_dev reports 0 without running when n < 2)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    if n < 2:
        return 0
    if not len(e):
        return 1
    e = e[order(e, lens, wmode)]  # position = rank
    i, j = e[:, 0], e[:, 1]
    comp = np.arange(n, dtype=np.int64)
    productive = 0
    while True:
        ci, cj = comp[i], comp[j]
        cross = ci != cj
        if not cross.any():
            return productive + 1
        i, j, ci, cj = i[cross], j[cross], ci[cross], cj[cross]
        m = len(i)
        best = np.full(n, m, dtype=np.int64)  # every component's first outgoing edge by rank
        u, first = np.unique(ci, return_index=True)
        best[u] = first
        u, first = np.unique(cj, return_index=True)
        best[u] = np.minimum(best[u], first)
        chosen = np.unique(best[best < m])
        g = coo_matrix((np.ones(len(chosen), dtype=np.int8), (ci[chosen], cj[chosen])), shape=(n, n))
        comp = connected_components(g, directed=False)[1].astype(np.int64)[comp]
        productive += 1


def forest_exact(n, edges, lens, wmode):
    """forest() with the weights as exact rationals (small inputs)"""
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    if n < 2 or not len(e):
        return np.zeros((0, 3), dtype=np.int64)
    d = denoms(e, lens, wmode).tolist()
    w = [Fraction(int(c), int(q)) if q else Fraction(0) for c, q in zip(e[:, 2].tolist(), d)]
    perm = np.array(sorted(range(len(e)), key=lambda p: (-w[p], int(e[p, 0]), int(e[p, 1]))), dtype=np.int64)
    chosen = _kruskal(n, e[:, 0], e[:, 1], perm)
    return e[np.array(chosen, dtype=np.int64)].reshape(-1, 3)
