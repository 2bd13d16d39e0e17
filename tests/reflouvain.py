"""rtc_louvain's definition (include/rtclust.h) restated with Python integers: the deterministic, synchronous Louvain the
library runs on the GPU.  Nothing here is taken from igraph; the header is the definition and this file repeats it.

louvain(n, edges, resolution) -> (labels, n_clusters, levels, rounds, modularity), edges an iterable of (u, v, q), q >= 1 the
weight in units of 2^-20."""

import math

MAX_ROUNDS = 64
MAX_LEVELS = 32


def _llround(x):
    """C's llround for x >= 0: to the nearest integer, halves away from zero (x - floor(x) is exact in doubles)"""
    r = math.floor(x)
    return r + 1 if x - r >= 0.5 else r


def quantise(weight):
    """q of a double weight as the callers form it: max(1, llround(weight * 2^20))"""
    return max(1, _llround(weight * 1048576.0))


def resolution_units(resolution):
    return _llround(resolution * 65536.0)


def _adjacency(n, entries):
    adj = [dict() for _ in range(n)]
    for a, b, w in entries:
        adj[a][b] = adj[a].get(b, 0) + w
    return adj


def _level(adj, M2, g):
    """one level from singletons: (community of every vertex, rounds run, moves made)"""
    n = len(adj)
    k = [sum(row.values()) for row in adj]
    comm = list(range(n))
    tot = list(k)
    rounds = moves = idle = 0
    while rounds < MAX_ROUNDS and idle < 2:
        odd = rounds & 1
        new = list(comm)
        moved = 0
        for x in range(n):
            c = comm[x]
            e = {}
            for y, w in adj[x].items():
                if y != x:
                    e[comm[y]] = e.get(comm[y], 0) + w
            s_c = e.get(c, 0) * M2 * 65536 - g * k[x] * (tot[c] - k[x])
            best_s, best_d = s_c, c
            for d in sorted(e):
                if d == c or (d > c) != bool(odd):
                    continue
                s = e[d] * M2 * 65536 - g * k[x] * tot[d]
                if s > best_s:  # ascending d: an equal score keeps the smaller community
                    best_s, best_d = s, d
            if best_d != c:
                new[x] = best_d
                moved += 1
        comm = new
        tot = [0] * n
        for x in range(n):
            tot[comm[x]] += k[x]
        rounds += 1
        moves += moved
        idle = 0 if moved else idle + 1
    return comm, rounds, moves


def louvain(n, edges, resolution=1.0):
    g = resolution_units(resolution)
    assert 0 < g < (1 << 32)
    entries = []
    for u, v, q in edges:
        assert 0 <= u < n and 0 <= v < n and q >= 1
        entries += [(u, v, q), (v, u, q)]  # u == v: both land on the self entry, 2q
    label = list(range(n))
    if not entries:
        return label, n, 0, 0, 0.0
    adj = _adjacency(n, entries)
    M2 = sum(sum(row.values()) for row in adj)
    levels = rounds = 0
    while levels < MAX_LEVELS:
        comm, r, moved = _level(adj, M2, g)
        levels += 1
        rounds += r
        if not moved:
            break
        # communities numbered by their smallest member
        smallest = {}
        for x, c in enumerate(comm):
            smallest.setdefault(c, x)
        order = {c: i for i, c in enumerate(sorted(smallest, key=smallest.get))}
        newc = [order[c] for c in comm]
        label = [newc[v] for v in label]
        adj = _adjacency(len(order), [(newc[x], newc[y], w) for x, row in enumerate(adj) for y, w in row.items()])
    ncl = len(adj)
    inner = [adj[c].get(c, 0) for c in range(ncl)]
    tot = [sum(adj[c].values()) for c in range(ncl)]
    num = sum(inner[c] * M2 * 65536 - g * tot[c] * tot[c] for c in range(ncl))
    return label, ncl, levels, rounds, num / (M2 * M2 * 65536)


def clusters_of(labels):
    """members of every cluster, clusters in label order"""
    out = {}
    for x, c in enumerate(labels):
        out.setdefault(c, []).append(x)
    return [out[c] for c in sorted(out)]
