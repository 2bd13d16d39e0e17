"""Restatement of the reference's MinHash DBSCAN (src/dbscan.cpp of the RabbitTClust tree), the yardstick of clust-dbscan
--minhash: the neighbour test findNeighborsMinHash (:685-720, dist <= eps), the sequential walk MinHashDBSCAN (:987-1096) and
printDBSCANResult (:1102-1210, the layout of printKssdDBSCANResult: tests/refdbscan.print_result).  MinHash::distance() is
Mash's union-truncated estimator as the project restates it (rtc_mash_merge.h, host_mst_distance mode 2): RabbitSketch is
absent from the reference tree, so the distance is parity-unpinned like rtc_mst_mash's.  Python floats are IEEE doubles and
math.log is the C library's log.  Also the closed form the GPU computes and the decision table of rtc_dbscan_mash."""
import math

import numpy as np

from tests.refdbscan import print_result  # noqa: F401  (the two printers coincide)


def mash_counts(a, b, sketch_size):
    """rtc_mash_merge: merge the ascending lists, stop after sketch_size union elements: (common, denom)."""
    i = j = c = d = 0
    na, nb = len(a), len(b)
    while d < sketch_size and i < na and j < nb:
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            c += 1
            i += 1
            j += 1
        d += 1
    if d < sketch_size:
        d += min((na - i) + (nb - j), sketch_size - d)
    return c, d


def distance(common, denom, kmer_size):
    """host_mst_distance, mode 2"""
    j = common / denom if denom else 0.0
    if j == 0.0:
        return 1.0
    if j == 1.0:
        return 0.0
    dist = -math.log(2.0 * j / (1.0 + j)) / kmer_size
    return 1.0 if dist > 1.0 else dist


def mash_counts_sets(a, b, sketch_size):
    """the same counts from the definition: the sketch_size smallest elements of the union, and the shared ones among them"""
    u = np.union1d(a, b)[:sketch_size]
    if len(u) == 0:
        return 0, 0
    both = np.intersect1d(a, b, assume_unique=True)
    return int(np.count_nonzero(both <= u[-1])), len(u)


def count_matrix(sketches, sketch_size):
    """(common, denom) of every pair, brute force"""
    arrs = [np.asarray(s) for s in sketches]
    n = len(arrs)
    common = np.zeros((n, n), dtype=np.int64)
    denom = np.zeros((n, n), dtype=np.int64)
    for p in range(n):
        for q in range(p, n):
            common[p, q], denom[p, q] = common[q, p], denom[q, p] = mash_counts_sets(arrs[p], arrs[q], sketch_size)
    return common, denom


def distance_matrix(counts, kmer_size):
    common, denom = counts
    n = len(common)
    memo = {}
    out = np.ones((n, n))
    for p in range(n):
        for q in range(n):
            key = (int(common[p, q]), int(denom[p, q]))
            if key not in memo:
                memo[key] = distance(key[0], key[1], kmer_size)
            out[p, q] = memo[key]
    return out


def neighbour_lists(dist, eps):
    """findNeighborsMinHash for every point (:696-716), ascending"""
    return [[int(q) for q in np.flatnonzero(dist[p] <= eps) if q != p] for p in range(len(dist))]


def sequential_walk(nbrs, min_pts):
    """MinHashDBSCAN's loop (:1011-1065): labels (>= 0 cluster, -2 noise).  The reference compares the neighbour count, a
    size_t, with the int minPts: at minPts <= 0 every point is a core point here (a negative value is treated like 0)."""
    n = len(nbrs)
    min_pts = max(min_pts, 0)
    labels = [-1] * n
    cluster_id = 0
    for i in range(n):
        if labels[i] != -1:
            continue
        neighbours = nbrs[i]
        if len(neighbours) < min_pts:  # :1017
            labels[i] = -2
            continue
        labels[i] = cluster_id
        seed = list(neighbours)
        head = 0
        while head < len(seed):
            q = seed[head]
            head += 1
            if labels[q] == -2:  # :1035
                labels[q] = cluster_id
                continue
            if labels[q] != -1:
                continue
            labels[q] = cluster_id
            qn = nbrs[q]
            if len(qn) >= min_pts:  # :1050
                for nb in qn:
                    if labels[nb] == -1 or labels[nb] == -2:
                        seed.append(nb)
        cluster_id += 1
    return labels


def closed_form(nbrs, min_pts):
    """What rtc_dbscan_mash computes: components of the core points over core-core edges numbered by their smallest core index,
    a border point takes the lowest number among its core neighbours', -1 noise.  Returns (labels, core flags)."""
    n = len(nbrs)
    core = [len(nbrs[v]) >= max(min_pts, 0) for v in range(n)]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for v in range(n):
        if core[v]:
            for u in nbrs[v]:
                if core[u]:
                    a, b = find(u), find(v)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    cid, labels = {}, [-1] * n
    for v in range(n):
        if core[v]:
            r = find(v)
            if r not in cid:
                cid[r] = len(cid)
            labels[v] = cid[r]
    for v in range(n):
        if not core[v]:
            ls = [labels[u] for u in nbrs[v] if core[u]]
            if ls:
                labels[v] = min(ls)
    return labels, core


def labels_of(dist, eps, min_pts):
    """MinHashDBSCAN's labels with noise as -1, and the core flags"""
    nbrs = neighbour_lists(dist, eps)
    lab = sequential_walk(nbrs, min_pts)
    return (np.array([x if x >= 0 else -1 for x in lab], dtype=np.int32),
            np.array([len(x) >= max(min_pts, 0) for x in nbrs], dtype=bool))


def decision_table(sketch_size, kmer_size, eps):
    """cmin[d], d = 0 .. sketch_size: the least common with distance(common, d) <= eps by a linear scan, d + 1 where none"""
    out = []
    for d in range(sketch_size + 1):
        c = 0
        while c <= d and not distance(c, d, kmer_size) <= eps:
            c += 1
        out.append(c)
    return out
