"""Pure-Python brute forces shared by the tests (no native code): the MST's exact size-ratio filter and Kruskal over
np.intersect1d counts, generateForest's cut, union-find partitions, and a runner for in-process ranks on host threads."""
import math
import threading

import numpy as np

INT32_MAX = 2 ** 31 - 1


def radio(threshold, kmer_size):
    """the filter's bound: floor of the reference's calr(threshold, k - 1), saturated at INT32_MAX"""
    r = 2.0 * math.exp(threshold * (kmer_size - 1)) - 1.0
    return int(r) if r < INT32_MAX else INT32_MAX


def mst_forest(sets, k, containment, thr):
    """(candidates, forest) as (dist, i, j) lists: a pair is a candidate iff it shares a hash and max <= R * min in Python
    integers; Kruskal over the candidates sorted by distance (api.mst_distance, the reference's expression order)"""
    from rabbittclust_amd import api
    R = radio(thr, k)
    cand = []
    for i in range(len(sets)):
        for j in range(i):
            c = len(np.intersect1d(sets[i], sets[j], assume_unique=True))
            a, b = len(sets[i]), len(sets[j])
            if c and max(a, b) <= R * min(a, b):
                cand.append((api.mst_distance(c, a, b, k, containment), i, j))
    cand.sort()
    parent = list(range(len(sets)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    forest = []
    for d, i, j in cand:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[ri] = rj
            forest.append((d, i, j))
    return cand, forest


def generate_forest(records, thr):
    """generateForest (src/MST.cpp:77-85): the tree's records with dist <= threshold, in order"""
    return [r for r in records if r[0] <= thr]


def partition(pairs, n):
    """the groups of n vertices joined by (dist, i, j) pairs, as a sorted list of sorted tuples"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for _, i, j in pairs:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[ri] = rj
    groups = {}
    for v in range(n):
        groups.setdefault(find(v), []).append(v)
    return sorted(tuple(g) for g in groups.values())


def run_ranks(fns, timeout=300):
    """run fns[r]() on one host thread each (in-process ranks); returns their results, re-raises the first error"""
    err, out = [], [None] * len(fns)

    def run(i):
        try:
            out[i] = fns[i]()
        except BaseException as e:  # noqa: BLE001 -- reported to the main thread
            err.append(e)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    if err:
        raise err[0]
    return out
