"""Line-by-line restatement of the reference's k-NN DBSCAN (src/dbscan.cpp of the RabbitTClust tree), the yardstick of
clust-dbscan --fast --knn K: buildKNNForPoint (:221-360) with its min-heap of (float score, id), the k-NN branch of
findNeighborsKSSDWithIndex (:444-454) and, through tests/refdbscan.py, the sequential walk of KssdDBSCAN (:807-948).  numpy's
float32 division is the correctly rounded binary32 division of the C code; heapq on (score, id) tuples is std::priority_queue
with std::greater on std::pair<float, int>.  Also the two closed forms the GPU computes, for the CPU check
that they agree with the heap and with the walk."""
import heapq
import math

import numpy as np

from tests import refdbscan as R


def effective_k(knn_k, min_pts):
    """KssdDBSCAN's adjustment (:754-757)"""
    return min_pts - 1 if 0 < knn_k < min_pts - 1 else knn_k


def passers_in_arrival_order(sketches, eps, kmer_size, max_posting=0):
    """Per point the candidates that pass the predicate of :333-338, in the order of the `touched` list, as (id, np.float32
    score) -- everything of buildKNNForPoint before the heap."""
    t = R.jaccard_min(eps, kmer_size)
    n = len(sketches)
    sizes = [len(s) for s in sketches]
    kept = R.kept_hashes(sketches, max_posting)
    pruned = [[h for h in s.tolist() if h in kept] for s in sketches]  # the point's hashes in list order (:268-272)
    post = {}
    for g, s in enumerate(pruned):
        for h in s:
            post.setdefault(h, []).append(g)  # ascending genome index
    out = [[] for _ in range(n)]
    for p in range(n):
        size_ref = sizes[p]
        if size_ref == 0:
            continue  # :246-248
        size_ref16 = 65535 if size_ref > 65535 else size_ref  # :260
        min_size = int(math.floor(t * size_ref)) if t > 0.0 else 0
        max_size = int(math.ceil(float(size_ref) / t)) if t > 0.0 else 2 ** 31 - 1
        cnt = {}
        touched = []
        for h in pruned[p]:  # the posting scan (:271-300)
            for c in post[h]:
                if c == p:
                    continue
                size_qry = sizes[c]
                if size_qry < min_size or size_qry > max_size:
                    continue
                if c not in cnt:
                    cnt[c] = 1
                    touched.append(c)
                elif cnt[c] < size_ref16:
                    cnt[c] += 1
        one_plus_t = 1.0 + t
        t_times_size_ref = t * float(size_ref)
        for c in touched:  # the evaluation (:323-343)
            size_qry = sizes[c]
            if size_qry == 0:
                continue
            common = cnt[c]
            if size_qry < min_size or size_qry > max_size:
                continue
            lhs = float(common) * one_plus_t
            rhs = t_times_size_ref + t * float(size_qry)
            if lhs + 1e-12 < rhs:
                continue
            union_size = size_ref + size_qry - common
            score = np.float32(0.0) if union_size == 0 else np.float32(common) / np.float32(union_size)
            out[p].append((c, score))
    return out


def heap_select(arrivals, k):
    """The min-heap of :344-349 over (id, score) in arrival order: the (id, score) it holds at the end, in the order the
    reference pops them (:354-357)."""
    heap = []
    for c, score in arrivals:
        if len(heap) < k:
            heapq.heappush(heap, (score, c))
        elif score > heap[0][0]:
            heapq.heappop(heap)
            heapq.heappush(heap, (score, c))
    out = []
    while heap:
        score, c = heapq.heappop(heap)
        out.append((c, score))
    return out


def closed_select(arrivals, k):
    """The selection's closed form: the set of ids the heap ends with, and whether the row needed its arrival order."""
    if len(arrivals) <= k:
        return {c for c, _ in arrivals}, False
    s_star = sorted((s for _, s in arrivals), reverse=True)[k - 1]
    above = {c for c, s in arrivals if s > s_star}
    at_or_above = [(c, s) for c, s in arrivals if s >= s_star]
    if len(at_or_above) == k:
        return {c for c, _ in at_or_above}, False
    first_k, later = at_or_above[:k], at_or_above[k:]  # T: the arrival of first_k[-1]
    tied = sorted(c for c, s in first_k if s == s_star)
    h = sum(1 for _, s in later if s > s_star)
    return above | set(tied[h:]), True


def knn_lists(sketches, eps, kmer_size, knn_k, max_posting=0):
    """Every point's neighbour list as the k-NN branch returns it (:444-454): the heap's members, in the order they were popped,
    with (double)score >= jaccard_min."""
    t = R.jaccard_min(eps, kmer_size)
    out = []
    for arrivals in passers_in_arrival_order(sketches, eps, kmer_size, max_posting):
        out.append([c for c, score in heap_select(arrivals, knn_k) if float(score) >= t])
    return out


def closed_walk(nbrs, min_pts):
    """The walk's closed form over directed lists: m(v) = the smallest core index with a path to v whose vertices other than v
    are core; labels by the rank of m(v), -1 where there is none.  Returns (labels, core flags)."""
    n = len(nbrs)
    core = [len(nbrs[v]) + 1 >= min_pts for v in range(n)]
    m = [None] * n
    for u in range(n):  # ascending: the first core point to reach v is the smallest
        if not core[u] or m[u] is not None:
            continue
        m[u] = u
        stack = [u]
        while stack:
            p = stack.pop()
            for q in nbrs[p]:
                if m[q] is None:
                    m[q] = u
                    if core[q]:
                        stack.append(q)
    rank = {r: i for i, r in enumerate(sorted({x for x in m if x is not None}))}
    return [-1 if x is None else rank[x] for x in m], core


def labels_of_knn(sketches, eps, min_pts, kmer_size, knn_k, max_posting=0, return_core=False):
    """KssdDBSCAN's labels with knn_k > 0 on u32 sketches, noise as -1 (what rtc_dbscan_knn returns)."""
    nbrs = knn_lists(sketches, eps, kmer_size, effective_k(knn_k, min_pts), max_posting)
    lab, _ = R.sequential_walk(nbrs, min_pts)
    labels = np.array([x if x >= 0 else -1 for x in lab], dtype=np.int32)
    if return_core:
        return labels, np.array([len(x) + 1 >= min_pts for x in nbrs], dtype=bool)
    return labels
