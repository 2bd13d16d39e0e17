"""Sequential restatement of clust-greedy --order degree (rtc_greedy_degree; include/rtclust.h has the definition): the
neighbour relation from tests/refdbscan.py (KSSD, the reference's predicate at eps = threshold) or tests/refdbscan_mash.py
(MinHash, distance <= threshold on the union-truncated counts) with the empty sketches isolated, the walk in the order
(degree descending, index ascending) and the assignment of the members, all in Python integers.  Also the two files the
command line writes, as text."""
import math

import numpy as np

from tests import refdbscan as R
from tests import refdbscan_mash as M


def _symmetric(nbrs):
    sets = [set(x) for x in nbrs]
    for p, x in enumerate(nbrs):
        for q in x:
            if p not in sets[q]:
                raise ValueError("the threshold test of the pair (%d, %d) depends on the orientation" % (min(p, q), max(p, q)))
    return [sorted(s) for s in sets]


def neighbours_kssd(sketches, threshold, kmer_size, use64):
    """N for KSSD sketches: refdbscan's lists, the empty sketches (neighbours of each other in its u64 brute force) isolated"""
    nbrs = R.neighbour_lists(sketches, threshold, kmer_size, use64)
    empty = {g for g, s in enumerate(sketches) if len(s) == 0}
    return _symmetric([[] if p in empty else [q for q in x if q not in empty] for p, x in enumerate(nbrs)])


def common_matrix(sketches):
    """|a & b| of every pair of a small set"""
    n = len(sketches)
    out = np.zeros((n, n), dtype=np.int64)
    for p in range(n):
        for q in range(p + 1, n):
            out[p, q] = out[q, p] = len(np.intersect1d(sketches[p], sketches[q], assume_unique=True))
    return out


def neighbours_kssd_dense(common, sizes, threshold, kmer_size):
    """The same relation from a matrix of the counts the predicate sees: refdbscan's test in both orientations as array
    arithmetic (IEEE doubles, no fused multiply-add), for sets too large for its posting walk.  Pairs without a common hash
    and empty sketches are no neighbours."""
    t = R.jaccard_min(threshold, kmer_size)
    a = np.asarray(sizes, dtype=np.float64)
    c = np.asarray(common, dtype=np.float64)

    def oriented(x, y):  # reference point x, candidate y
        ok = (y >= np.floor(t * x)) & (y <= np.ceil(x / t))
        return ok & ~(c * (1.0 + t) + 1e-12 < t * x + t * y)
    fwd, bwd = oriented(a[:, None], a[None, :]), oriented(a[None, :], a[:, None])
    live = (c > 0) & (a[:, None] > 0) & (a[None, :] > 0)
    np.fill_diagonal(live, False)
    if ((fwd != bwd) & live).any():
        p, q = np.argwhere((fwd != bwd) & live)[0]
        raise ValueError("the threshold test of the pair (%d, %d) depends on the orientation" % (min(p, q), max(p, q)))
    keep = fwd & bwd & live
    return [np.flatnonzero(keep[p]).astype(np.int32) for p in range(len(a))]


def walk(nbrs, counts):
    """The definition over neighbour lists: counts(v, r) -> (common, denom) of a pair.  Returns (rep, degree, common, denom,
    n_clusters), lists of Python integers."""
    n = len(nbrs)
    deg = [len(x) for x in nbrs]
    order = sorted(range(n), key=lambda v: (-deg[v], v))
    is_rep = [False] * n
    for v in order:
        is_rep[v] = not any(is_rep[int(u)] for u in nbrs[v])
    cand = [[] for _ in range(n)]  # the representatives next to v, in the order: of equal j the first one stays
    for r in order:
        if is_rep[r]:
            for v in nbrs[r]:
                cand[int(v)].append(r)
    rep, common, denom = list(range(n)), [0] * n, [0] * n
    for v in range(n):
        if is_rep[v]:
            continue
        best = None
        for r in cand[v]:
            c, d = counts(v, r)
            c, d = int(c), int(d)
            if best is None or c * best[2] > best[1] * d:
                best = (r, c, d)
        rep[v], common[v], denom[v] = best
    return rep, deg, common, denom, sum(is_rep)


def kssd_counts(sketches, use64):
    """counts(v, r) for KSSD sketches: the count the predicate sees (u32 sketches: saturated at 65 535) and |v| + |r| - it"""
    memo = {}

    def counts(v, r):
        key = (min(v, r), max(v, r))
        if key not in memo:
            c = len(np.intersect1d(sketches[v], sketches[r], assume_unique=True))
            c = c if use64 else min(c, 65535)
            memo[key] = (c, len(sketches[v]) + len(sketches[r]) - c)
        return memo[key]
    return counts


def kssd(sketches, threshold, kmer_size, use64, nbrs=None):
    t = R.jaccard_min(threshold, kmer_size)
    if not t > 1e-12:
        raise ValueError("jaccard_min %g <= 1e-12" % t)
    if nbrs is None:
        nbrs = neighbours_kssd(sketches, threshold, kmer_size, use64)
    return walk(nbrs, kssd_counts(sketches, use64))


def minhash(sketches, sketch_size, threshold, kmer_size, counts=None):
    """counts: M.count_matrix(sketches, sketch_size) when the caller has it already"""
    if not threshold >= 0.0:
        raise ValueError("threshold %r" % threshold)
    common, denom = counts if counts is not None else M.count_matrix(sketches, sketch_size)
    nbrs = M.neighbour_lists(M.distance_matrix((common, denom), kmer_size), threshold)
    return walk(nbrs, lambda v, r: (common[v, r], denom[v, r]))


def as_arrays(result):
    rep, deg, common, denom, ncl = result
    return tuple(np.asarray(x, dtype=np.uint32) for x in (rep, deg, common, denom)) + (int(ncl),)


# ---- the command line's two files ----
def clusters(rep):
    """clusters_from_rep_of: by the representative's index, the representative first, the members in ascending order"""
    cid, out = {}, []
    for v, r in enumerate(rep):
        if r == v:
            cid[v] = len(out)
            out.append([v])
    for v, r in enumerate(rep):
        if r != v:
            out[cid[r]].append(v)
    return out


def print_result(cl, genomes):
    """print_result without a threshold header, the -l layout: genomes[v] = (file, length, name, comment)"""
    out = []
    for i, c in enumerate(cl):
        out.append("the cluster %d is: \n" % i)
        for j, cur in enumerate(c):
            g = genomes[cur]
            out.append("\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n" % (j, cur, g[1], g[0], g[2], g[3]))
        out.append("\n")
    return "".join(out)


def kssd_distance(common, denom, kmer_size):
    if denom == common:
        return 0.0
    j = float(common) / float(denom)
    return -math.log(2.0 * j / (1.0 + j)) / kmer_size


def order_tsv(result, names, kmer_size, is_minhash):
    rep, deg, common, denom, _ = result
    out = ["name\tdegree\trole\trepresentative\tdistance\n"]
    for v in sorted(range(len(rep)), key=lambda v: (-deg[v], v)):
        if rep[v] == v:
            dist = 0.0
        elif is_minhash:
            dist = M.distance(common[v], denom[v], kmer_size)
        else:
            dist = kssd_distance(common[v], denom[v], kmer_size)
        out.append("%s\t%d\t%s\t%s\t%.6f\n" % (names[v], deg[v], "rep" if rep[v] == v else "member", names[rep[v]], dist))
    return "".join(out)
