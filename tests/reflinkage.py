"""clust-mst --linkage complete restated (include/rtclust.h holds the definition): the agglomeration on exact rationals in two
forms -- naive, all pairs each step, and row-best, the bookkeeping the kernels keep -- the host's distance and cut, the
conservative stop bound and the two files the command line writes.

Keys are compared as fractions.Fraction: every kappa a matrix holds is ranked once, exactly, and both forms then work on
(rank, denom) codes, whose integer order is the order of K(X, Y): kappa ascending, then denom ascending."""
import math
from fractions import Fraction

import numpy as np


def kappa(common, denom):
    return Fraction(int(common), int(denom)) if int(denom) else Fraction(0)


class _Codes:
    """the matrix as codes rank << 32 | denom (int64, symmetric; the diagonal is ignored)"""

    def __init__(self, keys):
        k = np.asarray(keys, dtype=np.uint64)
        assert k.ndim == 3 and k.shape[0] == k.shape[1] and k.shape[2] == 2
        self.m = m = int(k.shape[0])
        flat = k.reshape(-1, 2)
        uniq, inv = np.unique(flat, axis=0, return_inverse=True)
        # Ranking 10^5 Fractions by their own comparison takes seconds; floor(kappa 2^64) ranks them as exactly: two different
        # quotients of denominators below 2^32 lie more than 2^-64 apart, equal ones give the same integer.
        q = [((c << 64) // d if d else 0) for c, d in uniq.tolist()]
        by_q = {}
        for (c, d), v in zip(uniq.tolist(), q):
            by_q.setdefault(v, kappa(c, d))
        by_q.setdefault(0, Fraction(0))  # rank 0 is kappa = 0
        qs = sorted(by_q)
        self.order = [by_q[v] for v in qs]
        assert all(x < y for x, y in zip(self.order[:64], self.order[1:65]))
        rank_of = {v: i for i, v in enumerate(qs)}
        ur = np.array([rank_of[v] for v in q], dtype=np.int64)
        self.code = ((ur[inv.reshape(-1)] << 32) | flat[:, 1].astype(np.int64)).reshape(m, m)

    def key(self, code):
        """(common, denom) of a code with kappa > 0"""
        r, d = int(code) >> 32, int(code) & 0xFFFFFFFF
        c = self.order[r] * d
        assert c.denominator == 1
        return int(c), d

    def stops(self, rank, kmin):
        f = self.order[rank]
        return f == 0 or f < Fraction(int(kmin[0]), int(kmin[1]))


def naive(keys, kmin=(0, 1)):
    """the definition, all pairs each step: [(a, b, common, denom, size)] in step order"""
    K = _Codes(keys)
    m, C = K.m, K.code.copy()
    active = np.ones(m, dtype=bool)
    size = [1] * m
    upper = np.triu(np.ones((m, m), dtype=bool), 1)
    out = []
    for _ in range(max(m - 1, 0)):
        R = np.where(upper & active[:, None] & active[None, :], C >> 32, -1)
        a, b = divmod(int(np.argmax(R)), m)  # the first maximum in row-major order: the smallest a, then the smallest b
        if R[a, b] < 0 or K.stops(int(R[a, b]), kmin):
            break
        c, d = K.key(C[a, b])
        size[a] += size[b]
        out.append((a, b, c, d, size[a]))
        mn = np.minimum(C[a], C[b])
        C[a, :] = mn
        C[:, a] = mn
        active[b] = False
    return out


def rowbest(keys, kmin=(0, 1)):
    """the same merges from row-bests: every live row keeps its best partner (largest kappa, ties to the smallest index); after a
    step exactly the rows whose partner was a or b, and row a, look again.  Returns (merges, rescans)."""
    K = _Codes(keys)
    m, C = K.m, K.code.copy()
    active = np.ones(m, dtype=bool)
    size = [1] * m
    bp, bc = [None] * m, [0] * m

    def scan(x):
        r = np.where(active, C[x] >> 32, -1)
        r[x] = -1
        y = int(np.argmax(r)) if m else 0
        if m == 0 or r[y] <= 0:  # rank 0 is kappa 0: no partner
            bp[x], bc[x] = None, 0
        else:
            bp[x], bc[x] = y, int(C[x, y])

    for x in range(m):
        scan(x)
    out, rescans = [], 0
    for _ in range(max(m - 1, 0)):
        best = None
        for x in range(m):
            if active[x] and bp[x] is not None:
                cand = (-(bc[x] >> 32), min(x, bp[x]), max(x, bp[x]), bc[x])
                if best is None or cand[:3] < best[:3]:
                    best = cand
        if best is None or K.stops(-best[0], kmin):
            break
        a, b = best[1], best[2]
        c, d = K.key(best[3])
        size[a] += size[b]
        out.append((a, b, c, d, size[a]))
        mn = np.minimum(C[a], C[b])
        C[a, :] = mn
        C[:, a] = mn
        active[b] = False
        for x in range(m):
            if active[x] and (x == a or bp[x] == a or bp[x] == b):
                rescans += 1
                scan(x)
    return out, rescans


def distance(common, denom, kmer_size):
    """the distance of a key, as the MST's edges are weighed on the index path (same expression order)"""
    inv = 1.0 / kmer_size
    jaccard = 0.0 if denom == 0 else float(common) / float(denom)
    if jaccard == 1.0:
        return 0.0
    if jaccard == 0.0:
        return 1.0
    ratio = (2.0 * jaccard) / (1.0 + jaccard)
    return -inv * math.log(ratio)


def bound(threshold, kmer_size):
    """the stop bound the command line passes: J = 1 / (2 exp(k d) - 1), times (1 - 2^-20), as floor(J 2^31) / 2^31"""
    j = 1.0 / (2.0 * math.exp(kmer_size * threshold) - 1.0) * (1.0 - 2.0 ** -20)
    return (min(max(int(math.floor(j * 2147483648.0)), 0), 1 << 31), 1 << 31)


def cut(merges, threshold, kmer_size):
    """the merges the host keeps: in order, up to the first whose distance is > threshold"""
    kept = []
    for mg in merges:
        if distance(mg[2], mg[3], kmer_size) > threshold:
            break
        kept.append(mg)
    return kept


def clusters_of(members, kept):
    """the flat clusters of one component after its kept merges (a, b as genome indices), members ascending, by smallest member"""
    cl = {g: [g] for g in members}
    for a, b, *_ in kept:
        cl[a] = cl[a] + cl.pop(b)
    return sorted(sorted(c) for c in cl.values())


def keys_of(sketches):
    """the key matrix of a list of hash sets: common, |a| + |b| - common"""
    sets = [set(int(h) for h in s) for s in sketches]
    m = len(sets)
    k = np.zeros((m, m, 2), dtype=np.uint32)
    for i in range(m):
        for j in range(i):
            c = len(sets[i] & sets[j])
            k[i, j] = k[j, i] = (c, len(sets[i]) + len(sets[j]) - c)
    return k


def complete(sketches, comp, kmin=(0, 1)):
    """rtc_linkage_complete: (merges with genome indices, first) over the components of the labelling, in order of their
    smallest member"""
    groups = {}
    for g, lab in enumerate(comp):
        groups.setdefault(int(lab), []).append(g)
    merges, first = [], [0]
    for members in sorted(groups.values()):
        if len(members) >= 2:
            mg, _ = rowbest(keys_of([sketches[g] for g in members]), kmin)
            merges += [(members[a], members[b], c, d, s) for a, b, c, d, s in mg]
        first.append(len(merges))
    return merges, first


def refine(sketches, clusters, threshold, kmer_size):
    """clust-mst --linkage complete: (result clusters, linkage lines) from the plain run's clusters"""
    comp = [0] * len(sketches)
    for i, c in enumerate(clusters):
        for g in c:
            comp[g] = i
    merges, first = complete(sketches, comp, bound(threshold, kmer_size))
    groups = sorted(sorted(c) for c in clusters)
    out, lines = [], []
    n = len(sketches)
    cid = list(range(n))
    next_id = n
    for ci, members in enumerate(groups):
        kept = cut(merges[first[ci]:first[ci + 1]], threshold, kmer_size)
        out += clusters_of(members, kept)
        for a, b, c, d, s in kept:
            lines.append("%d\t%d\t%.6f\t%d\n" % (cid[a], cid[b], distance(c, d, kmer_size), s))
            cid[a] = next_id
            next_id += 1
    return sorted(out), "".join(lines)


def cluster_text(clusters, meta, by_file, threshold):
    """print_result with a threshold; meta[g] = (file, length, name, comment) by file, (name, length, comment) by sequence"""
    out = ["# Clustering threshold: %.6f\n# Total clusters: %d\n#\n" % (threshold, len(clusters))]
    for i, c in enumerate(clusters):
        out.append("the cluster %d is: \n" % i)
        for j, g in enumerate(c):
            if by_file:
                f, ln, name, comment = meta[g]
                out.append("\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n" % (j, g, ln, f, name, comment))
            else:
                name, ln, comment = meta[g]
                out.append("\t%6d\t%6d\t%12dnt\t%20s\t%s\n" % (j, g, ln, name, comment))
        out.append("\n")
    return "".join(out)
