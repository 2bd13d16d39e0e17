"""The k-distance curve of clust-dbscan --kdist (rtc_dbscan_sweep's h_kdist) restated in exact integer arithmetic, beside
tests/refdbscan.py whose predicate it is tied to in tests/test_cpu_dbscan_sweep.py.

For a point p and k = minPts - 1: among the points that share at least one kept hash with p, ranked by
j = common / (|p| + |q| - common) as exact fractions (larger first, equal j: the lower index first), the k-th.  common is the
count the reference's predicate sees: over the hashes --max-posting keeps and saturated at 65535 for u32 sketches, exact for
u64 sketches; the sizes are the unpruned ones.  Two empty u64 sketches see each other at j = 1 (the brute force accepts them
at every eps); an empty u32 sketch has no candidates."""
import math
from fractions import Fraction

from tests import refdbscan as R

NONE = 0xFFFFFFFF


def candidates(sketches, use64, max_posting=0):
    """Per point: {q: common} over the points sharing a kept hash (the empty-sketch clique of the u64 path included, common 0)."""
    n = len(sketches)
    kept = None if use64 else R.kept_hashes(sketches, max_posting)
    post = {}
    for g, s in enumerate(sketches):
        for h in s.tolist():
            if kept is None or h in kept:
                post.setdefault(h, []).append(g)
    out = [{} for _ in range(n)]
    for lst in post.values():
        for a in lst:
            for b in lst:
                if a != b:
                    out[a][b] = out[a].get(b, 0) + 1
    if not use64:
        for d in out:
            for q in d:
                d[q] = min(d[q], 65535)
    else:
        empty = [g for g, s in enumerate(sketches) if len(s) == 0]
        for a in empty:
            for b in empty:
                if a != b:
                    out[a][b] = 0
    return out


def jaccard(common, size_p, size_q):
    denom = size_p + size_q - common
    return Fraction(1) if denom == 0 else Fraction(common, denom)


def kdist(sketches, min_pts, use64, max_posting=0):
    """Per point (common, size_p, size_q, neighbour); neighbour NONE (and common = size_q = 0) with fewer than k candidates;
    k <= 0: (|p|, |p|, |p|, p)."""
    k = min_pts - 1
    sizes = [len(s) for s in sketches]
    if k <= 0:
        return [(a, a, a, p) for p, a in enumerate(sizes)]
    out = []
    for p, cand in enumerate(candidates(sketches, use64, max_posting)):
        ranked = sorted(cand.items(), key=lambda qc: (-jaccard(qc[1], sizes[p], sizes[qc[0]]), qc[0]))
        if len(ranked) < k:
            out.append((0, sizes[p], 0, NONE))
        else:
            q, c = ranked[k - 1]
            out.append((c, sizes[p], sizes[q], q))
    return out


def distance(common, size_p, size_q, kmer_size):
    """-ln(2 j / (1 + j)) / kmer_size in double, as the host forms it; 0 at j = 1."""
    denom = size_p + size_q - common
    if denom == common:
        return 0.0
    j = float(common) / float(denom)
    return -math.log(2.0 * j / (1.0 + j)) / kmer_size
