"""Average linkage (UPGMA) restated (include/rtclust.h holds the definition) in Python integers, twice: the naive scan of every
active pair at every step, and a variant that keeps every row's best partner and looks again only where it must.  Then the
host's side: the height of a merge, the integer cut, and the three writers of clust-mst --upgma."""
import math
from fractions import Fraction

import numpy as np

from tests import reflinkage as RL

Q1 = 1 << 20
W_MAX = 1 << 22


def _start(S, w):
    m = len(S)
    S = [[int(S[i][j]) for j in range(m)] for i in range(m)]
    n = [1] * m if w is None else [int(x) for x in w]
    assert len(n) == m and all(x >= 1 for x in n) and sum(n) < W_MAX
    return m, S, n


def _less(s1, p1, s2, p2):
    """mean s1 / p1 below mean s2 / p2, exactly"""
    return s1 * p2 < s2 * p1


def naive(S, w=None):
    """[(a, b, size_a, size_b, sum)] in step order: every step looks at all active pairs and takes the first of the least mean in
    ascending (a, b).  The means are ordered through floor(S 2^90 / (n_a n_b)) in Python integers (numpy object arrays, so the
    m^3 / 3 evaluations stay affordable): n_a n_b < 2^44, so two different means differ by more than 2^-88 and their keys by
    more than 4, and equal means have equal keys -- the key orders exactly as the cross products do."""
    m, S, n = _start(S, w)
    S = np.array(S, dtype=object).reshape(m, m)
    n = np.array(n, dtype=object)
    act = np.arange(m)
    out = []
    scale, never = 1 << 90, 1 << 200
    while len(act) > 1:
        r = len(act)
        na = n[act]
        key = (S[np.ix_(act, act)] * scale) // (na[:, None] * na[None, :])
        key[np.tril_indices(r)] = never
        p, q = divmod(int(np.argmin(key)), r)  # the first of equal keys in row-major order: smallest a, then smallest b
        a, b = int(act[p]), int(act[q])
        out.append((a, b, int(n[a]), int(n[b]), int(S[a, b])))
        ks = np.delete(act, [p, q])
        S[a, ks] = S[a, ks] + S[b, ks]
        S[ks, a] = S[a, ks]
        n[a] += n[b]
        act = np.delete(act, q)
    return out


def rowcache(S, w=None):
    """the same records from a per-row cache: best[x] is the partner y > x of row x with the least mean, the smallest y among
    equals.  After a merge row a looks again, so does every row whose partner was a or b, and every other row x < a compares the
    new D(x, a) with what it holds: a lower mean wins, and so does an EQUAL mean when a is below the cached partner.  Returns
    (records, rescans)."""
    m, S, n = _start(S, w)
    alive = [True] * m

    def scan(x):
        bx = None
        for y in range(x + 1, m):
            if alive[y] and (bx is None or _less(S[x][y], n[x] * n[y], S[x][bx], n[x] * n[bx])):
                bx = y
        return bx

    best = [scan(x) for x in range(m)]
    out, rescans = [], 0
    for _ in range(m - 1):
        a = None
        for x in range(m):
            if alive[x] and best[x] is not None:
                y = best[x]
                if a is None or _less(S[x][y], n[x] * n[y], S[a][best[a]], n[a] * n[best[a]]):
                    a = x
        b = best[a]
        out.append((a, b, n[a], n[b], S[a][b]))
        for c in range(m):
            if alive[c] and c != a and c != b:
                S[a][c] = S[c][a] = S[a][c] + S[b][c]
        n[a] += n[b]
        alive[b] = False
        best[b] = None
        for x in range(m):
            if not alive[x]:
                continue
            if x == a or best[x] == a or best[x] == b:
                best[x] = scan(x)
                rescans += 1
            elif x < a and best[x] is not None:
                y = best[x]
                l, r = S[x][a] * (n[x] * n[y]), S[x][y] * (n[x] * n[a])
                if l < r or (l == r and a < y):
                    best[x] = a
    return out, rescans


def distance(s, size_a, size_b):
    """rtc_upgma_distance: one double operation a step"""
    pairs = float(size_a) * float(size_b)
    scale = pairs * 1048576.0
    return float(s) / scale


def llround(x):
    lo = math.floor(abs(x))
    return (int(lo) + (1 if abs(x) - lo >= 0.5 else 0)) * (1 if x >= 0 else -1)


def keep(s, size_a, size_b, threshold):
    """the integer cut rule"""
    return int(s) <= llround(threshold * 1048576.0) * int(size_a) * int(size_b)


def cut(merges, threshold):
    """the merges that apply: in order, up to the first that the rule does not keep"""
    kept = []
    for mg in merges:
        if not keep(mg[4], mg[2], mg[3], threshold):
            break
        kept.append(mg)
    return kept


def means(merges):
    return [Fraction(s, na * nb) for _, _, na, nb, s in merges]


def quantise(common, denom, kmer_size):
    """the q of a key: rtc_cluster_quality's formula"""
    if common == 0 or denom == 0:
        return Q1
    return min(Q1, max(0, llround(RL.distance(int(common), int(denom), kmer_size) * 1048576.0)))


def sums_of(sketches, kmer_size):
    keys = RL.keys_of(sketches)
    m = len(sketches)
    return [[0 if i == j else quantise(int(keys[i, j, 0]), int(keys[i, j, 1]), kmer_size) for j in range(m)] for i in range(m)]


def clusters(sketches, comp, kmer_size):
    """rtc_upgma_clusters: (merges with genome indices, first) over the components of the labelling, in order of their smallest
    member"""
    groups = {}
    for g, lab in enumerate(comp):
        groups.setdefault(int(lab), []).append(g)
    merges, first = [], [0]
    for members in sorted(groups.values()):
        if len(members) >= 2:
            merges += [(members[a], members[b], na, nb, s) for a, b, na, nb, s in naive(sums_of([sketches[g] for g in members], kmer_size))]
        first.append(len(merges))
    return merges, first


def newick(label, members, merges):
    """one ultrametric tree: node height = distance / 2, branch = parent height - child height, %.6f; one member: 'label;'"""
    members = sorted(members)
    if len(members) == 1 or not merges:
        return label(members[0]) + ";"
    text = {g: label(g) for g in members}
    height = {g: 0.0 for g in members}
    for a, b, na, nb, s in merges:
        h = distance(s, na, nb) / 2.0
        text[a] = "(%s:%.6f,%s:%.6f)" % (text[a], h - height[a], text.pop(b), h - height[b])
        height[a] = h
    (only,) = text.values()
    return only + ";"


def report(run_clusters, merges, first, threshold, n, label):
    """clust-mst --upgma from the run's clusters (in <output>'s order) and rtc_upgma_clusters' records for that labelling:
    (refined clusters, the text of .upgma.linkage.txt, the text of .upgma.newick)"""
    order = sorted(range(len(run_clusters)), key=lambda c: min(run_clusters[c]))
    rank = {c: q for q, c in enumerate(order)}
    cid = list(range(n))
    next_id = n
    out, lines = [], []
    for q, c in enumerate(order):
        mine = merges[first[q]:first[q + 1]]
        assert len(mine) == len(run_clusters[c]) - 1
        for a, b, na, nb, s in mine:
            lines.append("%d\t%d\t%.6f\t%d\n" % (cid[a], cid[b], distance(s, na, nb), na + nb))
            cid[a] = next_id
            next_id += 1
        out += RL.clusters_of(sorted(run_clusters[c]), cut(mine, threshold))
    trees = [newick(label, c, merges[first[rank[i]]:first[rank[i] + 1]]) + "\n" for i, c in enumerate(run_clusters)]
    return sorted(out), "".join(lines), "".join(trees)


def as_tuples(records):
    return [(int(r["a"]), int(r["b"]), int(r["size_a"]), int(r["size_b"]), int(r["sum"])) for r in records]


def as_records(merges, dtype):
    out = np.zeros(len(merges), dtype=dtype)
    for i, (a, b, na, nb, s) in enumerate(merges):
        out[i] = (a, b, na, nb, s)
    return out
