"""rtc_silhouette and rtc_cluster_quality (include/rtclust.h) restated in Python integers, the dense silhouette they must agree
with in fractions, and the two reports of clust-mst --quality restated from their rules."""
import math
from fractions import Fraction

import numpy as np

ONE = 1 << 20
NONE = 0xFFFFFFFF
SIL_DT = np.dtype([("a_num", "<u8"), ("b_num", "<u8"), ("a_den", "<u4"), ("b_den", "<u4"), ("b_cluster", "<u4"), ("far_q", "<u4"),
                   ("near_q", "<u4"), ("near_cluster", "<u4")])
FIELDS = SIL_DT.names


def check_arguments(n, edges, labels):
    """the argument errors of rtc_silhouette, in its order: the first bad record, then the first bad label, then a pair given twice"""
    if n >= (1 << 31) - 1:
        raise ValueError("%d vertices" % n)
    for e, (u, v, q) in enumerate(edges):
        if u >= n or v >= n or u == v or q > ONE or q < 0:
            raise ValueError("record %d" % e)
    bad = np.flatnonzero(np.asarray(labels) >= n)
    if len(bad):
        raise ValueError("label of vertex %d" % bad[0])
    seen = set()
    for e, (u, v, _) in enumerate(edges):
        key = (min(u, v), max(u, v))
        if key in seen:
            raise ValueError("record %d gives a pair a second time" % e)
        seen.add(key)


def silhouette(n, edges, labels, check=True):
    """SIL_DT records of n vertices under labels from the records (u, v, q).  A vertex without a record is filled in numpy, so
    only the label array and the output are as long as n."""
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert lab.shape == (n,)
    edges = [(int(u), int(v), int(q)) for u, v, q in edges]
    if check:
        check_arguments(n, edges, lab)
    out = np.zeros(n, dtype=SIL_DT)
    out["b_cluster"] = NONE
    out["near_cluster"] = NONE
    if n == 0:
        return out
    clustered = lab >= 0
    size = np.bincount(lab[clustered], minlength=n) if clustered.any() else np.zeros(n, dtype=np.int64)
    total = int(clustered.sum())
    own = np.where(clustered, size[np.where(clustered, lab, 0)], 0)
    # a vertex none of whose listed neighbours is clustered: every distance is ONE
    out["a_num"] = np.where(clustered, (own - 1) * ONE, 0)
    out["a_den"] = np.where(clustered, own - 1, 0)
    others = clustered & (total > own)
    out["b_num"] = np.where(others, ONE, 0)
    out["b_den"] = np.where(others, 1, 0)
    out["far_q"] = np.where(clustered & (own > 1), ONE, 0)
    out["near_q"] = np.where(clustered, ONE, 0)
    rows = {}
    for u, v, q in edges:
        if lab[u] < 0 or lab[v] < 0:
            continue  # an unclustered vertex is no member of anything
        rows.setdefault(u, []).append((v, q))
        rows.setdefault(v, []).append((u, q))
    for x, row in rows.items():
        c = int(lab[x])
        cnt, tot = {}, {}
        far, near = 0, (ONE, NONE)
        for y, q in row:
            d = int(lab[y])
            cnt[d] = cnt.get(d, 0) + 1
            tot[d] = tot.get(d, 0) + q
            if d == c:
                far = max(far, q)
            else:
                near = min(near, (q, d))
        n_c = int(size[c])
        r = out[x]
        r["a_num"] = tot.get(c, 0) + (n_c - 1 - cnt.get(c, 0)) * ONE
        r["far_q"] = ONE if cnt.get(c, 0) < n_c - 1 else far
        best = None  # (S, N, d), the least S / N, then the least d
        for d in cnt:
            if d == c:
                continue
            n_d = int(size[d])
            s_d = tot[d] + (n_d - cnt[d]) * ONE
            if best is None or s_d * best[1] < best[0] * n_d or (s_d * best[1] == best[0] * n_d and d < best[2]):
                best = (s_d, n_d, d)
        if best is not None and best[0] < best[1] * ONE:
            r["b_num"], r["b_den"], r["b_cluster"] = best
        r["near_q"], r["near_cluster"] = near
    return out


def value(rec):
    """rtc_silhouette_value: Python's float operations are IEEE double operations"""
    a_num, b_num, a_den, b_den = int(rec["a_num"]), int(rec["b_num"]), int(rec["a_den"]), int(rec["b_den"])
    if a_den == 0 or b_den == 0:
        return 0.0
    a = float(a_num) / (float(a_den) * 1048576.0)
    b = float(b_num) / (float(b_den) * 1048576.0)
    hi = a if a > b else b
    if hi == 0.0:
        return 0.0
    return (b - a) / hi


def dense(n, edges, labels):
    """The textbook silhouette over the full n x n matrix in fractions, unlisted pairs at ONE: per vertex None for an unclustered
    one, else (a, b, b_cluster, far, near): a and b the mean distances as Fractions in units of 2^-20 (None where there is no other
    member / no other cluster), b_cluster the nearest cluster by mean (least id among equals), far the largest distance to a
    member of the own cluster (0 for a singleton), near the least distance to a clustered vertex outside it (ONE if none)."""
    D = [[ONE] * n for _ in range(n)]
    for u, v, q in edges:
        D[u][v] = D[v][u] = int(q)
    members = {}
    for x in range(n):
        if labels[x] >= 0:
            members.setdefault(int(labels[x]), []).append(x)
    out = []
    for x in range(n):
        if labels[x] < 0:
            out.append(None)
            continue
        c = int(labels[x])
        mine = [y for y in members[c] if y != x]
        a = Fraction(sum(D[x][y] for y in mine), len(mine)) if mine else None
        far = max((D[x][y] for y in mine), default=0)
        b, b_cluster, near = None, NONE, ONE
        for d in sorted(members):
            if d == c:
                continue
            mean = Fraction(sum(D[x][y] for y in members[d]), len(members[d]))
            if b is None or mean < b:
                b, b_cluster = mean, d
            near = min(near, min(D[x][y] for y in members[d]))
        out.append((a, b, b_cluster, far, near))
    return out


def quantise(distance):
    """q of a distance: min(ONE, llround(distance 2^20)); llround rounds halves away from zero, distances are not negative"""
    x = distance * 1048576.0
    whole = math.floor(x)
    return min(ONE, whole + 1 if x - whole >= 0.5 else whole)  # x - whole is exact


def cluster_quality(sketches, labels, kmer_size, distance, matrix=False):
    """rtc_cluster_quality by brute force: every pair that shares a hash is a record at quantise(distance(common, |u| + |v| -
    common, kmer_size)), distance the library's rtc_linkage_distance.  common is numpy's set intersection pair by pair; matrix:
    all intersections at once as the product of the sets' membership matrix with its transpose (for a few hundred sketches over
    a small universe).  Returns (records, edges)."""
    sets = [np.unique(np.asarray(s)) for s in sketches]
    n = len(sets)
    if matrix:
        universe, where = np.unique(np.concatenate(sets), return_inverse=True)
        member = np.zeros((n, len(universe)), dtype=np.int64)
        at = 0
        for g, s in enumerate(sets):
            member[g, where[at:at + len(s)]] = 1
            at += len(s)
        count = member @ member.T
    edges = []
    for u in range(n):
        for v in range(u):
            common = int(count[u, v]) if matrix else len(np.intersect1d(sets[u], sets[v], assume_unique=True))
            if common:
                edges.append((u, v, quantise(distance(common, len(sets[u]) + len(sets[v]) - common, kmer_size))))
    return silhouette(n, edges, labels), edges


def reports(names, clusters, rec):
    """(quality_tsv, silhouette_tsv) of clust-mst --quality from the records: clusters in the order and with the numbers the result
    file prints, members summed in ascending genome order, every value %.6f"""
    n = len(names)
    sil = [value(rec[g]) for g in range(n)]
    label = [-1] * n
    q = "cluster\tsize\tmean_silhouette\tmin_silhouette\tmean_intra_distance\tdiameter\tseparation\tnearest_cluster\n"
    for c, mem in enumerate(clusters):
        mem = sorted(mem)
        total, a_total = 0.0, 0
        for g in mem:
            label[g] = c
            total += sil[g]
            a_total += int(rec[g]["a_num"])
        size = len(mem)
        mean = total / float(size)
        intra = float(a_total) / (float(size) * float(size - 1) * 1048576.0) if size > 1 else 0.0
        far = max(int(rec[g]["far_q"]) for g in mem)
        near = min(int(rec[g]["near_q"]) for g in mem)
        holder = next(g for g in mem if int(rec[g]["near_q"]) == near)
        nearest = int(rec[holder]["near_cluster"])
        q += "%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%s\n" % (c, size, mean, min(sil[g] for g in mem), intra, far / 1048576.0, near / 1048576.0,
                                                         "-" if nearest == NONE else str(nearest))
    total = 0.0
    for g in range(n):
        total += sil[g]
    q += "all\t%d\t%.6f\t-\t-\t-\t-\t-\n" % (n, total / float(n) if n else 0.0)
    s = "name\tcluster\tsilhouette\ta\tb\tb_cluster\n"
    for g in range(n):
        r = rec[g]
        a = float(int(r["a_num"])) / (float(int(r["a_den"])) * 1048576.0) if r["a_den"] else 0.0
        b = float(int(r["b_num"])) / (float(int(r["b_den"])) * 1048576.0) if r["b_den"] else 0.0
        s += "%s\t%d\t%.6f\t%.6f\t%.6f\t%s\n" % (names[g], label[g], sil[g], a, b, "-" if int(r["b_cluster"]) == NONE else str(int(r["b_cluster"])))
    return q, s
