"""Line-by-line restatement of the reference's KSSD DBSCAN (src/dbscan.cpp of the RabbitTClust tree), the yardstick of
clust-dbscan --fast: the neighbour test findNeighborsKSSDWithIndex (:366-612) with the inverted index of
buildInvertedIndexCSR32 (:95-130), the sequential walk of KssdDBSCAN (:725-985) and printKssdDBSCANResult (:1212-1310).
Python floats are IEEE doubles and math.exp is the C library's exp, so the predicate is restated bit for bit.  Also the
closed form the GPU computes, for the CPU check that the two agree."""
import math

import numpy as np


def jaccard_min(eps, kmer_size):
    x = math.exp(-eps * kmer_size)  # :751
    return x / (2.0 - x)            # :752


def kept_hashes(sketches, max_posting):
    """buildInvertedIndexCSR32 (:95-130): the hashes whose posting list is kept (every hash when max_posting <= 0)."""
    counts = {}
    for s in sketches:
        for h in s.tolist():
            counts[h] = counts.get(h, 0) + 1
    return {h for h, c in counts.items() if not (max_posting > 0 and c > max_posting)}


def neighbour_lists(sketches, eps, kmer_size, use64, max_posting=0):
    """findNeighborsKSSDWithIndex for every point: list of neighbour lists (ascending)."""
    t = jaccard_min(eps, kmer_size)
    n = len(sketches)
    sizes = [len(s) for s in sketches]
    out = [[] for _ in range(n)]
    if use64:
        # the brute force (:383-445): every other u64 sketch, the exact merge count, no saturation, no pruning
        sets = [np.asarray(s, dtype=np.uint64) for s in sketches]
        for p in range(n):
            one_plus_t = 1.0 + t
            size1 = sizes[p]
            t_times_size1 = t * float(size1)
            min_size = math.floor(t * size1) if t > 0.0 else 0
            max_size = math.ceil(float(size1) / t) if t > 0.0 else float("inf")
            for i in range(n):
                if i == p:
                    continue
                size2 = sizes[i]
                if size2 < min_size or size2 > max_size:
                    continue
                common = len(np.intersect1d(sets[p], sets[i], assume_unique=True))
                lhs = float(common) * one_plus_t
                rhs = t_times_size1 + t * float(size2)
                if lhs + 1e-12 < rhs:
                    continue
                out[p].append(i)
        return out
    kept = kept_hashes(sketches, max_posting)
    pruned = [np.asarray(sorted(h for h in s.tolist() if h in kept), dtype=np.uint32) for s in sketches]
    # posting lists of the kept hashes
    post = {}
    for g, s in enumerate(pruned):
        for h in s.tolist():
            post.setdefault(h, []).append(g)
    for p in range(n):
        size_ref = sizes[p]
        if size_ref == 0:
            continue  # :470-473
        size_ref16 = 65535 if size_ref > 65535 else size_ref  # :474
        min_size = int(math.floor(t * size_ref)) if t > 0.0 else 0
        max_size = int(math.ceil(float(size_ref) / t)) if t > 0.0 else 2 ** 31 - 1
        cnt = {}
        touched = []
        for h in pruned[p].tolist():  # the posting scan (:486-507)
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
        for c in touched:  # the evaluation (:555-586)
            common = cnt[c]
            size_qry = sizes[c]
            if size_qry == 0:
                continue
            if size_qry < min_size or size_qry > max_size:
                continue
            lhs = float(common) * one_plus_t
            rhs = t_times_size_ref + t * float(size_qry)
            if lhs + 1e-12 < rhs:
                continue
            out[p].append(c)
    return out


def sequential_walk(nbrs, min_pts):
    """KssdDBSCAN's loop (:807-948) over given neighbour lists: labels (>= 0 cluster, -2 noise, as the reference keeps them
    before printing), and the number of core points it counted."""
    n = len(nbrs)
    labels = [-1] * n
    cluster_id = 0
    core_points = 0
    for i in range(n):
        if labels[i] != -1:
            continue
        neighbours = nbrs[i]
        if len(neighbours) + 1 < min_pts:  # :845
            labels[i] = -2
            continue
        core_points += 1
        labels[i] = cluster_id
        seed, inq = [], set()
        for nb in neighbours:
            if nb not in inq:
                seed.append(nb)
                inq.add(nb)
        head = 0
        while head < len(seed):
            q = seed[head]
            head += 1
            if labels[q] == -2:  # noise joins the cluster, is not expanded (:881-887)
                labels[q] = cluster_id
                continue
            if labels[q] != -1:
                continue
            labels[q] = cluster_id
            qn = nbrs[q]
            if len(qn) + 1 >= min_pts:  # :906
                core_points += 1
                for nb in qn:
                    if (labels[nb] == -1 or labels[nb] == -2) and nb not in inq:
                        seed.append(nb)
                        inq.add(nb)
        cluster_id += 1
    return labels, core_points


def closed_form(nbrs, min_pts):
    """The GPU's formulation: components of the core points over core-core edges, numbered by smallest core
    index; a border point takes the lowest number among its core neighbours'; -1 noise."""
    n = len(nbrs)
    core = [len(nbrs[v]) + 1 >= min_pts for v in range(n)]
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


def labels_of(sketches, eps, min_pts, kmer_size, use64, max_posting=0):
    """KssdDBSCAN's labels with noise as -1 (what rtc_dbscan returns)."""
    lab, _ = sequential_walk(neighbour_lists(sketches, eps, kmer_size, use64, max_posting), min_pts)
    return np.array([x if x >= 0 else -1 for x in lab], dtype=np.int32)


def print_result(labels, genomes, by_file, eps, min_pts):
    """printKssdDBSCANResult (:1212-1310) as text.  genomes: per point (fileName, totalSeqLength, name, comment) with -l, or
    (name, length, comment) without.  Members in ascending index order, noise after the clusters, one point each.  The -l
    layout prints the 64-bit totalSeqLength with %12d (:1250-1251): its low 32 bits as a signed int, negative from 2^31 on."""
    ncl = max([x for x in labels] + [-1]) + 1
    clusters = [[] for _ in range(ncl)]
    noise = []
    for i, x in enumerate(labels):
        (noise if x < 0 else clusters[x]).append(i)
    out = ["# DBSCAN clustering parameters: eps=%.6f, minPts=%d\n" % (eps, min_pts), "# Total clusters: %d\n" % ncl]
    if noise:
        out.append("# Total noise points (outliers): %d\n" % len(noise))
    out.append("#\n")

    def line(j, cur):
        g = genomes[cur]
        if by_file:
            return "\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n" % (j, cur, (g[1] + 2 ** 31) % 2 ** 32 - 2 ** 31, g[0], g[2], g[3])
        return "\t%6d\t%6d\t%12dnt\t%20s\t%s\n" % (j, cur, g[1], g[0], g[2])
    for i, c in enumerate(clusters):
        out.append("the cluster %d is: \n" % i)
        out.extend(line(j, cur) for j, cur in enumerate(c))
        out.append("\n")
    for i, cur in enumerate(noise):
        out.append("the cluster %d is: \n" % (ncl + i))
        out.append(line(0, cur))
        out.append("\n")
    return "".join(out)
