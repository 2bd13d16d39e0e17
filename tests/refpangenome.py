"""The definition of rtc_pangenome and rtc_pan_growth (include/rtclust.h), restated in numpy and plain Python floats: what the
GPU tests compare the library against.  Nothing here shares code with the library."""
import numpy as np

from rabbittclust_amd import api


def number_clusters(labels):
    """(cluster_of[g] or -1, sizes): clusters numbered by their smallest member; a negative label is in none"""
    labels = np.asarray(labels, dtype=np.int64)
    cluster_of = np.full(len(labels), -1, dtype=np.int64)
    number, sizes = {}, []
    for g, lab in enumerate(labels.tolist()):
        if lab < 0:
            continue
        if lab not in number:
            number[lab] = len(sizes)
            sizes.append(0)
        cluster_of[g] = number[lab]
        sizes[number[lab]] += 1
    return cluster_of, np.asarray(sizes, dtype=np.int64)


def hash_class(occ, m, soft_pct, cloud_pct):
    """0 core, 1 soft, 2 shell, 3 cloud; Python integers, so every compare is exact"""
    occ, m = int(occ), int(m)
    if occ == m:
        return 0
    if 100 * occ >= soft_pct * m:
        return 1
    if 100 * occ < cloud_pct * m:
        return 3
    return 2


def pangenome(sketches, labels, soft_pct=95, cloud_pct=15):
    """sketches: one ascending array of distinct hashes per genome.  Returns (clusters, hist, genomes) as Context.pangenome does."""
    n = len(sketches)
    cluster_of, sizes = number_clusters(labels)
    n_cl = len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    clusters = np.zeros(n_cl, dtype=api.PAN_DT)
    hist = np.zeros(n, dtype=np.uint64)
    genomes = np.zeros(n, dtype=api.PAN_GENOME_DT)
    lens = np.asarray([len(s) for s in sketches], dtype=np.int64)
    inside = cluster_of >= 0
    rec_g = np.repeat(np.arange(n, dtype=np.int64)[inside], lens[inside])
    rec_h = np.concatenate([np.asarray(sketches[g], dtype=np.uint64) for g in range(n) if inside[g]] + [np.zeros(0, dtype=np.uint64)])
    rec_c = cluster_of[rec_g]
    order = np.lexsort((rec_h, rec_c))
    sc, sh = rec_c[order], rec_h[order]
    K = len(order)
    head = np.ones(K, dtype=bool)
    head[1:] = (sc[1:] != sc[:-1]) | (sh[1:] != sh[:-1])
    run_start = np.flatnonzero(head)
    run_len = np.diff(np.concatenate([run_start, [K]]))
    run_c = sc[run_start]
    occ_sorted = np.repeat(run_len, run_len)  # occ of every record, in sorted order
    occ = np.zeros(K, dtype=np.int64)
    occ[order] = occ_sorted
    # the class of every (cluster size, occ) that occurs, through exact Python integers
    m_run = sizes[run_c]
    cls_of = {}
    for m_, f_ in set(zip(m_run.tolist(), run_len.tolist())):
        cls_of[(m_, f_)] = hash_class(f_, m_, soft_pct, cloud_pct)
    run_cls = np.asarray([cls_of[(m_, f_)] for m_, f_ in zip(m_run.tolist(), run_len.tolist())], dtype=np.int64)
    # per cluster
    clusters["size"] = sizes
    np.add.at(clusters["total"], rec_c, 1)
    np.add.at(clusters["pan"], run_c, 1)
    for k, name in enumerate(("core", "soft", "shell", "cloud")):
        np.add.at(clusters[name], run_c[run_cls == k], 1)
    np.add.at(clusters["single"], run_c[run_len == 1], 1)
    np.add.at(hist, first[run_c] + run_len - 1, 1)
    # per genome
    rec_cls = np.zeros(K, dtype=np.int64)
    rec_cls[order] = np.repeat(run_cls, run_len)
    np.add.at(genomes["unique"], rec_g[occ == 1], 1)
    np.add.at(genomes["occ_sum"], rec_g, occ.astype(np.uint64))
    for k, name in enumerate(("core", "soft", "shell", "cloud")):
        np.add.at(genomes[name], rec_g[rec_cls == k], 1)
    return clusters, hist, genomes


def cluster_hists(clusters, hist):
    """the histogram of every cluster, as a list of arrays"""
    out, at = [], 0
    for r in clusters:
        out.append(hist[at:at + int(r["size"])])
        at += int(r["size"])
    return out


def growth_points(m):
    if m <= 256:
        return list(range(1, m + 1))
    return [1 + (i * (m - 1)) // 255 for i in range(256)]


def growth(hist):
    """rtc_pan_growth: (j, pan, core) in Python floats, every step one IEEE-754 double operation in the header's order"""
    hist = [int(x) for x in hist]
    m = len(hist)
    js = growth_points(m)
    pan = [0.0] * len(js)
    core = [0.0] * len(js)
    for f in range(1, m + 1):
        k = hist[f - 1]
        if k == 0:
            continue
        u = v = 1.0
        p = 0
        for i in range(m):
            if i >= m - f:
                u = 0.0
            else:
                u = u * float(m - f - i) / float(m - i)
            v = v * float(f - i) / float(m - i)
            while p < len(js) and js[p] == i + 1:
                pan[p] = pan[p] + float(k) * (1.0 - u)
                core[p] = core[p] + float(k) * v
                p += 1
    return np.asarray(js, dtype=np.uint32), np.asarray(pan, dtype=np.float64), np.asarray(core, dtype=np.float64)


def identities(clusters, hist, genomes, labels):
    """the consequences the header states, as a list of violations (empty: all hold)"""
    bad = []
    cluster_of, sizes = number_clusters(labels)
    for c, (r, h) in enumerate(zip(clusters, cluster_hists(clusters, hist))):
        m = int(r["size"])
        h = [int(x) for x in h]
        mem = genomes[cluster_of == c]
        if int(r["core"]) + int(r["soft"]) + int(r["shell"]) + int(r["cloud"]) != int(r["pan"]):
            bad.append((c, "classes"))
        if sum(h) != int(r["pan"]):
            bad.append((c, "pan"))
        if sum((f + 1) * k for f, k in enumerate(h)) != int(r["total"]):
            bad.append((c, "total"))
        if h[m - 1] != int(r["core"]):
            bad.append((c, "core"))
        if h[0] != int(r["single"]) or int(mem["unique"].astype(np.int64).sum()) != h[0]:
            bad.append((c, "single"))
        if sum(int(x) for x in mem["occ_sum"]) != sum((f + 1) ** 2 * k for f, k in enumerate(h)):
            bad.append((c, "occ_sum"))
        if m == 1 and not (int(r["pan"]) == int(r["core"]) == int(r["single"]) == int(r["total"])):
            bad.append((c, "singleton"))
    return bad
