"""Python restatement of the reference's clust-mst post-processing, written from the cited lines (not a copy):
the MST edge-length analysis behind --auto-threshold / --stability (src/MST.cpp:1743-2376) and the --dedup-dist /
--reps-per-cluster functions (src/cluster_postprocess.cpp).  Floats are IEEE doubles as in C++, and every sum is taken in
the reference's order, so the results carry its rounding.  Edges are (preNode, sufNode, dist) tuples."""
import math
from bisect import bisect_right
from collections import deque


# ---- forest helpers (generateForest / generateClusterWithBfs, src/MST.cpp:77-85, :109-142) ----
def forest(mst, threshold):
    return [e for e in mst if e[2] <= threshold]


def clusters_bfs(edges, n):
    adj = [[] for _ in range(n)]
    for a, b, _ in edges:
        adj[a].append(b)
        adj[b].append(a)
    seen, out = [False] * n, []
    for i in range(n):
        if seen[i]:
            continue
        seen[i] = True
        q, cl = deque([i]), [i]
        while q:
            u = q.popleft()
            for v in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    q.append(v)
                    cl.append(v)
        out.append(cl)
    return out


# ---- analyzeEdgeLengthDistribution (:1742-1816) ----
def edge_stats(mst):
    d = sorted(e[2] for e in mst if e[2] > 1e-10)
    s = dict(min=0.0, max=0.0, median=0.0, q1=0.0, q3=0.0, mean=0.0, std=0.0, sorted=d)
    n = len(d)
    if n == 0:
        return s
    s["min"], s["max"] = d[0], d[-1]
    if n == 1:
        s["median"] = s["mean"] = s["q1"] = s["q3"] = d[0]
        return s
    s["median"] = (d[n // 2 - 1] + d[n // 2]) / 2.0 if n % 2 == 0 else d[n // 2]
    s["q1"] = d[max(0, n // 4)]
    s["q3"] = d[min(n - 1, 3 * n // 4)]
    tot = 0.0
    for x in d:
        tot += x
    s["mean"] = tot / n
    var = 0.0
    for x in d:
        var += (x - s["mean"]) * (x - s["mean"])
    s["std"] = math.sqrt(var / n)
    return s


# ---- computeThresholdStability (:1827-1955): (overall, split, merge, near_edge_count) ----
def stability(mst, thr, nv, eps=0.01, samples=5, min_near=100):
    if nv <= 0 or not mst:
        return 0.5, 0.5, 0.5, 0
    lo, hi = max(0.0, thr - eps), thr + eps
    cur, near = eps, []
    while len(near) < min_near and cur <= thr * 0.5:
        lo, hi = max(0.0, thr - cur), thr + cur
        near = [e[2] for e in mst if lo <= e[2] <= hi]
        if len(near) < min_near:
            cur *= 1.5
    if not near:
        return 1.0, 1.0, 1.0, 0
    near.sort()
    step = (hi - lo) / (samples - 1) if samples > 1 else 0.0
    tot = sp = mg = 0.0
    nt = ns = nm = 0
    for s in range(samples):
        t = lo + s * step
        if t < 0.0:
            continue
        if abs(t - thr) < 1e-10:
            c = 1.0
        else:
            flips = bisect_right(near, max(thr, t)) - bisect_right(near, min(thr, t))
            c = (len(near) - flips) / len(near)
        tot += c
        nt += 1
        if t < thr:
            sp += c
            ns += 1
        elif t > thr:
            mg += c
            nm += 1
    overall, split, merge = 0.5, 0.5, 0.5
    if nt:
        overall = tot / nt
    if ns:
        split = sp / ns
    if nm:
        merge = mg / nm
    return min(split, merge), split, merge, len(near)


def _level(t):
    for lim, name in ((0.001, "identical/near-identical"), (0.005, "strain/subspecies"), (0.01, "strain"), (0.03, "species"),
                      (0.1, "genus"), (0.2, "family")):
        if t < lim:
            return name
    return "higher"


def _cand(thr, gap, idx, conf, level):
    return dict(threshold=thr, gap=gap, edge_index=idx, confidence=conf, level=level, stab=0.5, split=0.5, merge=0.5,
                clusters=0, near=0)


def _fill(c, mst, enable, nv):
    if nv <= 0:
        return
    if enable:
        c["stab"], c["split"], c["merge"], c["near"] = stability(mst, c["threshold"], nv)
    c["clusters"] = len(clusters_bfs(forest(mst, c["threshold"]), nv))


# ---- findThresholdCandidates (:1957-2178).  Equal gaps: the test inputs have none (std::sort's order is not restated) ----
def candidates(mst, max_c, ratio, enable, nv):
    if len(mst) < 2:
        return []
    st = edge_stats(mst)
    d = st["sorted"]
    rng = st["max"] - st["min"]
    if rng <= 1e-10:
        t = st["median"]
        lvl = "strain" if t < 0.01 else "species" if t < 0.03 else "genus" if t < 0.1 else "higher"
        c = _cand(t, 0.0, -1, 0.5, lvl)
        _fill(c, mst, enable, nv)
        return [c]
    min_gap = rng * ratio
    gaps = [(d[i] - d[i - 1], i) for i in range(1, len(d)) if d[i] - d[i - 1] > min_gap]
    gaps.sort(key=lambda g: -g[0])
    out = []
    for gap, i in gaps[:max_c]:
        c = _cand(d[i], gap, i, min(1.0, gap / rng * 10.0), _level(d[i]))
        _fill(c, mst, enable, nv)
        out.append(c)
    pct = ([st["q1"]] if st["q1"] >= 0.001 else []) + [st["median"], st["q3"]]
    for t in pct:
        if t < 0.001:
            continue
        if any(abs(c["threshold"] - t) < min_gap * 0.5 for c in out):
            continue
        if st["min"] < t < st["max"]:
            c = _cand(t, 0.0, -1, 0.4, _level(t))
            _fill(c, mst, enable, nv)
            out.append(c)
    out.sort(key=lambda c: c["threshold"])
    return out


# ---- selectOptimalThreshold (:2180-2269); fields the reference leaves unset keep the candidate defaults ----
def optimal(cands, mst):
    if not cands:
        return _cand(0.05, 0.0, -1, 0.0, "unknown")
    best, opt, found = -1.0, _cand(0.0, 0.0, -1, 0.0, ""), False
    for c in cands:
        t = c["threshold"]
        if t < 0.001:
            continue
        score = c["confidence"]
        if 0.01 <= t <= 0.1:
            score *= 2.0
            found = True
        elif 0.001 <= t < 0.01:
            score *= 1.2
        elif 0.1 < t <= 0.2:
            score *= 1.1
        if c["gap"] > 0.0:
            score += c["gap"] * 20.0
        if score > best:
            best, opt = score, dict(c)
    if not found and best < 0:
        med = edge_stats(mst)["median"]
        if 0.01 <= med <= 0.2:
            opt.update(threshold=med, confidence=0.4, level="species" if med < 0.03 else "genus" if med < 0.1 else "family")
        else:
            opt.update(threshold=0.05, confidence=0.3, level="genus")
        opt.update(gap=0.0, edge_index=-1)
    return opt


# ---- printThresholdAnalysis (:2271-2376): the file's text ----
def analysis_text(mst, ratio, enable, nv):
    st = edge_stats(mst)
    cs = candidates(mst, 5, ratio, enable, nv)
    o = optimal(cs, mst)
    L = ["# Automatic Threshold Selection Analysis", "# Based on MST Edge Length Distribution",
         "# ===========================================", "", "## Edge Length Statistics", "Total edges: %d" % len(mst),
         "Min distance: %.6f" % st["min"], "Max distance: %.6f" % st["max"], "Mean distance: %.6f" % st["mean"],
         "Median distance: %.6f" % st["median"], "Q1 (25%%): %.6f" % st["q1"], "Q3 (75%%): %.6f" % st["q3"],
         "Standard deviation: %.6f" % st["std"], "Range: %.6f" % (st["max"] - st["min"]), "",
         "## Optimal Threshold (Recommended)", "Threshold: %.6f" % o["threshold"], "Confidence: %.3f" % o["confidence"]]
    if o["clusters"] > 0 or o["stab"] != 0.5:
        L.append("Stability (overall): %.3f" % o["stab"])
        if o["split"] != 0.5 or o["merge"] != 0.5:
            L.append("  - Split sensitivity: %.3f (stability when threshold decreases)" % o["split"])
            L.append("  - Merge sensitivity: %.3f (stability when threshold increases)" % o["merge"])
        if o["near"] > 0:
            L.append("  - Near edges evaluated: %d" % o["near"])
        L.append("Number of clusters: %d" % o["clusters"])
    L.append("Suggested level: %s" % o["level"])
    if o["edge_index"] >= 0:
        L += ["Edge index: %d" % o["edge_index"], "Gap score: %.6f" % o["gap"],
              "Source: gap-based detection (natural breakpoint in edge distribution)"]
    else:
        L += ["Source: percentile-based (median/quartile, no significant gap detected)",
              "Note: This threshold is based on distribution statistics, not natural breakpoints.",
              "      Consider manual adjustment (e.g., 0.01-0.05 for species/genus level) if needed."]
    L += ["", "## All Candidate Thresholds"]
    if any(c["clusters"] > 0 or c["stab"] != 0.5 for c in cs):
        L.append("# Threshold\tConfidence\tStability_Overall\tStability_Split\tStability_Merge\tNear_Edges\tClusters\tLevel\t"
                 "Gap_Score\tEdge_Index")
        L += ["%.6f\t%.3f\t%.3f\t%.3f\t%.3f\t%d\t%d\t%s\t%.6f\t%d" % (c["threshold"], c["confidence"], c["stab"], c["split"],
                                                                     c["merge"], c["near"], c["clusters"], c["level"], c["gap"],
                                                                     c["edge_index"]) for c in cs]
    else:
        L.append("# Threshold\tConfidence\tLevel\tGap_Score\tEdge_Index")
        L += ["%.6f\t%.3f\t%s\t%.6f\t%d" % (c["threshold"], c["confidence"], c["level"], c["gap"], c["edge_index"]) for c in cs]
    L += ["", "## Edge Length Distribution (sorted)", "# Index\tDistance"]
    L += ["%d\t%.6f" % (i, x) for i, x in enumerate(st["sorted"])]
    return "\n".join(L) + "\n", o


# ---- build_dedup_candidates_per_cluster_core (src/cluster_postprocess.cpp:60-156) ----
def _tree_dist(start, adj, nodes):
    """distances_from (:33-54) restricted to `nodes`' component: accumulated outward from start, one add per edge"""
    dist, parent, st = {start: 0.0}, {start: start}, [start]
    while st:
        u = st.pop()
        for v, w in adj[u]:
            if v == parent[u]:
                continue
            parent[v] = u
            dist[v] = dist[u] + w
            st.append(v)
    return dist


def tree_medoids(n, edges, dedup, seq_len):
    """node_to_rep[n]"""
    if dedup <= 0:
        return list(range(n))
    up = list(range(n))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    adj = [[] for _ in range(n)]
    for a, b, w in edges:
        if w <= dedup:
            up[find(a)] = find(b)
            adj[a].append((b, w))
            adj[b].append((a, w))
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    rep = list(range(n))
    for mem in groups.values():
        if len(mem) == 1:
            continue
        chosen, best, clen = mem[0], math.inf, 0
        for c in mem:
            dist = _tree_dist(c, adj, mem)
            tot = 0.0
            for m in mem:
                if m != c and dist.get(m, -1.0) >= 0:
                    tot += dist[m]
            ln = seq_len[c]
            if tot < best or (tot == best and (ln > clen or (ln == clen and c < chosen))):
                chosen, best, clen = c, tot, ln
        for m in mem:
            rep[m] = chosen
    return rep


def dedup_candidates(clusters, rep, dedup):
    if dedup <= 0:
        return [list(c) for c in clusters]
    return [sorted(set(rep[v] for v in cl)) for cl in clusters]


# ---- select_k_reps_per_cluster_tree (:192-329) ----
def select_k_reps(clusters, cands, edges, n, rep, k):
    if k <= 0:
        return [[] for _ in clusters]
    adj = [[] for _ in range(n)]
    for a, b, w in edges:
        adj[a].append((b, w))
        adj[b].append((a, w))
    out = []
    for comp, cand in zip(clusters, cands):
        if not cand:
            out.append([])
            continue
        if len(cand) <= k:
            out.append(list(cand))
            continue
        m = len(comp)
        idx = {v: i for i, v in enumerate(comp)}
        ladj = [[(idx[v], w) for v, w in adj[u] if v in idx] for u in comp]

        def dists(s):
            d = _tree_dist(s, ladj, None)
            return [d.get(i, -1.0) for i in range(m)]

        def farthest(s):
            d = dists(s)
            far, best = s, -1.0
            for i in range(m):
                if d[i] > best:
                    best, far = d[i], i
            return far

        u = farthest(0)
        v = farthest(u)
        cs = set(cand)

        def to_cand(node):
            r = rep[node]
            return r if r in cs else node if node in cs else cand[0]

        chosen = [to_cand(comp[u])]
        if len(chosen) < k and to_cand(comp[v]) not in chosen:
            chosen.append(to_cand(comp[v]))
        mind = [math.inf] * m

        def add(r):
            if r not in idx:
                return
            d = dists(idx[r])
            for i in range(m):
                if d[i] >= 0.0 and d[i] < mind[i]:
                    mind[i] = d[i]

        for r in chosen:
            add(r)
        cl = [idx[c] for c in cand if c in idx]
        while len(chosen) < k:
            bi, bs = -1, -1.0
            for li in cl:
                if to_cand(comp[li]) in chosen:
                    continue
                if mind[li] > bs:
                    bs, bi = mind[li], li
            if bi < 0:
                break
            nx = to_cand(comp[bi])
            if nx in chosen:
                break
            chosen.append(nx)
            add(nx)
        out.append(sorted(chosen))
    return out


def dedup_and_reps(n, forest_edges, seq_len, dedup, k):
    """(node_to_rep, clusters, candidates, reps) of the forest as clust-mst --fast computes them"""
    rep = tree_medoids(n, forest_edges, dedup, seq_len)
    cl = clusters_bfs(forest_edges, n)
    cd = dedup_candidates(cl, rep, dedup)
    return rep, cl, cd, select_k_reps(cl, cd, forest_edges, n, rep, k)


def result_text(clusters, genomes, by_file=True, threshold=None):
    """printResult / print_result's text for genomes [(file, name, comment, length)]"""
    L = []
    if threshold is not None:
        L += ["# Clustering threshold: %.6f" % threshold, "# Total clusters: %d" % len(clusters), "#"]
    for i, cl in enumerate(clusters):
        L.append("the cluster %d is: " % i)
        for j, g in enumerate(cl):
            fn, name, cm, length = genomes[g]
            if by_file:
                L.append("\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s" % (j, g, length, fn, name, cm))
            else:
                L.append("\t%6d\t%6d\t%12dnt\t%20s\t%s" % (j, g, length, name, cm))
        L.append("")
    return "\n".join(L) + "\n" if L else ""
