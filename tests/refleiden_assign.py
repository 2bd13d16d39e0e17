"""Restatement of clust-leiden --db --assign (include/rtclust.h: rtc_graph_query, rtc_leiden_place), brute force with Python
integers: a query against every model genome.

  - jstar(): rtc_graph_build's J*, the bisection over the bit patterns of the doubles in [0, 1] through the distance function
    of tests/refgraph.py (from the quotient on), moved past every failing double within 64 ulps above the flip;
  - graph_query(): C(x) by the edge rule, E(x) by the exact rank, and the `nearest` record over all candidates;
  - quantise(): the model's own quantisation of one weight (the host's leiden_quantise for one record);
  - place(): e_d, k_x, the 128-bit scores as Python integers, label and runner-up;
  - assign(): the two chained with the weights of rtc_graph_weight (the library's host function, through ctypes: the very
    doubles the command line forms), and tsv_line(): the command line's output.
  - model_sums(): k_p, tot_d, M2 and N_d of a run's records and labels."""
import math
import struct
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
CPM, MODULARITY = 0, 1


def _bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def _dbl(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _dist_of_jaccard(j, k):
    if j <= 0.0:
        return 1.0
    if j >= 1.0:
        return 0.0
    return max(0.0, min(1.0, -1.0 / k * math.log(2.0 * j / (1.0 + j))))


def jstar(threshold, k):
    if _dist_of_jaccard(0.0, k) < threshold:
        return 0.0
    lo, hi = _bits(0.0), _bits(1.0)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if _dist_of_jaccard(_dbl(mid), k) < threshold:
            hi = mid
        else:
            lo = mid
    top = min(hi + 64, _bits(1.0))
    for b in range(top, hi, -1):
        if not _dist_of_jaccard(_dbl(b), k) < threshold:
            hi = b + 1
            break
    return _dbl(hi)


def graph_query(model, queries, threshold, kmer_size, knn_k=0):
    """-> (edges [(q, p, common)] in (q, p) order, near [(nearest, common, denom, n_candidates, n_passing, n_kept)])"""
    js = jstar(threshold, kmer_size)
    msets = [set(int(h) for h in s) for s in model]
    edges, near = [], []
    for qi, x in enumerate(queries):
        xs = set(int(h) for h in x)
        cand, passing = [], []
        for p, ps in enumerate(msets):
            common = len(xs & ps)
            if common == 0:
                continue
            a, b = len(xs), len(ps)
            union = a + b - common
            cand.append((p, common, union))
            if not 2 * min(a, b) < max(a, b) and float(common) / float(union) >= js:
                passing.append((p, common, union))
        kept = passing
        if knn_k > 0 and len(passing) > knn_k:
            kept = sorted(passing, key=lambda r: (-Fraction(r[1], r[2]), r[0]))[:knn_k]
        edges += [(qi, p, c) for p, c, _ in sorted(kept)]
        if cand:
            p, c, u = min(cand, key=lambda r: (-Fraction(r[1], r[2]), r[0]))
            near.append((p, c, u, len(cand), len(passing), len(kept)))
        else:
            near.append((NONE, 0, 0, 0, 0, 0))
    return edges, near


def _llround(x):
    f = math.floor(x)
    r = int(f) + (1 if x - f >= 0.5 else 0)
    if x < 0 and x - f == 0.5:  # halves go away from zero
        r = int(f)
    return r


def quantise(w, objective, scale=False, lo=0.0, rng=1.0):
    """q of one weight as the model's run formed it; 0: the record is dropped"""
    x = (w - lo) / rng if (objective == CPM and scale) else w
    q = _llround(x * 1048576.0)
    if objective != CPM and q < 1:
        q = 1
    if q < 1:
        return 0
    return min(q, 0xFFFFFFFF)


def place(records, labels, objective, g, tot, m2=0):
    """records [(p, q)] of ONE query (duplicates summed), tot[d]: N_d (CPM) or tot_d -> (label, runner_up, n_edges, n_comms, k_x,
    e_label, e_runner); ValueError where the call refuses (M2 + 2 k_x >= 2^46)"""
    e, seen, k_x = {}, set(), 0
    for p, q in records:
        assert q >= 1
        d = int(labels[p])
        e[d] = e.get(d, 0) + int(q)
        seen.add(p)
        k_x += int(q)
    if objective == MODULARITY and m2 + 2 * k_x >= 1 << 46:
        raise ValueError("unsupported")
    scored = []
    for d, ed in e.items():
        if objective == CPM:
            s = ed * 65536 - g * (1 << 20) * int(tot[d])
        else:
            s = ed * (m2 + 2 * k_x) * 65536 - g * k_x * (int(tot[d]) + ed)
        if s > 0:
            scored.append((-s, d))
    scored.sort()
    label = scored[0][1] if scored else -1
    runner = scored[1][1] if len(scored) > 1 else -1
    return (label, runner, len(seen), len(e), k_x, e.get(label, 0), e.get(runner, 0))


def place_all(n_queries, records, labels, objective, resolution, tot, m2=0):
    """records [(u, v, q)] in any order -> one place() tuple per query"""
    g = _llround(resolution * 65536.0)
    per = [[] for _ in range(n_queries)]
    for u, v, q in records:
        per[u].append((v, q))
    return [place(r, labels, objective, g, tot, m2) for r in per]


def model_sums(n, records, labels, n_clusters):
    """k_p, tot_d, M2, N_d of the records (u, v, q) a run gave rtc_louvain / rtc_leiden (k_x as the rtc_louvain comment defines
    it: u == v adds 2q to the self entry) and its labels"""
    k = [0] * n
    for u, v, q in records:
        k[u] += int(q)
        k[v] += int(q)
    tot, size = [0] * n_clusters, [0] * n_clusters
    for p in range(n):
        tot[int(labels[p])] += k[p]
        size[int(labels[p])] += 1
    return k, tot, sum(tot), size


def weights(edges, model, queries, kmer_size, weight_fn):
    return [weight_fn(c, len(set(int(h) for h in queries[q])), len(set(int(h) for h in model[p])), kmer_size) for q, p, c in edges]


def assign(model, labels, queries, threshold, kmer_size, knn_k, objective, resolution, tot, m2, scale, lo, rng, weight_fn):
    """-> (placements, near, records): the whole flow for every query; weight_fn is rtc_graph_weight"""
    edges, near = graph_query(model, queries, threshold, kmer_size, knn_k)
    records = []
    for (q, p, c), w in zip(edges, weights(edges, model, queries, kmer_size, weight_fn)):
        qq = quantise(w, objective, scale, lo, rng)
        if qq:
            records.append((q, p, qq))
    return place_all(len(queries), records, labels, objective, resolution, tot, m2), near, records


def tsv_line(name, pl, near, model_names, q_size, model_sizes, kmer_size, weight_fn):
    """one line of clust-leiden --db --assign"""
    label, runner, n_edges, n_comms, k_x, e_label, _ = pl
    share = float(e_label) / float(k_x) if (label >= 0 and k_x) else 0.0
    cols = [name, str(label) if label >= 0 else "novel", str(runner) if runner >= 0 else "-", str(n_edges), str(n_comms),
            "%.6f" % (float(e_label) / 1048576.0), "%.6f" % share]
    if near[0] == NONE:
        cols += ["-", "inf"]
    else:
        cols += [model_names[near[0]], "%.6f" % (1.0 - weight_fn(near[1], q_size, model_sizes[near[0]], kmer_size))]
    return "\t".join(cols)


def parse_model(blob):
    """a clust-leiden --db model file -> dict"""
    assert blob[:8] == b"RTCLDNM1"
    head = struct.unpack_from("<12i", blob, 8)
    names = ("version", "algorithm", "objective", "width", "by_file", "kmer_size", "half_k", "half_subk", "drlevel", "knn", "n_clusters", "scale")
    m = dict(zip(names, head))
    at = 8 + 48
    m["min_len"], m["n"], m["threshold"], m["resolution"], m["lo"], m["range"], m["m2"] = struct.unpack_from("<QQddddQ", blob, at)
    at += 56
    n, ncl = m["n"], m["n_clusters"]
    m["labels"] = np.frombuffer(blob, "<i4", n, at); at += 4 * n
    m["tot"] = np.frombuffer(blob, "<u8", ncl, at); at += 8 * ncl
    m["sections"] = {"header": 8 + 48 + 56, "labels": 8 + 48 + 56 + 4 * n, "tot": at}
    genomes = []
    for _ in range(n):
        g = {}
        for key in ("file", "name", "comment"):
            (ln,) = struct.unpack_from("<I", blob, at); at += 4
            g[key] = blob[at:at + ln].decode(); at += ln
        g["length"], g["total_length"] = struct.unpack_from("<QQ", blob, at); at += 16
        genomes.append(g)
    m["genomes"] = genomes
    m["sections"]["genomes"] = at
    lens = np.frombuffer(blob, "<u4", n, at); at += 4 * n
    m["sections"]["lengths"] = at
    w = m["width"]
    m["sketches"] = []
    for ln in lens.tolist():
        m["sketches"].append(np.frombuffer(blob, "<u8" if w == 8 else "<u4", ln, at)); at += w * ln
    assert at == len(blob)
    return m
