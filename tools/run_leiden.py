#!/usr/bin/env python
"""The graph-based family on a synthetic family set: sketches the genomes (KSSD), builds the similarity graph
(Context.graph_build) and runs the deterministic Louvain (Context.louvain), then prints both counter sets.  With --leiden it
also runs the deterministic Leiden (Context.leiden) on the same graph -- the weights quantised as the command line does for
the objective -- and prints its counters and the whole-call time of rtc_leiden beside rtc_louvain's (the best of --repeat calls
each, after one call to warm up).

    python tools/run_leiden.py --families 40 --per-family 12 [--threshold 0.05] [--knn 1000] [--resolution 1.0]
    python tools/run_leiden.py --leiden [--objective cpm|modularity] [--leiden-resolution 0.5] [--repeat 3]

With --assign M it holds M genomes of the set out, builds the model on the rest (Louvain, or with --leiden the Leiden of
--objective) and places them (clust-leiden --db --assign: Context.graph_query, the host's weights on --threads host threads,
Context.leiden_place); it prints the three times, the best of --repeat warm calls each, beside the time of the full run over
all genomes (graph_build plus the clustering call), and how many held-out genomes came back to the community of their family.

    python tools/run_leiden.py --families 200 --per-family 12 --assign 200 [--leiden --objective modularity] [--threads 16]

With --minhash the genomes are sketched with MinHash (-k 21, --sketch-size hashes) and the graph is clust-leiden --minhash's
(Context.graph_build_mash): it prints the graph's counter set (the call with the least whole-call time of --repeat warm calls)
and Louvain's, and beside them the counters of Context.dbscan_mash on the same sketches at eps = --threshold (min_pts 2), whose
pair phase and merge kernel the graph shares.

    python tools/run_leiden.py --minhash [--sketch-size 1000] [--threshold 0.05] [--knn 1000]

With --mcl it also runs the Markov clustering (Context.mcl) on Louvain's records of the same graph and prints its counter set,
the column paths it took and the whole-call time of rtc_mcl beside rtc_louvain's (the best of --repeat calls each, after one
call to warm up), and how many families came back whole.

    python tools/run_leiden.py --mcl [--inflation 2.0] [--mcl-select 1024] [--mcl-iterations 100] [--repeat 3]

With --snn it also counts the shared neighbours of the graph's edges (Context.graph_snn, clust-leiden --snn) and prints the
counter set of the call with the least whole-call time, the paths it took, the probes per second of its counting part, and the
whole-call times of rtc_graph_snn (with its adjacency and counting parts), of rtc_graph_build and of rtc_louvain on the
SNN-weighted records, all in one loop in this process: lowest and highest of --repeat calls each, after one call to warm up.

    python tools/run_leiden.py --snn [--families 20 --per-family 300 --threshold 0.15] [--repeat 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=40)
    ap.add_argument("--per-family", type=int, default=12)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--knn", type=int, default=1000)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--leiden", action="store_true")
    ap.add_argument("--objective", choices=("cpm", "modularity"), default="cpm")
    ap.add_argument("--leiden-resolution", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--assign", type=int, default=0, metavar="M")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--minhash", action="store_true")
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--mcl", action="store_true")
    ap.add_argument("--inflation", type=float, default=2.0)
    ap.add_argument("--mcl-select", type=int, default=1024)
    ap.add_argument("--mcl-iterations", type=int, default=100)
    ap.add_argument("--snn", action="store_true")
    a = ap.parse_args()
    if a.minhash and (a.leiden or a.assign or a.mcl or a.snn):
        ap.error("--minhash prints the graph's and Louvain's counters alone")
    from rabbittclust_amd import api, host
    ctx = api.Context(0)
    desc = api.synth_family_descs(a.families, a.per_family, global_seed=11)
    n = len(desc)
    off = np.arange(n + 1, dtype=np.uint64) * a.length
    seq = ctx.synth_genomes(desc, off)
    kmer = 21
    if a.minhash:
        return minhash(ctx, a, seq, off, kmer, n)
    sk = ctx.sketch_kssd(seq, off, host.generate_shuffle_dim(6), kmer_size=kmer, drlevel=3)
    ctx.sync()
    sizes = sk.len.cpu().numpy().tolist()
    edges = ctx.graph_build(sk, a.threshold, kmer, a.knn)
    graph = ctx.graph_counters()
    rec = api.graph_weights(edges, sizes, kmer)
    labels, modularity = ctx.louvain(n, rec, a.resolution, return_modularity=True)
    out = {"genomes": n, "edges": int(len(edges)), "clusters": ctx.louvain_clusters, "modularity": modularity,
           "graph": graph, "louvain": ctx.louvain_counters()}
    if a.leiden:
        weights = [api.graph_weight(c, sizes[u], sizes[v], kmer) for u, v, c in zip(edges["u"].tolist(), edges["v"].tolist(), edges["common"].tolist())]
        lrec, _ = host.leiden_quantise(edges["u"], edges["v"], weights, 0 if a.objective == "cpm" else 1)
        louvain_ns, leiden_ns = [], []
        for i in range(a.repeat + 1):  # the first call of each warms up
            ctx.louvain(n, rec, a.resolution)
            louvain_ns.append(ctx.louvain_counters()["total_ns"])
            _, quality = ctx.leiden(n, lrec, a.leiden_resolution, a.objective, return_quality=True)
            leiden_ns.append(ctx.leiden_counters()["total_ns"])
        out.update({"leiden": ctx.leiden_counters(), "leiden_objective": a.objective, "leiden_resolution": a.leiden_resolution,
                    "leiden_records": int(len(lrec)), "leiden_clusters": ctx.leiden_clusters, "leiden_quality": quality,
                    "louvain_call_ms": min(louvain_ns[1:]) / 1e6, "leiden_call_ms": min(leiden_ns[1:]) / 1e6})
    if a.mcl:
        louvain_ns, mcl_ns = [], []
        for i in range(a.repeat + 1):  # the first call of each warms up
            ctx.louvain(n, rec, a.resolution)
            louvain_ns.append(ctx.louvain_counters()["total_ns"])
            mlabels = ctx.mcl(n, rec, a.inflation, a.mcl_select, a.mcl_iterations)
            mcl_ns.append(ctx.mcl_counters()["total_ns"])
        whole = sum(1 for f in range(a.families) if len(set(mlabels[f * a.per_family:(f + 1) * a.per_family].tolist())) == 1)
        out.update({"mcl": ctx.mcl_counters(), "mcl_paths": ctx.mcl_last_path(), "mcl_inflation": a.inflation, "mcl_select": a.mcl_select,
                    "mcl_clusters": ctx.mcl_clusters, "mcl_families_whole": whole, "louvain_call_ms": min(louvain_ns[1:]) / 1e6,
                    "mcl_call_ms": min(mcl_ns[1:]) / 1e6})
    if a.snn:
        out.update(snn(ctx, a, sk, kmer, n, edges))
    if a.assign:
        out["assign"] = assign(ctx, a, sk, kmer, n)
    print(json.dumps(out))


def snn(ctx, a, sk, kmer, n, edges):
    from rabbittclust_amd import api
    build_ns, calls, louvain_ns, srec = [], [], [], None
    for i in range(a.repeat + 1):  # the first call of each warms up
        ctx.graph_build(sk, a.threshold, kmer, a.knn)
        build_ns.append(ctx.graph_counters()["total_ns"])
        shared, du, dv, _ = ctx.graph_snn(n, edges["u"], edges["v"])
        calls.append(ctx.graph_snn_counters())
        if srec is None:  # the command line's records: q = max(1, llround(w 2^20)) of the one double division
            w = (shared.astype(np.float64) + 2.0) / (du.astype(np.float64) + dv.astype(np.float64) - shared.astype(np.float64))
            srec = np.zeros(len(edges), dtype=api.WEDGE_DT)
            srec["u"], srec["v"], srec["q"] = edges["u"], edges["v"], np.maximum(1, np.floor(w * 1048576.0 + 0.5)).astype(np.uint32)
        labels = ctx.louvain(n, srec, a.resolution)
        louvain_ns.append(ctx.louvain_counters()["total_ns"])
    warm = calls[1:]
    best = min(warm, key=lambda c: c["total_ns"])
    span = lambda ns: [min(ns) / 1e6, max(ns) / 1e6]
    whole = sum(1 for f in range(a.families) if len(set(labels[f * a.per_family:(f + 1) * a.per_family].tolist())) == 1)
    return {"snn": best, "snn_paths": ctx.graph_snn_last_path(), "snn_weights": [float(w.min()), float(w.max())] if len(w) else [],
            "snn_call_ms": span([c["total_ns"] for c in warm]), "snn_adjacency_ms": span([c["adjacency_ns"] for c in warm]),
            "snn_count_ms": span([c["count_ns"] for c in warm]), "snn_probes_per_s": best["probes"] / max(best["count_ns"], 1) * 1e9,
            "graph_build_call_ms": span(build_ns[1:]), "louvain_snn_call_ms": span(louvain_ns[1:]), "snn_clusters": ctx.louvain_clusters,
            "snn_families_whole": whole}


def minhash(ctx, a, seq, off, kmer, n):
    from rabbittclust_amd import api
    sk = ctx.sketch_minhash(seq, off, k=kmer, size=a.sketch_size)
    ctx.sync()
    graph = None
    for i in range(a.repeat + 1):  # the first call warms up
        edges = ctx.graph_build_mash(sk, a.sketch_size, a.threshold, kmer, a.knn)
        c = ctx.graph_counters()
        if i and (graph is None or c["total_ns"] < graph["total_ns"]):
            graph = c
    rec = api.graph_weights_mash(edges, a.sketch_size, kmer)
    _, modularity = ctx.louvain(n, rec, a.resolution, return_modularity=True)
    out = {"sketch": "minhash", "sketch_size": a.sketch_size, "genomes": n, "edges": int(len(edges)), "clusters": ctx.louvain_clusters,
           "modularity": modularity, "graph": graph, "louvain": ctx.louvain_counters(),
           "graph_ms": {k[:-3]: graph[k] / 1e6 for k in ("pair_ns", "filter_ns", "select_ns", "total_ns")}}
    if a.threshold < 1.0:
        best = None
        for i in range(a.repeat + 1):
            ctx.dbscan_mash(sk, a.sketch_size, [a.threshold], 2, kmer)
            c = ctx.dbscan_mash_counters()
            if i and (best is None or c["total_ns"] < best["total_ns"]):
                best = c
        out["dbscan_mash"] = best
    print(json.dumps(out))


def assign(ctx, a, sk, kmer, n):
    import time
    from rabbittclust_amd import api, host
    m = min(a.assign, n - 1)
    held = set(np.linspace(0, n - 1, m).astype(int).tolist())
    sets = sk.to_host()
    keep = [g for g in range(n) if g not in held]
    hold = sorted(held)
    model, queries = [sets[g] for g in keep], [sets[g] for g in hold]
    sk_model = api.SketchSet.from_host(model, ctx.device, k=kmer, kind="kssd", width=sk.width)
    sk_all = api.SketchSet.from_host(model + queries, ctx.device, k=kmer, kind="kssd", width=sk.width)
    msz, qsz = [len(s) for s in model], [len(s) for s in queries]
    objective = (0 if a.objective == "cpm" else 1) if a.leiden else 1
    resolution = a.leiden_resolution if a.leiden else a.resolution

    def cluster(skx, sizes):
        """the full run's two device calls -> (labels, clusters, records, weights, ns)"""
        edges = ctx.graph_build(skx, a.threshold, kmer, a.knn)
        ns = ctx.graph_counters()["total_ns"]
        w = [api.graph_weight(c, sizes[u], sizes[v], kmer) for u, v, c in zip(edges["u"].tolist(), edges["v"].tolist(), edges["common"].tolist())]
        rec, _ = host.leiden_quantise(edges["u"], edges["v"], w, objective)
        if a.leiden:
            labels = ctx.leiden(skx.n, rec, resolution, objective)
            return labels, ctx.leiden_clusters, rec, w, ns + ctx.leiden_counters()["total_ns"]
        labels = ctx.louvain(skx.n, rec, resolution)
        return labels, ctx.louvain_clusters, rec, w, ns + ctx.louvain_counters()["total_ns"]
    full_ns = [cluster(sk, [len(s) for s in sets])[4] for _ in range(a.repeat + 1)]
    labels, ncl, rec, w, _ = cluster(sk_model, msz)
    scale, lo, span, _ = host.leiden_quantiser(w, objective)
    _, tot, m2, _ = host.leiden_model_sums(rec, labels, ncl)
    query_ns, weight_s, place_ns = [], [], []
    for _ in range(a.repeat + 1):
        qe, near = ctx.graph_query(sk_all, len(model), a.threshold, kmer, a.knn)
        query_ns.append(ctx.graph_query_counters()["total_ns"])
        t0 = time.perf_counter()
        qrec = host.leiden_assign_weights(qe, msz, qsz, kmer, objective, scale, lo, span, threads=a.threads)
        weight_s.append(time.perf_counter() - t0)
        got = ctx.leiden_place(labels, ncl, len(queries), qrec, resolution, objective, tot=tot if objective else None, m2=m2 if objective else 0)
        place_ns.append(ctx.leiden_place_counters()["total_ns"])
    family_label = {}
    for i, g in enumerate(keep):
        family_label.setdefault(g // a.per_family, {}).setdefault(int(labels[i]), 0)
        family_label[g // a.per_family][int(labels[i])] += 1
    home = sum(1 for i, g in enumerate(hold) if g // a.per_family in family_label and
               int(got["label"][i]) == max(family_label[g // a.per_family].items(), key=lambda kv: kv[1])[0])
    return {"model_genomes": len(model), "queries": len(queries), "model_clusters": int(ncl), "algorithm": "leiden" if a.leiden else "louvain",
            "objective": "cpm" if objective == 0 else "modularity", "records": int(len(qe)), "placed": int((got["label"] >= 0).sum()),
            "in_family_community": home, "graph_query": ctx.graph_query_counters(), "leiden_place": ctx.leiden_place_counters(),
            "graph_query_ms": min(query_ns[1:]) / 1e6, "weights_ms": min(weight_s[1:]) * 1e3, "leiden_place_ms": min(place_ns[1:]) / 1e6,
            "full_run_ms": min(full_ns[1:]) / 1e6}


if __name__ == "__main__":
    main()
