#!/usr/bin/env python
"""The graph-based family on a synthetic family set: sketches the genomes (KSSD), builds the similarity graph
(Context.graph_build) and runs the deterministic Louvain (Context.louvain), then prints both counter sets.  With --leiden it
also runs the deterministic Leiden (Context.leiden) on the same graph -- the weights quantised as the command line does for
the objective -- and prints its counters and the whole-call time of rtc_leiden beside rtc_louvain's (the best of --repeat calls
each, after one call to warm up).

    python tools/run_leiden.py --families 40 --per-family 12 [--threshold 0.05] [--knn 1000] [--resolution 1.0]
    python tools/run_leiden.py --leiden [--objective cpm|modularity] [--leiden-resolution 0.5] [--repeat 3]"""
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
    a = ap.parse_args()
    from rabbittclust_amd import api, host
    ctx = api.Context(0)
    desc = api.synth_family_descs(a.families, a.per_family, global_seed=11)
    n = len(desc)
    off = np.arange(n + 1, dtype=np.uint64) * a.length
    seq = ctx.synth_genomes(desc, off)
    kmer = 21
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
