#!/usr/bin/env python
"""The graph-based family on a synthetic family set: sketches the genomes (KSSD), builds the similarity graph
(Context.graph_build) and runs the deterministic Louvain (Context.louvain), then prints both counter sets.

    python tools/run_leiden.py --families 40 --per-family 12 [--threshold 0.05] [--knn 1000] [--resolution 1.0]"""
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
    labels, modularity = ctx.louvain(n, api.graph_weights(edges, sizes, kmer), a.resolution, return_modularity=True)
    print(json.dumps({"genomes": n, "edges": int(len(edges)), "clusters": ctx.louvain_clusters, "modularity": modularity,
                      "graph": graph, "louvain": ctx.louvain_counters()}))


if __name__ == "__main__":
    main()
