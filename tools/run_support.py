#!/usr/bin/env python
"""clust-mst --cluster-support on a synthetic family set: KSSD sketches of api.synth_family_descs genomes (families of --per
members, 2 Mbp each), the labels from rtc_mst's forest cut at --threshold.  Runs Context.cluster_support with --replicates
replicates (the best whole-call time of --repeat warm calls) and prints, one JSON line a set size, the counter set -- row chunks,
candidates, inner and crossing edges kept, hooking passes -- and the four phase times (the pair phase, the counts and masks, the
components, the tally) beside rtc_mst's call time on the same sketches.

    python tools/run_support.py [--sizes 5000,20000] [--per 10] [--threshold 0.05] [--replicates 64] [--seed 0] [--repeat 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tools.run_quality import cut_labels, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000")
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--replicates", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    from rabbittclust_amd import api
    ctx = api.Context(0)
    for n in [int(v) for v in a.sizes.split(",")]:
        sk = synth(ctx, api, n, a.per, seed=42)
        n = sk.n
        mst_s = None
        for r in range(a.repeat + 1):  # the first call warms up
            t0 = time.perf_counter()
            mst = ctx.mst(sk, a.threshold)
            dt = time.perf_counter() - t0
            if r and (mst_s is None or dt < mst_s):
                mst_s = dt
        labels = cut_labels(n, mst, a.threshold)
        best = None
        for r in range(a.repeat + 1):
            rec, together = ctx.cluster_support(sk, labels, sk.k, a.threshold, a.replicates, seed=a.seed)
            c = ctx.cluster_support_counters()
            if r and (best is None or c["total_ns"] < best["total_ns"]):
                best = c
        B = a.replicates
        print(json.dumps({"genomes": n, "kmer": sk.k, "threshold": a.threshold, "replicates": B, "seed": a.seed, "clusters": len(rec),
                          "mst_s": round(mst_s, 6), "counters": best, "pair_s": best["pair_ns"] * 1e-9, "count_s": best["count_ns"] * 1e-9,
                          "components_s": best["components_ns"] * 1e-9, "tally_s": best["tally_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9,
                          "recovered_mean": round(float(rec["recovered"].mean()), 3), "clusters_always_recovered": int((rec["recovered"] == B).sum()),
                          "clusters_ever_split": int((rec["split"] + rec["mixed"] > 0).sum()),
                          "clusters_ever_merged": int((rec["merged"] + rec["mixed"] > 0).sum()), "max_pieces": int(rec["max_pieces"].max())}), flush=True)
        del sk


if __name__ == "__main__":
    main()
