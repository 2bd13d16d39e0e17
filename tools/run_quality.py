#!/usr/bin/env python
"""clust-mst --quality on a synthetic family set: KSSD sketches of api.synth_family_descs genomes (families of --per members,
2 Mbp each), the labels from rtc_mst's forest cut at --threshold.  Runs Context.cluster_quality (the best whole-call time of
--repeat warm calls) with and without RTC_SIL_GLOBAL=1 and prints, one JSON line a set size, the counter set and the three phase
times -- the pair phase, the host's distances, the score -- beside rtc_mst's call time on the same sketches.

    python tools/run_quality.py [--sizes 5000,20000] [--per 10] [--threshold 0.05] [--threads 16] [--repeat 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def synth(ctx, api, n, per, seed, L=2_000_000, batch=5_000):
    """KSSD sketches of n synthetic genomes, batch by batch, joined into one set"""
    import torch
    from rabbittclust_amd import host
    desc = api.synth_family_descs(n // per, per, global_seed=seed)
    sd = host.generate_shuffle_dim(6)
    parts = []
    for b0 in range(0, n, batch):
        d = desc[b0:b0 + batch]
        off = np.arange(len(d) + 1, dtype=np.uint64) * np.uint64(L)
        seq = ctx.synth_genomes(d, off)
        parts.append(ctx.sketch_kssd(seq, off, sd, kmer_size=21, drlevel=3))
        ctx.sync()
        del seq
        torch.cuda.empty_cache()
    base, hs, st = 0, [], []
    for p in parts:
        hs.append(p.hashes)
        st.append(p.start + base)
        base += p.hashes.numel()
    return api.SketchSet(torch.cat(hs), torch.cat(st), torch.cat([p.len for p in parts]), 4, parts[0].k, "kssd")


def cut_labels(n, mst, threshold):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in mst[mst["dist"] <= threshold]:
        a, b = find(int(e["preNode"])), find(int(e["sufNode"]))
        parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000")
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the distance pass")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    from rabbittclust_amd import api
    ctx = api.Context(0)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, a.threads))
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
        out = {"genomes": n, "kmer": sk.k, "threshold": a.threshold, "host_threads": a.threads, "clusters": int(len(np.unique(labels))),
               "mst_s": round(mst_s, 6)}
        ref = None
        for name, flag in (("default", None), ("global", "1")):
            with ctx.env(RTC_SIL_GLOBAL=flag):
                best = None
                for r in range(a.repeat + 1):
                    rec = ctx.cluster_quality(sk, labels, sk.k)
                    c = ctx.cluster_quality_counters()
                    if r and (best is None or c["total_ns"] < best["total_ns"]):
                        best = c
            if ref is None:
                ref = rec
                out["silhouette_mean"] = round(float(api.silhouette_value(rec).mean()), 6)
            assert rec.tobytes() == ref.tobytes(), "RTC_SIL_GLOBAL=1 changed the records"
            out[name] = {"counters": best, "pair_s": best["pair_ns"] * 1e-9, "distance_s": best["distance_ns"] * 1e-9,
                         "score_s": best["score_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9}
        print(json.dumps(out), flush=True)
        del sk


if __name__ == "__main__":
    main()
