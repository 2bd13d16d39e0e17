#!/usr/bin/env python
"""clust-mst --pangenome on synthetic family sets: KSSD sketches of api.synth_family_descs genomes (2 Mbp each), the labels the
families themselves.  Three shapes over --genomes genomes: many small families (--small members each), families of --per, and
one cluster of everything (the sketches of the second shape under one label).  Runs Context.pangenome (the best whole-call time
of --repeat warm calls), by default and with every cluster in the arena (RTC_PAN_GLOBAL=1), and prints, one JSON line a shape and
mode, the counters -- clusters, records, distinct hashes, clusters by path, groups -- and the times of the three steps beside
rtc_mst's call time on the same sketches.  Then four sets of made-up sketches with a core (the synthetic genomes' families share
too little to have one): --core hashes per family or for everybody and --own per genome, as families and as one cluster.

    python tools/run_pangenome.py [--genomes 10000] [--small 4] [--per 50] [--threshold 0.05] [--repeat 3] [--core 400] [--own 80] [--made-only]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tools.run_quality import synth  # noqa: E402


def measure(ctx, sk, labels, repeat, all_global):
    best = None
    with ctx.env(RTC_PAN_GLOBAL="1" if all_global else None):
        for r in range(repeat + 1):  # the first call warms up
            clusters, hist, genomes = ctx.pangenome(sk, labels)
            c = ctx.pangenome_counters()
            if r and (best is None or c["total_ns"] < best["total_ns"]):
                best = c
    return clusters, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=10000)
    ap.add_argument("--small", type=int, default=4)
    ap.add_argument("--per", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--core", type=int, default=400, help="the made-up sketches' hashes that a family (or everybody) shares")
    ap.add_argument("--own", type=int, default=80, help="the made-up sketches' hashes of their own")
    ap.add_argument("--made-only", action="store_true", help="skip the synthetic genomes: the made-up sketches only")
    a = ap.parse_args()
    from rabbittclust_amd import api
    ctx = api.Context(0)
    for shape, per, one in (("small families", a.small, False), ("families", a.per, False), ("one cluster", a.per, True)):
        if a.made_only:
            break
        sk = synth(ctx, api, a.genomes // per * per, per, seed=42)
        n = sk.n
        mst_s = None
        for r in range(a.repeat + 1):
            t0 = time.perf_counter()
            ctx.mst(sk, a.threshold)
            dt = time.perf_counter() - t0
            if r and (mst_s is None or dt < mst_s):
                mst_s = dt
        labels = np.zeros(n, dtype=np.int32) if one else (np.arange(n) // per * per).astype(np.int32)
        for all_global in (False, True):
            clusters, best = measure(ctx, sk, labels, a.repeat, all_global)
            pan = clusters["pan"].astype(np.float64)
            share = float((clusters["core"][pan > 0] / pan[pan > 0]).mean())
            print(json.dumps({"shape": shape, "genomes": n, "members": n if one else per, "all_global": all_global, "mst_s": round(mst_s, 6),
                              "counters": best, "count_s": best["count_ns"] * 1e-9, "sweep_s": best["sweep_ns"] * 1e-9,
                              "genome_s": best["genome_ns"] * 1e-9, "kernel_s": best["kernel_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9,
                              "records_per_kernel_s": best["records"] / max(best["kernel_ns"] * 1e-9, 1e-12), "core_share_mean": round(share, 4)}),
                  flush=True)
        del sk
    # what the genomes above do not have: a core.  Every member of a family holds the family's --core hashes and --own of its
    # own; under one label the 200 cores become shell.  "shared core": all genomes hold the same --core hashes -- the
    # most contended addresses the count can meet.
    rng = np.random.default_rng(7)
    n = a.genomes // a.per * a.per

    def made(shared):
        out = []
        core = None
        for g in range(n):
            if g % a.per == 0 and (core is None or not shared):
                core = rng.integers(0, 1 << 32, size=a.core, dtype=np.uint64)
            out.append(np.unique(np.concatenate([core, rng.integers(0, 1 << 32, size=a.own, dtype=np.uint64)])).astype(np.uint32))
        return api.SketchSet.from_host(out, ctx.device, k=21, kind="kssd", width=4)
    for shape, shared, one in (("family cores", False, False), ("family cores, one cluster", False, True), ("shared core, families", True, False),
                               ("shared core, one cluster", True, True)):
        sk = made(shared)
        labels = np.zeros(n, dtype=np.int32) if one else (np.arange(n) // a.per * a.per).astype(np.int32)
        clusters, best = measure(ctx, sk, labels, a.repeat, False)
        print(json.dumps({"shape": shape, "genomes": n, "members": n if one else a.per, "core": a.core, "own": a.own, "counters": best,
                          "count_s": best["count_ns"] * 1e-9, "sweep_s": best["sweep_ns"] * 1e-9, "genome_s": best["genome_ns"] * 1e-9,
                          "kernel_s": best["kernel_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9,
                          "records_per_kernel_s": best["records"] / max(best["kernel_ns"] * 1e-9, 1e-12),
                          "core_hashes": int(clusters["core"].sum())}), flush=True)
        del sk


if __name__ == "__main__":
    main()
