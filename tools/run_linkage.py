#!/usr/bin/env python
"""clust-mst --linkage complete on a synthetic family set: families of 10 ... 5 000 sketches (every family draws its sketches from
a pool of hashes of its own, so its pairs share from a little to most), the families as the components.  Runs
Context.linkage_complete (the best whole-call time of --repeat warm calls) and prints the counter set and both phase times.
With --host it also prints the time of a plain single-thread NumPy row-best restatement of the same components on the same key
blocks (quotients in double; its merge count is checked against the device's).

    python tools/run_linkage.py [--sizes 10,30,64,65,100,300,1000,3000,5000] [--copies 1] [--sketch-size 1000] [--repeat 3] [--host]
    RTC_LINKAGE_BYTES=2000000000 python tools/run_linkage.py     (several batches)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def family_sketches(sizes, sketch_size, seed):
    rng = np.random.default_rng(seed)
    sketches, comp = [], []
    for f, m in enumerate(sizes):
        pool = np.unique(rng.integers(1, 1 << 40, size=3 * sketch_size, dtype=np.uint64))[:2 * sketch_size]
        for _ in range(m):
            keep = rng.random(pool.size) < rng.uniform(0.3, 0.6)
            sketches.append(pool[keep][:sketch_size])
            comp.append(f)
    order = rng.permutation(len(sketches))  # scattered genome indices
    return [sketches[i] for i in order], np.asarray(comp)[order]


def host_rowbest(c, d):
    """row-best complete linkage over one block, kappa = c / d in double; returns the number of merges"""
    m = c.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        K = np.where(d > 0, c / np.maximum(d, 1), 0.0)
    np.fill_diagonal(K, 0.0)
    bp = np.argmax(K, axis=1)
    bk = K[np.arange(m), bp]
    alive = np.ones(m, dtype=bool)
    merges = 0
    for _ in range(m - 1):
        x = int(np.argmax(np.where(alive, bk, -1.0)))
        if bk[x] <= 0.0:
            break
        a, b = min(x, int(bp[x])), max(x, int(bp[x]))
        merges += 1
        row = np.minimum(K[a], K[b])
        row[a] = 0.0
        K[a, :] = row
        K[:, a] = row
        K[b, :] = 0.0
        K[:, b] = 0.0
        alive[b] = False
        again = np.flatnonzero(alive & ((bp == a) | (bp == b)))
        again = np.union1d(again, [a])
        bp[again] = np.argmax(K[again], axis=1)
        bk[again] = K[again, bp[again]]
    return merges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,30,64,65,100,300,1000,3000,5000")
    ap.add_argument("--copies", type=int, default=1, help="families of every size")
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    from rabbittclust_amd import api
    sizes = [int(v) for v in a.sizes.split(",")] * a.copies
    sketches, comp = family_sketches(sizes, a.sketch_size, seed=7)
    ctx = api.Context(0)
    sk = api.SketchSet.from_host(sketches, ctx.device, k=21, kind="minhash", width=8)
    best = None
    for r in range(a.repeat + 1):  # the first call warms up
        merges, first = ctx.linkage_complete(sk, comp)
        c = ctx.linkage_counters()
        if r and (best is None or c["total_ns"] < best["total_ns"]):
            best = c
    out = {"sketches": sk.n, "sketch_size": a.sketch_size, "families": sorted(sizes), "counters": best,
           "fill_s": best["fill_ns"] * 1e-9, "agglomerate_s": best["agglomerate_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9}
    if a.host:
        t_host, n_host = 0.0, 0
        for f in sorted(set(comp.tolist())):
            mem = np.flatnonzero(comp == f)
            sub = api.SketchSet.from_host([sketches[g] for g in mem], ctx.device, k=21, kind="minhash", width=8)
            cm = ctx.pair_common(sub, lower_only=False).cpu().numpy().astype(np.int64)
            ctx.sync()
            ln = np.array([len(sketches[g]) for g in mem], dtype=np.int64)
            d = ln[:, None] + ln[None, :] - cm
            t0 = time.perf_counter()
            n_host += host_rowbest(cm.astype(np.float64), d.astype(np.float64))
            t_host += time.perf_counter() - t0
        out["host_rowbest_s"] = t_host
        out["host_merges"] = n_host
        assert n_host == len(merges), (n_host, len(merges))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
