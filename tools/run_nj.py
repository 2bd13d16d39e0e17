#!/usr/bin/env python
"""clust-mst --nj-tree on the device.

Default: a synthetic family set (families of 10 ... 3 000 sketches, each drawing from a pool of hashes of its own), the families
as the components, through Context.nj_clusters -- the best whole-call time of --repeat warm calls, the counter set and the three
phase times (fill, host distances, joining).

--crossover: the measurement behind the default RTC_NJ_GRID_MIN.  The same additive matrix -- a caterpillar tree
with integer branch lengths, so every value is exact -- through the workgroup path and through the grid path at every m of
--sizes; one JSON line per m with both joining times (the best of --repeat calls, upload excluded) and whether the records agree.

--support B: clust-mst --nj-support on the same set: Context.nj_support with B replicates, the best
whole-call time of --repeat warm calls with its four phase times (counting, host distances, joining, splits), and beside it B
times Context.nj_clusters' best whole-call time on the same set in the same session -- what B separate runs over filtered sets
could not beat.

    python tools/run_nj.py [--sizes 10,30,64,65,100,300,1000,3000] [--copies 1] [--sketch-size 1000] [--repeat 3] [--threads 16] [--support B [--seed S]]
    python tools/run_nj.py --crossover [--sizes 256,512,1024,2048,4096,8192] [--repeat 2] [--wg-max 8192]"""
import argparse
import json
import os
import sys

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


def caterpillar(m, seed):
    """leaf i hangs by a branch of a_i at x_i of a spine: D[i][j] = |x_i - x_j| + a_i + a_j, integers"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(1, 10, size=m)).astype(np.float64)[rng.permutation(m)]
    a = rng.integers(1, 10, size=m).astype(np.float64)
    D = np.abs(x[:, None] - x[None, :]) + a[:, None] + a[None, :]
    np.fill_diagonal(D, 0.0)
    return D


def timed_nj(ctx, D, grid_min, repeat):
    os.environ["RTC_NJ_GRID_MIN"] = str(grid_min)
    ctx.reload_options()
    best, rec = None, None
    for _ in range(repeat):
        rec = ctx.nj(D)
        c = ctx.nj_counters()
        if best is None or c["join_ns"] < best["join_ns"]:
            best = c
    return rec, best


def crossover(a):
    from rabbittclust_amd import api
    ctx = api.Context(0)
    timed_nj(ctx, caterpillar(128, 1), 4, 1)  # the units' first launches
    timed_nj(ctx, caterpillar(128, 1), (1 << 31) - 1, 1)
    for m in [int(v) for v in a.sizes.split(",")]:
        D = caterpillar(m, seed=m)
        row = {"m": m}
        rec_g, c = timed_nj(ctx, D, 4, a.repeat)
        assert c["paths"] == api.NJ_PATH_GRID
        row["grid_s"] = c["join_ns"] * 1e-9
        if m <= a.wg_max:
            rec_w, c = timed_nj(ctx, D, (1 << 31) - 1, a.repeat)
            assert c["paths"] == api.NJ_PATH_WORKGROUP
            row["workgroup_s"] = c["join_ns"] * 1e-9
            row["records_equal"] = bool(rec_w.tobytes() == rec_g.tobytes())
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--copies", type=int, default=1, help="families of every size")
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the distances")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--support", type=int, default=0, help="jackknife replicates (1 .. 256): time Context.nj_support as well")
    ap.add_argument("--seed", type=int, default=0, help="--support: the mask seed")
    ap.add_argument("--wg-max", type=int, default=8192, help="--crossover: the largest m the workgroup path is timed at")
    a = ap.parse_args()
    if a.crossover:
        a.sizes = a.sizes or "256,512,1024,2048,4096,8192"
        return crossover(a)
    from rabbittclust_amd import api
    sizes = [int(v) for v in (a.sizes or "10,30,64,65,100,300,1000,3000").split(",")] * a.copies
    sketches, comp = family_sketches(sizes, a.sketch_size, seed=7)
    ctx = api.Context(0)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, a.threads))
    sk = api.SketchSet.from_host(sketches, ctx.device, k=21, kind="minhash", width=8)
    best = None
    for r in range(a.repeat + 1):  # the first call warms up
        joins, first = ctx.nj_clusters(sk, comp, 21)
        c = ctx.nj_counters()
        if r and (best is None or c["total_ns"] < best["total_ns"]):
            best = c
    print(json.dumps({"sketches": sk.n, "sketch_size": a.sketch_size, "families": sorted(sizes), "records": len(joins), "counters": best,
                      "fill_s": best["fill_ns"] * 1e-9, "distance_s": best["distance_ns"] * 1e-9, "join_s": best["join_ns"] * 1e-9,
                      "total_s": best["total_ns"] * 1e-9}), flush=True)
    if a.support:
        sbest, main = None, None
        for r in range(a.repeat + 1):
            sjoins, _, support = ctx.nj_support(sk, comp, 21, a.support, seed=a.seed)
            c = ctx.nj_support_counters()
            if r and (sbest is None or c["total_ns"] < sbest["total_ns"]):
                sbest, main = c, ctx.nj_counters()
        assert sjoins.tobytes() == joins.tobytes()
        print(json.dumps({"replicates": a.support, "seed": a.seed, "counters": sbest, "main_counters": main,
                          "mean_count": sbest["count_sum"] / max(sbest["splits"], 1), "count_s": sbest["count_ns"] * 1e-9,
                          "distance_s": sbest["distance_ns"] * 1e-9, "join_s": sbest["join_ns"] * 1e-9, "split_s": sbest["split_ns"] * 1e-9,
                          "total_s": sbest["total_ns"] * 1e-9, "replicates_times_nj_clusters_s": a.support * best["total_ns"] * 1e-9}), flush=True)


if __name__ == "__main__":
    main()
