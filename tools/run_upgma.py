#!/usr/bin/env python
"""clust-mst --upgma on the device.

Default: a synthetic family set (families of 10 ... 2 000 sketches, each drawing from a pool of hashes of its own), the families
as the components, through Context.upgma_clusters and -- on the same sketches and the same labelling, calls alternating --
Context.nj_clusters and Context.linkage_complete: the best whole-call time of --repeat warm calls of each, the counter sets and
the phase times.  All three consume the same key blocks; the yardstick for upgma's agglomeration time is nj's joining time.

--crossover: the measurement behind the default RTC_UPGMA_GRID_MIN.  The same matrix -- families of 8 at small q
with a little spread, Q1 across families, which is what the key blocks of real clusters look like: ties everywhere -- through the
workgroup path and through the grid path at every m of --sizes; one JSON line per m with both agglomeration times (the best of
--repeat calls after a warm-up call of that shape, upload excluded, the call ending in a stream synchronise) and whether the
records agree.

    python tools/run_upgma.py [--sizes 10,30,64,65,100,300,1000,2000] [--copies 1] [--sketch-size 1000] [--repeat 3] [--threads 16]
    python tools/run_upgma.py --crossover [--sizes 64,128,256,512,1024,2048] [--repeat 3] [--wg-max 4096]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

Q1 = 1 << 20


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


def family_matrix(m, seed, fam=8):
    """q in [4 000, 4 016) inside a family of `fam`, Q1 across"""
    rng = np.random.default_rng(seed)
    of = rng.permutation(m) // fam
    q = rng.integers(4000, 4016, size=(m, m)).astype(np.uint64)
    q = np.triu(q, 1)
    q = q + q.T
    S = np.where(of[:, None] == of[None, :], q, np.uint64(Q1)).astype(np.uint64)
    np.fill_diagonal(S, 0)
    return S


def timed_upgma(ctx, S, grid_min, repeat):
    os.environ["RTC_UPGMA_GRID_MIN"] = str(grid_min)
    ctx.reload_options()
    best, rec = None, None
    for r in range(repeat + 1):  # the first call of a shape warms up
        rec = ctx.upgma(S)
        c = ctx.upgma_counters()
        if r and (best is None or c["agglomerate_ns"] < best["agglomerate_ns"]):
            best = c
    return rec, best


def crossover(a):
    from rabbittclust_amd import api
    ctx = api.Context(0)
    never = (1 << 31) - 1
    for m in [int(v) for v in a.sizes.split(",")]:
        S = family_matrix(m, seed=m)
        row = {"m": m}
        rec_g, c = timed_upgma(ctx, S, 4, a.repeat)
        assert c["paths"] == api.UPGMA_PATH_GRID
        row["grid_s"] = c["agglomerate_ns"] * 1e-9
        if m <= a.wg_max:
            rec_w, c = timed_upgma(ctx, S, never, a.repeat)
            assert c["paths"] == (api.UPGMA_PATH_WORKGROUP if m > 64 else api.UPGMA_PATH_WAVE)
            row["workgroup_s" if m > 64 else "wave_s"] = c["agglomerate_ns"] * 1e-9
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
    ap.add_argument("--wg-max", type=int, default=4096, help="--crossover: the largest m the one-workgroup path is timed at")
    a = ap.parse_args()
    if a.crossover:
        a.sizes = a.sizes or "64,128,256,512,1024,2048"
        return crossover(a)
    from rabbittclust_amd import api
    sizes = [int(v) for v in (a.sizes or "10,30,64,65,100,300,1000,2000").split(",")] * a.copies
    sketches, comp = family_sketches(sizes, a.sketch_size, seed=7)
    ctx = api.Context(0)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, a.threads))
    sk = api.SketchSet.from_host(sketches, ctx.device, k=21, kind="minhash", width=8)
    best = {}
    n_rec = {}
    for r in range(a.repeat + 1):  # the first round warms up; the three alternate
        for name, call, counters in (("upgma", lambda: ctx.upgma_clusters(sk, comp, 21), ctx.upgma_counters),
                                     ("nj", lambda: ctx.nj_clusters(sk, comp, 21), ctx.nj_counters),
                                     ("complete", lambda: ctx.linkage_complete(sk, comp), ctx.linkage_counters)):
            rec, _ = call()
            c = counters()
            n_rec[name] = len(rec)
            if r and (name not in best or c["total_ns"] < best[name]["total_ns"]):
                best[name] = c
    u, j, l = best["upgma"], best["nj"], best["complete"]
    print(json.dumps({"sketches": sk.n, "sketch_size": a.sketch_size, "families": sorted(sizes), "records": n_rec,
                      "upgma": {"fill_s": u["fill_ns"] * 1e-9, "distance_s": u["distance_ns"] * 1e-9, "agglomerate_s": u["agglomerate_ns"] * 1e-9,
                                "total_s": u["total_ns"] * 1e-9, "counters": u},
                      "nj": {"fill_s": j["fill_ns"] * 1e-9, "distance_s": j["distance_ns"] * 1e-9, "join_s": j["join_ns"] * 1e-9,
                             "total_s": j["total_ns"] * 1e-9, "counters": j},
                      "complete": {"total_s": l["total_ns"] * 1e-9, "counters": l}}))


if __name__ == "__main__":
    main()
