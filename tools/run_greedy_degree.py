#!/usr/bin/env python
"""clust-greedy --order degree on the device.

Default: a synthetic family set (--families families of --per sketches, each family drawing from a pool of hashes of its own, the
sketches ordered by size as the command line leaves them) through Context.greedy_degree and -- on the same sketches, calls
alternating -- Context.greedy (rtc_greedy, the walk in the given order): the best whole-call time of --repeat warm calls of each,
the cluster counts and greedy_degree's counter set with its phase times.  The two define different clusters; the times are of
interest side by side because the degree order has no serial dependency on the representative set.

--crossover: the measurement behind the default RTC_DEGREE_TAIL.  A path of --path genomes (a dependency chain of
n / 2 rounds, the worst case of the selection) and the family set, each at every tail value of --tails (0: never, the rounds
launched from the host): one JSON line per set and value with the selection time (the best of --repeat calls after a warm-up
call), the rounds run by the host and inside the one-workgroup kernel, and whether the result equals the first value's.

    python tools/run_greedy_degree.py [--families 200] [--per 50] [--sketch-size 400] [--threshold 0.05] [--repeat 3]
    python tools/run_greedy_degree.py --crossover [--tails 0,64,256,1024,2048,4096,16384,1000000] [--path 20000] [--repeat 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

K = 21


def family_sketches(families, per, sketch_size, seed):
    rng = np.random.default_rng(seed)
    sketches = []
    for _ in range(families):
        pool = np.unique(rng.integers(1, (1 << 31) - 1, size=3 * sketch_size, dtype=np.int64))[:2 * sketch_size]
        for _ in range(per):
            keep = rng.random(pool.size) < rng.uniform(0.45, 0.6)
            sketches.append(pool[keep][:sketch_size].astype(np.uint32))
    sketches.sort(key=lambda s: -len(s))
    return sketches


def path_sketches(n, block=8):
    return [np.arange(1000 + block * i, 1000 + block * (i + 2), dtype=np.uint32) for i in range(n)]


def best_degree(ctx, sk, threshold, repeat):
    best, out = None, None
    for r in range(repeat + 1):  # the first call warms up
        out = ctx.greedy_degree(sk, threshold, K)
        c = ctx.greedy_degree_counters()
        if r and (best is None or c["select_ns"] < best["select_ns"]):
            best = c
    return out, best


def crossover(a):
    from rabbittclust_amd import api
    ctx = api.Context(0)
    sets = {"path": path_sketches(a.path), "families": family_sketches(a.families, a.per, a.sketch_size, seed=7)}
    for name, host in sets.items():
        sk = api.SketchSet.from_host(host, ctx.device, k=K, kind="kssd", width=4)
        first = None
        for tail in [int(v) for v in a.tails.split(",")]:
            with ctx.env(RTC_DEGREE_TAIL=str(tail)):
                out, c = best_degree(ctx, sk, a.threshold, a.repeat)
            if first is None:
                first = out
            same = all(np.array_equal(x, y) for x, y in zip(out[:4], first[:4])) and out[4] == first[4]
            print(json.dumps({"set": name, "genomes": sk.n, "edges": c["kept_edges"], "tail": tail, "select_s": c["select_ns"] * 1e-9,
                              "host_rounds": c["rounds"] - c["tail_rounds"], "tail_rounds": c["tail_rounds"], "clusters": out[4],
                              "equal": bool(same)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=200)
    ap.add_argument("--per", type=int, default=50)
    ap.add_argument("--sketch-size", type=int, default=400)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--tails", default="0,64,256,1024,2048,4096,16384,1000000")
    ap.add_argument("--path", type=int, default=20000)
    a = ap.parse_args()
    if a.crossover:
        return crossover(a)
    from rabbittclust_amd import api
    ctx = api.Context(0)
    host = family_sketches(a.families, a.per, a.sketch_size, seed=7)
    sk = api.SketchSet.from_host(host, ctx.device, k=K, kind="kssd", width=4)
    best, plain_s, ncl_plain = None, None, 0
    for r in range(a.repeat + 1):  # the first round warms up; the two alternate
        out = ctx.greedy_degree(sk, a.threshold, K)
        c = ctx.greedy_degree_counters()
        t0 = time.perf_counter()
        ncl_plain, _ = ctx.greedy(sk, a.threshold)  # synchronous, like greedy_degree
        ms = (time.perf_counter() - t0) * 1e3
        if r and (best is None or c["total_ns"] < best["total_ns"]):
            best = c
        if r and (plain_s is None or ms * 1e-3 < plain_s):
            plain_s = ms * 1e-3
    print(json.dumps({"genomes": sk.n, "sketch_size": a.sketch_size, "threshold": a.threshold,
                      "degree": {"clusters": out[4], "pair_s": best["pair_ns"] * 1e-9, "predicate_s": best["predicate_ns"] * 1e-9,
                                 "select_s": best["select_ns"] * 1e-9, "assign_s": best["assign_ns"] * 1e-9, "total_s": best["total_ns"] * 1e-9,
                                 "paths": ctx.greedy_degree_last_path(), "counters": best},
                      "greedy": {"clusters": ncl_plain, "total_s": plain_s}}))


if __name__ == "__main__":
    main()
