"""Medoid timing of clust-mst --dedup-dist: rtc_tree_medoids on synthetic forests, host path (RTC_DEDUP_GPU=0, --threads host
threads) against the GPU path (RTC_DEDUP_GPU=2), one JSON line per (shape, group size).  The GPU cutoff of RTC_DEDUP_GPU=1
(kDedupGpuMinGroup, csrc/rtc_postprocess.hip) is the smallest group size from which the GPU is faster.

    python tools/run_dedup.py [--sizes 256,1024,4096,10000] [--shapes random,chain,star] [--threads 16] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rabbittclust_amd import api  # noqa: E402


def forest(size, shape, seed):
    """one dedup group of `size` members (a tree of the given shape, weights with exact ties) plus 64 singletons"""
    rng = np.random.default_rng(seed)
    n = size + 64
    ids = rng.permutation(n)[:size]
    e = np.zeros(size - 1, dtype=api.EDGE_DT)
    for i in range(1, size):
        p = i - 1 if shape == "chain" else 0 if shape == "star" else int(rng.integers(0, i))
        e[i - 1] = (ids[i], ids[p], float(rng.choice([0.0, 0.0005, 0.001, 0.0015])))
    return n, e, rng.integers(1000, 2000, size=n).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,10000")
    ap.add_argument("--shapes", default="random,chain,star")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    lines = []
    for shape in a.shapes.split(","):
        for size in [int(x) for x in a.sizes.split(",")]:
            n, e, lens = forest(size, shape, size)
            row = {"shape": shape, "group": size, "threads": a.threads}
            reps = {}
            for name, mode in (("host", 0), ("gpu", 2)):
                with ctx.env(RTC_DEDUP_GPU=mode):
                    ctx.tree_medoids(n, e, 0.01, lens, threads=a.threads)  # warm: code objects, allocations
                    best = float("inf")
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        reps[name] = ctx.tree_medoids(n, e, 0.01, lens, threads=a.threads)
                        best = min(best, time.perf_counter() - t0)
                    row[name + "_ms"] = round(best * 1e3, 3)
                    row[name + "_path"] = ctx.dedup_last_path()
            row["equal"] = bool(np.array_equal(reps["host"], reps["gpu"]))
            row["speedup"] = round(row["host_ms"] / row["gpu_ms"], 2)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()
    return 0 if all(json.loads(x)["equal"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
