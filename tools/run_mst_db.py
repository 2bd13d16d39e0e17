"""clust-mst --db --query: rtc_rep_topk alone, split into the join, the bucketing (count, scan, scatter) and the selection, for
Q in {1e3, 1e4, 1e5} queries against R in {1e3, 1e4, 1e5} representatives at k in {1, 5, 64}, on KSSD u32 and MinHash u64
sketches.  Beside it: the dense Q x R intersection matrix and its read-back, what clust-greedy's repdb_query_topk does.

    python tools/run_mst_db.py [--reps 1000,10000,100000] [--queries 1000,10000,100000] [--k 1,5,64] [--repeat 3]

The sets are families of near-identical sketches (a quarter of the queries from new families).  Prints one JSON line per
case: the phase times from rtc_rep_topk_counters, candidates per query, bytes read back, and the dense path's time and bytes.
No number of this tool has been measured on an MI355X yet."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sets(rng, n_reps, n_q, width, size):
    hmax = (1 << 62) if width == 8 else (1 << 31) - 1
    n_fam = n_reps + n_q // 4
    dt = np.uint64 if width == 8 else np.uint32
    bases = rng.integers(1, hmax, size=(n_fam, size), dtype=np.int64)
    out = []
    for g in range(n_reps + n_q):
        f = g if g < n_reps else int(rng.integers(0, n_fam))
        s = bases[f].copy()
        flip = rng.random(size) < 0.02  # ~2 % of the hashes differ from the family's
        s[flip] = rng.integers(1, hmax, size=int(flip.sum()), dtype=np.int64)
        out.append(np.unique(s).astype(dt))
    return out


def _dense(ctx, s, R, Q, budget=256 << 20):
    """repdb_query_topk's read-back: the Q x R common matrix in row blocks of at most `budget` bytes"""
    import torch
    B = max(1, min(Q, budget // (4 * R)))
    t0 = time.perf_counter()
    nbytes = 0
    for q0 in range(0, Q, B):
        q1 = min(Q, q0 + B)
        m = ctx.pair_common(s, row0=R + q0, row1=R + q1, col0=0, col1=R)
        nbytes += m.numel() * 4
        m.cpu()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", default="1000,10000,100000")
    ap.add_argument("--queries", default="1000,10000,100000")
    ap.add_argument("--k", default="1,5,64")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true", help="leave out the dense read-back beside it")
    a = ap.parse_args()
    from rabbittclust_amd import api
    ctx = api.Context(0)
    for kind, width, size, mode in (("kssd", 4, 600, 0), ("minhash", 8, 1000, 2 | (1000 << 2))):
        for R in map(int, a.reps.split(",")):
            for Q in map(int, a.queries.split(",")):
                rng = np.random.default_rng(R + Q)
                s = api.SketchSet.from_host(_sets(rng, R, Q, width, size), ctx.device, k=21, kind=kind, width=width)
                dense_s, dense_b = _dense(ctx, s, R, Q) if not a.no_dense else (None, None)
                for k in map(int, a.k.split(",")):
                    ctx.rep_topk(s, R, mode, k)  # warm-up
                    best = None
                    for _ in range(a.repeat):
                        t0 = time.perf_counter()
                        hits, per = ctx.rep_topk(s, R, mode, k)
                        wall = time.perf_counter() - t0
                        c = ctx.rep_topk_counters()
                        if best is None or wall < best[0]:
                            best = (wall, c)
                    wall, c = best
                    print(json.dumps({"sketch": kind, "width": width, "reps": R, "queries": Q, "k": k,
                                      "wall_ms": round(1e3 * wall, 3), "join_ms": round(c["join_ns"] / 1e6, 3),
                                      "bucket_ms": round(c["bucket_ns"] / 1e6, 3), "select_ms": round(c["select_ns"] / 1e6, 3),
                                      "chunks": c["chunks"], "candidates_per_query": round(c["candidates"] / Q, 2),
                                      "bytes_read": c["bytes_read"], "kept": int(len(hits)),
                                      "dense_ms": None if dense_s is None else round(1e3 * dense_s, 3), "dense_bytes": dense_b}),
                          flush=True)
                del s
    ctx.close()


if __name__ == "__main__":
    main()
