"""clust-mst --db --screen: rtc_rep_screen alone on a synthetic set, beside rtc_rep_topk(topk = 0, wmode 0), the nearest existing
call over the same candidates.

    python tools/run_screen.py [--reps 20000] [--size 300] [--family 20] [--samples 8] [--mix 200] [--noise 5000] [--repeat 3]

The set: --reps representatives of --size hashes (u32, KSSD-like) in families of --family whose members differ from the family's
hashes in about 5 % of them; --samples samples, each the union of --mix representatives drawn at random and --noise hashes no
representative has.  Prints one JSON line: rtc_rep_screen_counters and the wall time of the best of --repeat calls with the
command line's defaults (min_common 2, containment 0.05, min_unique 2, no pick limit), the same with RTC_SCREEN_GLOBAL=1, and the
wall time and phase times of rtc_rep_topk on the same set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _set(rng, n_reps, size, family, n_samples, mix, noise):
    hmax = (1 << 31) - 1
    n_fam = (n_reps + family - 1) // family
    bases = rng.integers(1, hmax // 2, size=(n_fam, size), dtype=np.int64)
    reps = []
    for g in range(n_reps):
        s = bases[g // family].copy()
        flip = rng.random(size) < 0.05
        s[flip] = rng.integers(1, hmax // 2, size=int(flip.sum()), dtype=np.int64)
        reps.append(np.unique(s).astype(np.uint32))
    samples = []
    for _ in range(n_samples):
        parts = [reps[int(r)] for r in rng.choice(n_reps, size=min(mix, n_reps), replace=False)]
        parts.append(rng.integers(hmax // 2 + 1, hmax, size=noise, dtype=np.int64).astype(np.uint32))  # above every representative's
        samples.append(np.unique(np.concatenate(parts)))
    return reps, samples


def _best(fn, repeat):
    fn()  # warm-up
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, out)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20000)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--family", type=int, default=20)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--mix", type=int, default=200)
    ap.add_argument("--noise", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    from rabbittclust_amd import api
    ctx = api.Context(0)
    rng = np.random.default_rng(a.reps + a.samples)
    reps, samples = _set(rng, a.reps, a.size, a.family, a.samples, a.mix, a.noise)
    s = api.SketchSet.from_host(reps + samples, ctx.device, k=21, kind="kssd", width=4)
    R = len(reps)
    cont = int(round(0.05 * api.SCREEN_Q20))

    def screen():
        hits, sums = ctx.rep_screen(s, R, 2, cont, 2, 0)
        return hits, sums, ctx.rep_screen_counters(), ctx.rep_screen_last_path()

    def topk():
        hits, per = ctx.rep_topk(s, R, 0, 0)
        return hits, ctx.rep_topk_counters()

    wall, (hits, sums, c, path) = _best(screen, a.repeat)
    with ctx.env(RTC_SCREEN_GLOBAL="1"):
        wall_g, (hits_g, sums_g, c_g, _) = _best(screen, a.repeat)
    assert hits.tobytes() == hits_g.tobytes() and sums.tobytes() == sums_g.tobytes()
    wall_t, (hits_t, c_t) = _best(topk, a.repeat)
    ms = lambda ns: round(ns / 1e6, 3)  # noqa: E731
    print(json.dumps({
        "reps": R, "rep_hashes": int(sum(len(r) for r in reps)), "samples": len(samples), "sample_hashes": [int(len(x)) for x in samples],
        "screen": {"wall_ms": round(1e3 * wall, 3), "expand_ms": ms(c["expand_ns"]), "gather_ms": ms(c["gather_ns"]), "call_ms": ms(c["call_ns"]),
                   "chunks": c["chunks"], "matches": c["matches"], "candidates": c["candidates"], "eligible": c["eligible"], "picks": c["picks"],
                   "rounds_max": c["rounds_max"], "paths": [c["wave_queries"], c["workgroup_queries"], c["global_queries"]], "last_path": path,
                   "explained": [int(x) for x in sums["n_explained"]], "matched": [int(x) for x in sums["n_matched"]]},
        "screen_global": {"wall_ms": round(1e3 * wall_g, 3), "expand_ms": ms(c_g["expand_ns"]), "gather_ms": ms(c_g["gather_ns"])},
        "rep_topk_all": {"wall_ms": round(1e3 * wall_t, 3), "join_ms": ms(c_t["join_ns"]), "bucket_ms": ms(c_t["bucket_ns"]),
                         "select_ms": ms(c_t["select_ns"]), "candidates": c_t["candidates"], "kept": int(len(hits_t))}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
