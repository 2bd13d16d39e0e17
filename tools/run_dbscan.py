"""clust-dbscan --fast on one GPU: Context.dbscan timed warm next to Context.mst on the same resident sketches, with the split
of the DBSCAN call into the pair phase, the eps filter and the components from rtc_dbscan_counters.

    python tools/run_dbscan.py [--sets dense25k,cfg4_200k] [--eps 0.05] [--minpts 5] [--repeat 3] [--sweep e1,e2,...] [--kdist]
                               [--hierarchy] [--knn K] [--assign Q] [--update M]

--knn K times Context.dbscan_knn (clust-dbscan --knn K) beside Context.dbscan on the same set: the best of --repeat warm calls with
the counters of rtc_dbscan_knn_counters -- passers, rows truncated, rows that needed arrival keys, neighbour edges, propagation
rounds -- and the selection's and the propagation's share of the call.

--sweep times one Context.dbscan_sweep over the listed eps values (best of --repeat warm calls) against the same values run as
separate Context.dbscan calls (the sum of each value's best warm call), with the sweep's phases from rtc_dbscan_sweep_counters;
--kdist adds the k-distance curve to the sweep.  --hierarchy (with --sweep) times Context.dbscan_hierarchy at the largest listed
eps, its calls alternating with the sweep's, with its phases from rtc_dbscan_hierarchy_counters.  --separate-only times the separate calls alone (a library without the sweep).

Sets (KSSD u32 sketches from synthetic genomes, k 21, drlevel 3, sketched on the GPU as bench.py does):
  dense25k   25 000 x 2 Mbp genomes in 25 families of 1 000 (substitution rate <= 0.01): bench.py's dense u32_25000 set, the
             dense regime (~12.5 M pairs within the families);
  cfg4_200k  200 000 x 2 Mbp genomes in families of ten: BASELINE config[4]'s shape on one GPU, sketched in batches of 25 000;
  sparse25k / sparse200k  host-drawn random u32 sets of ~1 100 / ~330 hashes in families of ten (~2 % of a member's hashes
             replaced): a sparse eps graph.
--minhash times Context.dbscan_mash (clust-dbscan --minhash) instead, on 10 000 MinHash sketches of s = 1000 in 10 families of
1 000 (bench.py's extra.dense_pairs shape), --eps and --sweep as its levels: one JSON line with the counters of the best of
--repeat warm calls for each of the four configurations -- the wave-cooperative merge and RTC_DBSCAN_MASH_SERIAL=1, each with
the prefilter and with RTC_DBSCAN_MASH_NOPREFILTER=1 -- and whether the four label sets are identical.

--assign Q times Context.dbscan_assign (clust-dbscan --db --assign): the last Q sketches of a set are the queries, the rest the
model, clustered once at --eps / --minpts; best of --repeat warm calls with the phases of rtc_dbscan_assign_counters, beside the
baseline it replaces, Context.dbscan (with --minhash: dbscan_mash) on all n sketches.  --baseline-lib PATH takes that baseline
from another build of the library, e.g. the parent commit's librtclust_hip.so, in a child process (RTC_HIP_LIB); without it the
baseline is this build's.

--update M times Context.dbscan_update (clust-dbscan --db --update): the last M sketches of a set are the new genomes, the rest
the model, clustered once at --eps / --minpts; best of --repeat warm calls with the counters of rtc_dbscan_update_counters -- the
rows of both stages, promoted points, clusters merged away, the join, predicate and components times -- beside Context.dbscan on
all n sketches, and whether the two label vectors are identical.  Its default set is fam20k: 20 000 host-drawn u32 sets of ~600
hashes in families of ten at three substitution rates (2 %, 10 %, 30 % of a member's hashes replaced) and loners, in shuffled
order, so the new genomes come from every family.

Prints one JSON line per set.  The kernel split under rocprofv3 --kernel-trace --stats comes from a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPARSE = {"sparse25k": (25_000, 1100, 10), "sparse200k": (200_000, 330, 10)}
SYNTH = {"dense25k": (25_000, 1000, 0.01, 44), "cfg4_200k": (200_000, 10, None, 42)}  # n, family size, max_rate, seed


def _sparse(rng, n, size, per):
    n_fam = (n + per - 1) // per
    bases = rng.integers(1, (1 << 31) - 1, size=(n_fam, size), dtype=np.int64)
    out = []
    for g in range(n):
        s = bases[g // per].copy()
        flip = rng.random(size) < 0.02
        s[flip] = rng.integers(1, (1 << 31) - 1, size=int(flip.sum()), dtype=np.int64)
        out.append(np.unique(s).astype(np.uint32))
    return out


def _mixed_families(rng, n, size=600, per=10):
    """families of `per` at three substitution rates, every tenth family a lone sketch, shuffled"""
    out, f = [], 0
    while len(out) < n:
        base = rng.integers(1, (1 << 31) - 1, size=size, dtype=np.int64)
        members = 1 if f % 10 == 9 else per
        rate = (0.02, 0.1, 0.3)[f % 3]
        for _ in range(min(members, n - len(out))):
            s = base.copy()
            flip = rng.random(size) < rate
            s[flip] = rng.integers(1, (1 << 31) - 1, size=int(flip.sum()), dtype=np.int64)
            out.append(np.unique(s).astype(np.uint32))
        f += 1
    return [out[i] for i in rng.permutation(n)]


def _synth(ctx, api, n, per, max_rate, seed, L=2_000_000, batch=25_000):
    """KSSD sketches of n synthetic genomes, batch by batch (a batch of 25 000 x 2 Mbp is 50 GB of bases), joined into one set"""
    import torch
    from rabbittclust_amd import host
    kw = {} if max_rate is None else {"max_rate": max_rate}
    desc = api.synth_family_descs(n // per, per, global_seed=seed, **kw)
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


def _sweep_row(ctx, sk, name, n, kmer, eps_list, a):
    """one sweep against the same eps values as separate calls, each warm, best of a.repeat"""
    sep_ms, sep_labels = [], []
    for eps in eps_list:
        ctx.dbscan(sk, eps, a.minpts, kmer)
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            lab = ctx.dbscan(sk, eps, a.minpts, kmer)
            ts.append(time.perf_counter() - t0)
        sep_ms.append(min(ts) * 1e3)
        sep_labels.append(lab)
    row = {"set": name, "n": n, "kmer": kmer, "minpts": a.minpts, "eps": eps_list, "separate_ms": [round(x, 3) for x in sep_ms],
           "separate_sum_ms": round(sum(sep_ms), 3)}
    if a.separate_only:
        return row
    ctx.dbscan_sweep(sk, eps_list, a.minpts, kmer, kdist=a.kdist)
    if a.hierarchy:
        ctx.dbscan_hierarchy(sk, max(eps_list), a.minpts, kmer)
    ts, cs, hts, hcs = [], [], [], []
    for _ in range(a.repeat):  # the two calls alternate, so drift of the machine falls on both
        t0 = time.perf_counter()
        out = ctx.dbscan_sweep(sk, eps_list, a.minpts, kmer, kdist=a.kdist)
        ts.append(time.perf_counter() - t0)
        cs.append(ctx.dbscan_sweep_counters())
        if a.hierarchy:
            t0 = time.perf_counter()
            forest, _ = ctx.dbscan_hierarchy(sk, max(eps_list), a.minpts, kmer)
            hts.append(time.perf_counter() - t0)
            hcs.append(ctx.dbscan_hierarchy_counters())
    labels = out[0] if a.kdist else out
    c = cs[int(np.argmin(ts))]
    row.update({"sweep_ms": round(min(ts) * 1e3, 3), "sweep_all_ms": [round(x * 1e3, 3) for x in ts], "kdist": bool(a.kdist),
                "identical": all(np.array_equal(labels[e], sep_labels[e]) for e in range(len(eps_list))),
                "pair_ms": round(c["pair_ns"] / 1e6, 3), "predicate_ms": round(c["predicate_ns"] / 1e6, 3),
                "components_ms": round(c["components_ns"] / 1e6, 3), "kdist_ms": round(c["kdist_ns"] / 1e6, 3),
                "library_ms": round(c["total_ns"] / 1e6, 3), "chunks": c["chunks"], "candidate_edges": c["candidate_edges"],
                "kept_edges": c["kept_edges"], "hook_rounds": c["hook_rounds"],
                "clusters": [int(x.max(initial=-1)) + 1 for x in labels]})
    if a.hierarchy:
        h = hcs[int(np.argmin(hts))]
        row["hierarchy"] = {"eps_max": max(eps_list), "ms": round(min(hts) * 1e3, 3), "all_ms": [round(x * 1e3, 3) for x in hts],
                            "pair_ms": round(h["pair_ns"] / 1e6, 3), "kdist_ms": round(h["kdist_ns"] / 1e6, 3),
                            "rank_ms": round(h["rank_ns"] / 1e6, 3), "forest_ms": round(h["forest_ns"] / 1e6, 3),
                            "library_ms": round(h["total_ns"] / 1e6, 3), "kept_edges": h["kept_edges"], "forest_edges": len(forest),
                            "boruvka_rounds": h["boruvka_rounds"]}
    return row


def _minhash_rows(ctx, api, a, n=10_000, fam=10, rate=0.01, L=500_000, s=1000, k=21):
    desc = api.synth_family_descs(fam, n // fam, global_seed=42, max_rate=rate)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    seq = ctx.synth_genomes(desc, off)
    sk = ctx.sketch_minhash(seq, off, k=k, size=s)
    ctx.sync()
    del seq
    eps_list = [float(x) for x in a.sweep.split(",")] if a.sweep else [a.eps]
    row = {"set": "minhash10k", "n": n, "sketch_size": s, "kmer": k, "minpts": a.minpts, "eps": eps_list, "configs": {}}
    labels = []
    for name, env in (("cooperative", {}), ("cooperative_noprefilter", {"RTC_DBSCAN_MASH_NOPREFILTER": "1"}),
                      ("serial", {"RTC_DBSCAN_MASH_SERIAL": "1"}),
                      ("serial_noprefilter", {"RTC_DBSCAN_MASH_SERIAL": "1", "RTC_DBSCAN_MASH_NOPREFILTER": "1"})):
        with ctx.env(RTC_DBSCAN_MASH_SERIAL=env.get("RTC_DBSCAN_MASH_SERIAL"), RTC_DBSCAN_MASH_NOPREFILTER=env.get("RTC_DBSCAN_MASH_NOPREFILTER")):
            ctx.dbscan_mash(sk, s, eps_list, a.minpts, k)  # warm-up
            ts, cs = [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                lab = ctx.dbscan_mash(sk, s, eps_list, a.minpts, k)
                ts.append(time.perf_counter() - t0)
                cs.append(ctx.dbscan_mash_counters())
        c = cs[int(np.argmin([x["predicate_ns"] for x in cs]))]
        labels.append(lab)
        row["configs"][name] = {"call_ms": round(min(ts) * 1e3, 3), "pair_ms": round(c["pair_ns"] / 1e6, 3),
                                "predicate_ms": round(c["predicate_ns"] / 1e6, 3), "components_ms": round(c["components_ns"] / 1e6, 3),
                                "chunks": c["chunks"], "candidate_edges": c["candidate_edges"], "merged": c["merged"],
                                "kept_edges": c["kept_edges"], "hook_rounds": c["hook_rounds"]}
    row["identical"] = all(np.array_equal(labels[0], x) for x in labels[1:])
    row["clusters"] = [int(x.max(initial=-1)) + 1 for x in labels[0]]
    row["noise"] = [int((x < 0).sum()) for x in labels[0]]
    return row


def _head(api, sk, n_db):
    """the first n_db sketches of a set, over the same hash buffer"""
    return api.SketchSet(sk.hashes, sk.start[:n_db].contiguous(), sk.len[:n_db].contiguous(), sk.width, sk.k, sk.kind)


def _best(fn, repeat):
    fn()  # warm-up: code objects, scratch
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, out


def _assign_row(ctx, api, sk, name, kmer, a, sketch_size=None):
    n, q = sk.n, a.assign

    def cluster(s):
        if sketch_size:
            lab, core = ctx.dbscan_mash(s, sketch_size, [a.eps], a.minpts, kmer, return_core=True)
            return lab[0], core[0]
        return ctx.dbscan(s, a.eps, a.minpts, kmer, return_core=True)
    base_ms, _ = _best(lambda: cluster(sk), a.repeat)
    row = {"set": name, "n": n, "queries": q, "kmer": kmer, "eps": a.eps, "minpts": a.minpts, "recluster_all_ms": round(base_ms, 3)}
    if a.baseline_only:
        return row
    labels, core = cluster(_head(api, sk, n - q))
    cs = []

    def call():
        out = ctx.dbscan_assign(sk, n - q, labels, core, a.eps, a.minpts, kmer, sketch_size=sketch_size)
        cs.append(ctx.dbscan_assign_counters())
        return out
    ms, _ = _best(call, a.repeat)
    c = min(cs[1:], key=lambda x: x["total_ns"])
    row.update({"assign_ms": round(ms, 3), "library_ms": round(c["total_ns"] / 1e6, 3), "join_ms": round(c["join_ns"] / 1e6, 3),
                "predicate_ms": round(c["predicate_ns"] / 1e6, 3), "fold_ms": round(c["fold_ns"] / 1e6, 3), "chunks": c["chunks"],
                "candidates": c["candidates"], "neighbours": c["neighbours"], "placed": c["placed"], "novel": c["novel"],
                "bridging": c["bridging"], "fold_paths": c["fold_paths"]})
    if a.baseline_lib:  # the same set in a child that loads the other build
        import subprocess
        args = [sys.executable, os.path.abspath(__file__), "--sets", name, "--assign", str(q), "--eps", str(a.eps), "--minpts", str(a.minpts),
                "--repeat", str(a.repeat), "--baseline-only"] + (["--minhash"] if sketch_size else [])
        r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, RTC_HIP_LIB=a.baseline_lib))
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        row["baseline_lib"] = a.baseline_lib
        row["baseline_lib_recluster_all_ms"] = json.loads(lines[-1])["recluster_all_ms"] if r.returncode == 0 and lines else None
    return row


def _update_row(ctx, api, sk, name, kmer, a):
    n, m = sk.n, a.update
    full_ms, (want, want_core) = _best(lambda: ctx.dbscan(sk, a.eps, a.minpts, kmer, return_core=True), a.repeat)
    fc = ctx.dbscan_counters()
    labels, core = ctx.dbscan(_head(api, sk, n - m), a.eps, a.minpts, kmer, return_core=True)
    cs = []

    def call():
        out = ctx.dbscan_update(sk, n - m, labels, core, a.eps, a.minpts, kmer)
        cs.append(ctx.dbscan_update_counters())
        return out
    ms, (got, got_core) = _best(call, a.repeat)
    c = min(cs[1:], key=lambda x: x["total_ns"])
    return {"set": name, "n": n, "new": m, "kmer": kmer, "eps": a.eps, "minpts": a.minpts, "dbscan_all_ms": round(full_ms, 3),
            "dbscan_all_pair_ms": round(fc["pair_ns"] / 1e6, 3), "dbscan_all_filter_ms": round(fc["filter_ns"] / 1e6, 3),
            "dbscan_all_components_ms": round(fc["components_ns"] / 1e6, 3), "dbscan_all_candidate_edges": fc["candidate_edges"],
            "update_ms": round(ms, 3), "library_ms": round(c["total_ns"] / 1e6, 3), "join_ms": round(c["join_ns"] / 1e6, 3),
            "predicate_ms": round(c["predicate_ns"] / 1e6, 3), "components_ms": round(c["components_ns"] / 1e6, 3),
            "stage1_rows": c["stage1_rows"], "stage2_rows": c["stage2_rows"], "chunks": c["chunks"], "candidate_edges": c["candidate_edges"],
            "kept_edges": c["kept_edges"], "promoted": c["promoted"], "merged": c["merged"], "hook_rounds": c["hook_rounds"],
            "identical": bool(np.array_equal(got, want) and np.array_equal(got_core, want_core)),
            "clusters": int(want.max(initial=-1)) + 1, "noise": int((want < 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="dense25k,cfg4_200k")
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--minpts", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-mst", action="store_true")
    ap.add_argument("--sweep", default="")
    ap.add_argument("--kdist", action="store_true")
    ap.add_argument("--separate-only", action="store_true")
    ap.add_argument("--hierarchy", action="store_true")
    ap.add_argument("--minhash", action="store_true")
    ap.add_argument("--assign", type=int, default=0)
    ap.add_argument("--knn", type=int, default=0)
    ap.add_argument("--update", type=int, default=0)
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    import torch
    from rabbittclust_amd import api
    ctx = api.Context(0)
    if a.minhash and a.assign:
        n, fam, L, s, k = 10_000, 10, 500_000, 1000, 21
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        order = np.random.default_rng(1).permutation(n)  # the queries come from every family
        seq = ctx.synth_genomes(api.synth_family_descs(fam, n // fam, global_seed=42, max_rate=0.01)[order], off)
        sk = ctx.sketch_minhash(seq, off, k=k, size=s)
        ctx.sync()
        del seq
        print(json.dumps(_assign_row(ctx, api, sk, "minhash10k", k, a, sketch_size=s)), flush=True)
        ctx.close()
        return
    if a.minhash:
        print(json.dumps(_minhash_rows(ctx, api, a)), flush=True)
        ctx.close()
        return
    if a.update and a.sets == ap.get_default("sets"):
        a.sets = "fam20k"
    for name in a.sets.split(","):
        if name == "fam20k":
            n = 20_000
            sk = api.SketchSet.from_host(_mixed_families(np.random.default_rng(11), n), ctx.device, k=22, kind="kssd", width=4)
        elif name in SPARSE:
            n, size, per = SPARSE[name]
            sk = api.SketchSet.from_host(_sparse(np.random.default_rng(7), n, size, per), ctx.device, k=22, kind="kssd", width=4)
        else:
            n, per, rate, seed = SYNTH[name]
            sk = _synth(ctx, api, n, per, rate, seed)
        kmer = sk.k  # half_k * 2, as clust-dbscan --presketched takes it
        torch.cuda.synchronize()
        if a.assign:
            print(json.dumps(_assign_row(ctx, api, sk, name, kmer, a)), flush=True)
            del sk
            continue
        if a.update:
            print(json.dumps(_update_row(ctx, api, sk, name, kmer, a)), flush=True)
            del sk
            continue
        if a.sweep:
            print(json.dumps(_sweep_row(ctx, sk, name, n, kmer, [float(x) for x in a.sweep.split(",")], a)), flush=True)
            del sk
            continue
        ctx.dbscan(sk, a.eps, a.minpts, kmer)  # warm-up: code objects, scratch
        ts, cs = [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            lab = ctx.dbscan(sk, a.eps, a.minpts, kmer)
            ts.append(time.perf_counter() - t0)
            cs.append(ctx.dbscan_counters())
        best = int(np.argmin(ts))
        c = cs[best]
        row = {"set": name, "n": n, "mean_hashes": round(float(sk.len.float().mean().item()), 1), "kmer": kmer, "eps": a.eps, "minpts": a.minpts, "dbscan_ms": round(ts[best] * 1e3, 3),
               "pair_ms": round(c["pair_ns"] / 1e6, 3), "filter_ms": round(c["filter_ns"] / 1e6, 3),
               "components_ms": round(c["components_ns"] / 1e6, 3), "chunks": c["chunks"],
               "candidate_edges": c["candidate_edges"], "eps_edges": c["eps_edges"], "core_points": c["core_points"],
               "hook_rounds": c["hook_rounds"], "clusters": int(lab.max()) + 1, "noise": int((lab < 0).sum())}
        if a.knn > 0:
            kcs = []

            def knn_call():
                out = ctx.dbscan_knn(sk, a.eps, a.minpts, kmer, a.knn)
                kcs.append(ctx.dbscan_knn_counters())
                return out
            knn_ms, klab = _best(knn_call, a.repeat)
            kc = min(kcs[1:], key=lambda x: x["total_ns"])
            row["knn"] = {"k": a.knn, "call_ms": round(knn_ms, 3), "library_ms": round(kc["total_ns"] / 1e6, 3),
                          "select_ms": round(kc["select_ns"] / 1e6, 3), "propagate_ms": round(kc["propagate_ns"] / 1e6, 3),
                          "chunks": kc["chunks"], "candidate_edges": kc["candidate_edges"], "passers": kc["passers"],
                          "truncated_rows": kc["truncated_rows"], "arrival_rows": kc["arrival_rows"],
                          "neighbour_edges": kc["neighbour_edges"], "core_points": kc["core_points"], "rounds": kc["rounds"],
                          "clusters": int(klab.max(initial=-1)) + 1, "noise": int((klab < 0).sum()),
                          "points_labelled_differently": int((klab != lab).sum())}
        if not a.no_mst:
            ctx.mst(sk, a.eps)
            tm = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                ctx.mst(sk, a.eps)
                tm.append(time.perf_counter() - t0)
            row["mst_ms"] = round(min(tm) * 1e3, 3)
        print(json.dumps(row), flush=True)
        del sk
    ctx.close()


if __name__ == "__main__":
    main()
