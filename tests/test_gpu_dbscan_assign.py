"""clust-dbscan --db --assign on the GPU (rtc_dbscan_assign): every record field by field against the brute-force restatement of
the placement rule (tests/refdbscan_assign.py) for KSSD and MinHash models, both fold paths, query chunks, the tie to the
clustering itself (a border or noise point taken out and assigned back), the error returns and the command line end to end.
No tolerances: the records are integers, and the printed distances are the host's on both sides."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refdbscan_assign as A
from tests import refdbscan_mash as M
from tests.test_gpu_dbscan import BIN, _write_fastas
from tests.test_gpu_dbscan_mash import _edge_case_set, _families

pytestmark = pytest.mark.gpu

K = 21


def _set(ctx, sketches, width, kind="kssd"):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=K, kind=kind, width=width)


def _same(got, want, what):
    for f in A.PLACE_DT.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, [(int(q), got[q].tolist(), want[q].tolist()) for q in bad[:4]])


# ---- KSSD -------------------------------------------------------------------------------------------------------------
def _kssd_case():
    """300 model points (30 families x 10 at three substitution rates) and two lone near-identical points; 40 queries: mutated
    family members, a copy of a model point, an empty one, unrelated ones, one next to the lone pair only, one built from two
    families"""
    rng = np.random.default_rng(5)

    def fresh(m):
        return rng.choice((1 << 31) - 2, size=m, replace=False).astype(np.int64) + 1

    def mutate(base, rate):
        s = base.copy()
        flip = rng.random(len(s)) < rate
        s[flip] = fresh(int(flip.sum()))
        return np.unique(s)
    bases, model = [], []
    for f in range(30):
        base = fresh(200 + 7 * (f % 5))
        bases.append(base)
        model += [mutate(base, (0.02, 0.1, 0.3)[f % 3]) for _ in range(10)]
    lone = fresh(150)
    model += [np.unique(lone), mutate(lone, 0.02)]
    queries = [mutate(bases[f % 30], (0.02, 0.1, 0.3, 0.5)[f % 4]) for f in range(33)]
    queries += [model[3].copy(), np.zeros(0, dtype=np.int64), fresh(180), fresh(90), mutate(lone, 0.02),
                np.unique(np.concatenate([bases[0][:100], bases[3][:100]])), mutate(bases[29], 0.02)]
    assert len(model) == 302 and len(queries) == 40
    return model, queries


@pytest.mark.parametrize("width", [4, 8])
def test_kssd_records_equal_the_restatement(ctx, width):
    model, queries = _kssd_case()
    sk_model, sk_all = _set(ctx, model, width), _set(ctx, model + queries, width)
    seen = set()
    for eps in (0.02, 0.05):
        for min_pts in (1, 2, 5):
            labels, core = ctx.dbscan(sk_model, eps, min_pts, K, return_core=True)
            got = ctx.dbscan_assign(sk_all, len(model), labels, core, eps, min_pts, K)
            want = A.place_all(model, labels, core, queries, eps, min_pts, K, use64=width == 8)
            _same(got, want, (width, eps, min_pts))
            c = ctx.dbscan_assign_counters()
            assert c["chunks"] == 1 and c["neighbours"] == int(want["n_neighbours"].sum())
            assert c["placed"] == int((want["label"] >= 0).sum()) and c["novel"] == int((want["label"] < 0).sum())
            assert c["bridging"] == int((want["label"] != want["label_max"]).sum()) and c["fold_paths"] == 1
            assert want["nearest"][33] == 3 and want["common"][33] == want["denom"][33] == len(model[3])  # the copy
            assert want[34].tolist() == (-1, -1, 0, 0, A.NONE, 0, 0, int(min_pts <= 1))  # empty: no neighbour at either width
            assert want["nearest"][35] == A.NONE and want["nearest"][36] == A.NONE  # no shared hash
            if want["n_neighbours"][37] == 2 and want["n_core"][37] == 0:
                seen.add("non-core only")
            if want["label"][38] != want["label_max"][38]:
                seen.add("bridge")
            if ((want["label"] >= 0) & (want["flags"] == 0)).any():
                seen.add("border")
    assert seen == {"non-core only", "bridge", "border"}


def test_kssd_empty_query_at_width_8(ctx):
    # the u64 brute force has no emptiness test: the empty sketches are each other's neighbours, and an empty query theirs
    model = [np.arange(100), np.zeros(0), np.arange(50, 150), np.zeros(0), np.zeros(0)]
    queries = [np.zeros(0), np.arange(100)]
    for width in (8, 4):
        for min_pts in (2, 3, 4, 5):
            labels, core = ctx.dbscan(_set(ctx, model, width), 0.05, min_pts, K, return_core=True)
            got = ctx.dbscan_assign(_set(ctx, model + queries, width), 5, labels, core, 0.05, min_pts, K)
            _same(got, A.place_all(model, labels, core, queries, 0.05, min_pts, K, use64=width == 8), (width, min_pts))
            assert int(got["n_neighbours"][0]) == (3 if width == 8 else 0) and int(got["nearest"][0]) == A.NONE
    labels, core = ctx.dbscan(_set(ctx, model, 8), 0.05, 3, K, return_core=True)
    assert core.tolist() == [False, True, False, True, True]
    got = ctx.dbscan_assign(_set(ctx, model + queries, 8), 5, labels, core, 0.05, 3, K)
    assert got[0].tolist() == (int(labels[1]), int(labels[1]), 3, 3, A.NONE, 0, 0, 1)


# ---- MinHash ----------------------------------------------------------------------------------------------------------
def test_minhash_records_equal_the_restatement(ctx, oracle):
    _, host, _ = _families(ctx, oracle, 1)
    model = [np.asarray(h) for h in host]
    rng = np.random.default_rng(9)
    queries = []
    for i in range(34):  # a model sketch with some hashes drawn anew: a genome of the same family, mutated
        src = model[int(rng.integers(0, 300))]
        keep = src[rng.random(len(src)) >= (0.02, 0.1, 0.3)[i % 3]]
        new = rng.integers(1, 1 << 62, size=128, dtype=np.int64).astype(np.uint64)
        queries.append(np.unique(np.concatenate([keep, new]))[:128])
    queries += [model[7].copy(), np.zeros(0, dtype=np.uint64), np.unique(rng.integers(1, 1 << 62, size=128, dtype=np.int64).astype(np.uint64)),
                np.unique(np.concatenate([model[0][:64], model[299][:64]])), model[150][:40].copy(), model[150][60:].copy()]
    assert len(queries) == 40
    sk_model, sk_all = _set(ctx, model, 8, "minhash"), _set(ctx, model + queries, 8, "minhash")
    cases = set()
    for eps in (0.01, 0.04):
        for min_pts in (1, 2, 5):
            labels, core = ctx.dbscan_mash(sk_model, 128, [eps], min_pts, K, return_core=True)
            got = ctx.dbscan_assign(sk_all, 300, labels[0], core[0], eps, min_pts, K, sketch_size=128)
            want = A.place_all(model, labels[0], core[0], queries, eps, min_pts, K, sketch_size=128)
            _same(got, want, (eps, min_pts))
            c = ctx.dbscan_assign_counters()
            assert c["candidates"] > 0 and c["neighbours"] == int(want["n_neighbours"].sum())
            assert want["nearest"][34] == 7 and want["common"][34] == want["denom"][34] == 128
            assert want["nearest"][35] == A.NONE and want["nearest"][36] == A.NONE
            cases.add((int((want["label"] >= 0).sum()), int((want["flags"] & 1).sum())))
    assert len(cases) >= 4


@pytest.mark.parametrize("s,width", [(1, 8), (64, 8), (65, 8), (65, 4)])
def test_minhash_truncated_counts_at_chunk_ends(ctx, s, width):
    sets = _edge_case_set(s, np.random.default_rng(1000 + s))
    model, queries = sets[::2], sets[1::2]  # the hand-built pairs are split between the two
    sk_model, sk_all = _set(ctx, model, width, "minhash"), _set(ctx, model + queries, width, "minhash")
    for eps, min_pts in ((0.05, 2), (0.3, 0)):
        labels, core = ctx.dbscan_mash(sk_model, s, [eps], min_pts, K, return_core=True)
        got = ctx.dbscan_assign(sk_all, len(model), labels[0], core[0], eps, min_pts, K, sketch_size=s)
        _same(got, A.place_all(model, labels[0], core[0], queries, eps, min_pts, K, sketch_size=s), (s, width, eps))
    assert (got["nearest"] != A.NONE).any()


# ---- fold paths, chunks ---------------------------------------------------------------------------------------------
_FOLD = {}


def _fold_case(ctx):
    """5 000 near-duplicates of one 16-hash sketch and 200 of another: a query of the first group has a segment past the wave
    path's tile of 4 096 records, one of the second group lies below it"""
    if not _FOLD:
        rng = np.random.default_rng(11)
        base_a, base_b = np.arange(1000, 1016), np.arange(5000, 5016)

        def variant(base, g):
            s = base.copy()
            s[g % 16] = 1_000_000 + g  # distinct sketches: one hash of its own each
            return np.sort(s)
        model = [variant(base_a, g) for g in range(5000)] + [variant(base_b, g) for g in range(5000, 5200)]
        queries = [base_a, variant(base_a, 77), base_b, variant(base_b, 5100), rng.integers(1 << 24, 1 << 30, 16)]
        queries = [np.unique(q) for q in queries]
        labels, core = ctx.dbscan(_set(ctx, model, 4), 0.05, 5, K, return_core=True)
        want = A.place_all(model, labels, core, queries, 0.05, 5, K)
        _FOLD.update(model=model, queries=queries, labels=labels, core=core, want=want)
    return _FOLD


def test_both_fold_paths(ctx):
    f = _fold_case(ctx)
    model, queries, want = f["model"], f["queries"], f["want"]
    assert want["n_neighbours"].tolist()[:4] == [5000, 5000, 200, 200] and want["nearest"].tolist()[1] == 77
    for pick, paths in (([0, 1, 2, 3, 4], 3), ([0, 1], 2), ([2, 3, 4], 1)):
        got = ctx.dbscan_assign(_set(ctx, model + [queries[i] for i in pick], 4), len(model), f["labels"], f["core"], 0.05, 5, K)
        _same(got, want[pick], pick)
        assert ctx.dbscan_assign_counters()["fold_paths"] == paths


def test_query_chunks_and_edge_budget(ctx):
    f = _fold_case(ctx)
    sk = _set(ctx, f["model"] + f["queries"], 4)
    for chunk, chunks in ((0, 1), (1, 5), (7, 1), (2, 3)):
        got = ctx.dbscan_assign(sk, len(f["model"]), f["labels"], f["core"], 0.05, 5, K, query_chunk=chunk)
        _same(got, f["want"], chunk)
        assert ctx.dbscan_assign_counters()["chunks"] == chunks
    with ctx.env(RTC_EDGE_BUDGET="1024"):  # room for one query's candidates (n_db + 1 024): the chunk of five is halved twice
        got = ctx.dbscan_assign(sk, len(f["model"]), f["labels"], f["core"], 0.05, 5, K)
        c = ctx.dbscan_assign_counters()
    _same(got, f["want"], "budget")
    assert c["chunks"] >= 4 and c["candidates"] == 2 * 5000 + 2 * 200
    model, queries = _kssd_case()
    sk = _set(ctx, model + queries, 8)
    labels, core = ctx.dbscan(_set(ctx, model, 8), 0.05, 2, K, return_core=True)
    ref = ctx.dbscan_assign(sk, len(model), labels, core, 0.05, 2, K)
    for chunk in (1, 7):
        _same(ctx.dbscan_assign(sk, len(model), labels, core, 0.05, 2, K, query_chunk=chunk), ref, chunk)
        assert ctx.dbscan_assign_counters()["chunks"] == -(-40 // chunk)


# ---- consistency with the clustering ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kssd4", "kssd8", "minhash"])
def test_border_and_noise_points_come_back_to_their_label(ctx, kind):
    sets = A.satellite_set(2, kind != "kssd4")
    width, s = (4 if kind == "kssd4" else 8), (300 if kind == "minhash" else None)
    checked = {"cluster": 0, "noise": 0}
    for eps, min_pts in ((0.04, 5),):
        def run(points):
            sk = _set(ctx, points, width, "minhash" if s else "kssd")
            if s:
                lab, cr = ctx.dbscan_mash(sk, s, [eps], min_pts, K, return_core=True)
                return lab[0], cr[0]
            return ctx.dbscan(sk, eps, min_pts, K, return_core=True)
        full_labels, full_core = run(sets)
        for p in np.flatnonzero(~full_core):
            rest = [x for i, x in enumerate(sets) if i != p]
            labels, core = run(rest)
            if not np.array_equal(core, np.delete(full_core, p)):
                continue  # p held a core point up
            got = ctx.dbscan_assign(_set(ctx, rest + [sets[p]], width), len(rest), labels, core, eps, min_pts, K, sketch_size=s)
            assert np.array_equal(labels, np.delete(full_labels, p))
            assert int(got["label"][0]) == int(full_labels[p]) and not int(got["flags"][0]) & 1, (kind, eps, int(p))
            checked["cluster" if full_labels[p] >= 0 else "noise"] += 1
    assert checked["cluster"] >= 5 and checked["noise"] >= 5, checked


# ---- error returns ------------------------------------------------------------------------------------------------------
def test_error_returns(ctx):
    from rabbittclust_amd import api
    sets = [np.arange(10), np.arange(5, 15), np.arange(3, 13)]
    sk = _set(ctx, sets, 8)
    labels, core = np.array([0, 0], dtype=np.int32), np.array([1, 1], dtype=np.uint8)

    def fails(status, text, *a, **kw):
        with pytest.raises(api.RtcError) as ei:
            ctx.dbscan_assign(*a, **kw)
        assert ei.value.status == status and text in str(ei.value), str(ei.value)
    fails(api._lib.RTC_ERR_ARG, "is not in [0, 1)", sk, 2, labels, core, -0.1, 1, K, sketch_size=10)
    fails(api._lib.RTC_ERR_ARG, "is not in [0, 1)", sk, 2, labels, core, float("nan"), 1, K, sketch_size=10)
    fails(api._lib.RTC_ERR_UNSUPPORTED, "from 1 on", sk, 2, labels, core, 1.0, 1, K, sketch_size=10)
    fails(api._lib.RTC_ERR_ARG, "sketch size 0", sk, 2, labels, core, 0.1, 1, K, sketch_size=0)
    fails(api._lib.RTC_ERR_UNSUPPORTED, "jaccard_min", sk, 2, labels, core, 5.0, 1, K)  # exp(-105): t <= 1e-12
    fails(api._lib.RTC_ERR_ARG, "h_labels", sk, 2, None, core, 0.05, 1, K)
    fails(api._lib.RTC_ERR_ARG, "h_core", sk, 2, labels, None, 0.05, 1, K)
    with pytest.raises(ValueError):
        ctx.dbscan_assign(sk, 4, labels, core, 0.05, 1, K)
    assert ctx.dbscan_assign(sk, 3, [0, 0, 0], [1, 1, 1], 0.05, 1, K).shape == (0,)  # no query
    got = ctx.dbscan_assign(sk, 0, [], [], 0.05, 1, K)  # no model: everything is novel
    assert got["label"].tolist() == [-1] * 3 and got["nearest"].tolist() == [A.NONE] * 3 and got["flags"].tolist() == [1] * 3
    got = ctx.dbscan_assign(sk, 2, labels, core, 0.05, 1, K)
    assert got[0].tolist() == (0, 0, 2, 2, 1, 8, 12, 1)  # shares 7 with the first, 8 with the second


# ---- the command line ---------------------------------------------------------------------------------------------------
def _cli(args, cwd, env=None, fails=False):
    r = subprocess.run([os.path.join(BIN, "clust-dbscan")] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env) if env else None)
    assert (r.returncode == 1) if fails else (r.returncode == 0), r.stderr[-3000:]
    return r.stderr


@pytest.mark.parametrize("kind", ["kssd", "minhash"])
def test_cli_build_assign_end_to_end(oracle, tmp_path, kind):
    tmp = str(tmp_path)
    mash = kind == "minhash"
    # eps 0.08, minPts 3: every family is one cluster, three of the new members find theirs and one does not
    L, k, s, eps, min_pts = (500_000, 19, 128, 0.08, 3) if mash else (1_000_000, 17, None, 0.08, 3)
    _, seqs, meta = _write_fastas(oracle, tmp, 4, 5, L, seed=9)
    other = os.path.join(tmp, "other"); os.makedirs(other)
    _, seqs2, meta2 = _write_fastas(oracle, other, 1, 1, L, seed=77)
    db_ids = [g for g in range(20) if g % 5 != 4]
    q_seqs = [seqs[g] for g in range(20) if g % 5 == 4] + seqs2  # one more member of every family, and a stranger
    q_meta = [meta[g] for g in range(20) if g % 5 == 4] + meta2
    db_list, q_list = os.path.join(tmp, "db.txt"), os.path.join(tmp, "q.txt")
    open(db_list, "w").write("".join(meta[g][0] + "\n" for g in db_ids))
    open(q_list, "w").write("".join(m[0] + "\n" for m in q_meta))

    def sketch(batch):
        if mash:
            off = np.arange(len(batch) + 1, dtype=np.uint64) * L
            return [np.asarray(h) for h in oracle.sketch_minhash_batch(np.concatenate(batch), off, k, s)]
        return [oracle.kssd_sketch(x, k, 3) for x in batch]
    db_sk, q_sk = sketch([seqs[g] for g in db_ids]), sketch(q_seqs)
    if mash:
        want, want_core = M.labels_of(M.distance_matrix(M.count_matrix(db_sk, s), k), eps, min_pts)
    else:
        want = R.labels_of(db_sk, eps, min_pts, k, False)
        want_core = np.array([len(x) + 1 >= min_pts for x in R.neighbour_lists(db_sk, eps, k, False)])
    flags = ["--minhash", "-s", str(s)] if mash else ["--fast"]
    common = flags + ["-l", "-i", db_list, "-k", str(k), "--eps", str(eps), "--minpts", str(min_pts), "-t", "4", "-e"]
    # --build: the ordinary run, byte for byte, and the model beside it
    plain, built, db = os.path.join(tmp, "plain.out"), os.path.join(tmp, "built.out"), os.path.join(tmp, "model.db")
    _cli(common + ["-o", plain], tmp)
    err = _cli(common + ["--db", db, "--build", "-o", built], tmp)
    assert open(built, "rb").read() == open(plain, "rb").read() and "-----write the DBSCAN model (16 genomes" in err
    assert open(built).read() == R.print_result(want, [meta[g] for g in db_ids], True, eps, min_pts) and not os.path.exists(db + ".tmp")
    m = A.parse_model(open(db, "rb").read())
    assert (m["version"], m["kind"], m["width"], m["by_file"], m["kmer_size"], m["min_pts"], m["max_posting"]) == (1, int(mash), 8 if mash else 4, 1, k, min_pts, 0)
    assert m["eps"] == eps and m["n"] == 16 and m["n_clusters"] == int(want.max()) + 1 and m["min_len"] == 10000
    assert (m["sketch_size"] == s) if mash else ((m["half_k"], m["drlevel"]) == (9, 3))
    assert np.array_equal(m["labels"], want) and np.array_equal(m["core"].astype(bool), want_core)
    assert all(np.array_equal(a, b) for a, b in zip(m["sketches"], db_sk))
    assert [(g["file"], g["total_length"], g["name"], g["comment"]) for g in m["genomes"]] == [meta[g] for g in db_ids]
    # --assign from a list: the TSV the restatement predicts from the model file and the queries' oracle sketches
    recs = A.place_all(m["sketches"], m["labels"], m["core"], q_sk, eps, min_pts, k, use64=False, sketch_size=s)
    assert recs["label"].tolist() == [0, 1, 2, -1, -1] and recs["nearest"][3] != A.NONE and recs["nearest"][4] == A.NONE
    tsv, mj = os.path.join(tmp, "assign.tsv"), os.path.join(tmp, "assign.json")
    err = _cli(["--db", db, "--assign", "-l", "-i", q_list, "-k", "31", "--eps", "0.9", "--minpts", "40", "-t", "4", "-o", tsv], tmp,
               env={"RTC_METRICS_JSON": mj})
    assert open(tsv).read() == A.tsv([x[0] for x in q_meta], recs, [g["file"] for g in m["genomes"]], k, s)
    metrics = json.load(open(mj))
    assert metrics["command"] == "clust-dbscan" and metrics["sketch"] == kind
    for key in ("dbscan_assign_join_s", "dbscan_assign_predicate_s", "dbscan_assign_fold_s"):
        assert metrics[key] >= 0, key
    assert (metrics["dbscan_assign_placed"], metrics["dbscan_assign_novel"], metrics["dbscan_assign_bridging"]) == (3, 2, 0)
    # the same queries as the records of one FASTA, without -l: the same placements under the records' names
    fa = os.path.join(tmp, "queries.fna")
    with open(fa, "wb") as f:
        for g, x in enumerate(q_seqs):
            f.write(f">r{g} query {g}\n".encode() + x.tobytes() + b"\n")
    tsv2 = os.path.join(tmp, "assign2.tsv")
    _cli(flags[:1] + ["--db", db, "--assign", "-i", fa, "-t", "4", "-o", tsv2], tmp)
    assert open(tsv2).read() == A.tsv(["r%d" % g for g in range(5)], recs, [g["file"] for g in m["genomes"]], k, s)
    # a model flagged with --max-posting is refused, by name, as is a model of the other kind
    blob = bytearray(open(db, "rb").read())
    struct.pack_into("<i", blob, 8 + 4 * 10, 7)
    open(os.path.join(tmp, "mp.db"), "wb").write(bytes(blob))
    err = _cli(["--db", "mp.db", "--assign", "-l", "-i", q_list, "-o", os.path.join(tmp, "x.tsv")], tmp, fails=True)
    assert "was built with --max-posting 7" in err and "context" not in err
    err = _cli(["--fast" if mash else "--minhash", "--db", db, "--assign", "-l", "-i", q_list, "-o", os.path.join(tmp, "x.tsv")], tmp, fails=True)
    assert "--assign: " in err and ("is a MinHash model" if mash else "is a KSSD model") in err
