"""clust-dbscan --db --update on the GPU (rtc_dbscan_update): labels and core flags against the full call on the union
(Context.dbscan / Context.dbscan_mash), the stage row counts and the promoted / merged counters against the plain-Python
restatement of the two-stage rule (tests/refdbscan_update.py), the crafted event sets, family sets at both widths and kinds, the
edge cases, and the command line against --build over both lists.  No tolerances: everything is an integer."""
import os
import subprocess

import numpy as np
import pytest

from tests import refdbscan_assign as A
from tests import refdbscan_update as U
from tests.test_gpu_dbscan import BIN, _write_fastas

pytestmark = pytest.mark.gpu

K = U.GRAPH_K
S = U.GRAPH_SKETCH_SIZE
KINDS = [("kssd", 4), ("kssd", 8), ("minhash", 8)]


def _set(ctx, sketches, kind, width):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=K, kind=kind, width=width)


def _full(ctx, sk, kind, eps, min_pts, sketch_size):
    if kind == "minhash":
        lab, core = ctx.dbscan_mash(sk, sketch_size, [eps], min_pts, K, return_core=True)
        return lab[0].copy(), core[0].copy()
    return ctx.dbscan(sk, eps, min_pts, K, return_core=True)


def _update(ctx, sk_all, n_old, lab_old, core_old, kind, eps, min_pts, sketch_size):
    return ctx.dbscan_update(sk_all, n_old, lab_old, core_old, eps, min_pts, K, sketch_size=sketch_size if kind == "minhash" else None)


def _check(ctx, sketches, n_old, kind, width, eps, min_pts, sketch_size=S, restate=True):
    """the full call on the first n_old, the update with the rest, against the full call on all and the restatement's rows"""
    sk_all = _set(ctx, sketches, kind, width)
    lab_old, core_old = _full(ctx, _set(ctx, sketches[:n_old], kind, width), kind, eps, min_pts, sketch_size)
    got, got_core = _update(ctx, sk_all, n_old, lab_old, core_old, kind, eps, min_pts, sketch_size)
    c = ctx.dbscan_update_counters()
    counts = ctx.dbscan_update_counts
    want, want_core = _full(ctx, sk_all, kind, eps, min_pts, sketch_size)
    assert np.array_equal(got, want), (kind, width, n_old, min_pts, np.flatnonzero(got != want)[:8].tolist())
    assert np.array_equal(got_core, want_core), (kind, width, n_old, min_pts, np.flatnonzero(got_core != want_core)[:8].tolist())
    assert counts == (int(want.max(initial=-1)) + 1, int((want < 0).sum()))
    info = None
    if restate:
        rel = U.mash_relation(sketches, sketch_size, eps, K) if kind == "minhash" else U.kssd_relation(sketches, eps, K, width == 8)
        lab, core, info = U.update(n_old, len(sketches), rel, lab_old, core_old, U.need_of(min_pts, kind == "minhash"))
        assert np.array_equal(lab, want) and np.array_equal(core, want_core)
        assert (c["stage1_rows"], c["stage2_rows"]) == (len(info["rows1"]), len(info["rows2"])), (c, len(info["rows2"]))
        assert (c["promoted"], c["merged"]) == (info["promoted"], info["merged"]), (c, info["promoted"], info["merged"])
        if all(len(s) for s in sketches):  # (the empty u64 sketches are neighbours without a pair of the list)
            assert c["kept_edges"] == info["kept"]
    return c, info, got


# ---- the events ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("event", sorted(U.CRAFTED))
def test_crafted_event_sets(ctx, event):
    n_old, n, edges, min_pts = U.CRAFTED[event]
    for kind, width in KINDS:
        sk = U.graph_sketches(n, edges, np.random.default_rng(3), use64=width == 8)
        c, info, _ = _check(ctx, sk, n_old, kind, width, U.GRAPH_EPS, min_pts - (kind == "minhash"))
        assert event in info["events"], (event, kind, width)
    if event == "clusters merged":
        assert c["merged"] == 1
    if event in ("noise promoted", "border promoted"):
        assert c["promoted"] == 1


# ---- family sets --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", KINDS)
def test_family_sets(ctx, kind, width):
    seen = set()
    for seed, eps, min_pts in ((1, 0.04, 5), (2, 0.02, 3)):
        sk, n_old = U.family_sets(seed, width == 8)
        assert n_old == 300 and len(sk) == 360 and max(len(s) for s in sk) <= 200
        c, info, _ = _check(ctx, sk, n_old, kind, width, eps, min_pts - (kind == "minhash"), sketch_size=256)
        assert c["stage1_rows"] == 60 and 0 < c["stage2_rows"] < n_old and c["chunks"] >= 2 and c["hook_rounds"] >= 1
        seen |= info["events"]
    assert {"noise promoted", "border promoted"} & seen, seen


def test_rows_are_few_where_the_old_points_are_core(ctx):
    sk, n_old = U.mostly_core_set(np.random.default_rng(8))
    c, info, _ = _check(ctx, sk, n_old, "kssd", 4, U.GRAPH_EPS, 3)
    assert 0 < c["stage2_rows"] < n_old // 4, c


# ---- edge cases ---------------------------------------------------------------------------------------------------------
def test_no_new_and_no_old_points(ctx):
    n_old, n, edges, min_pts = U.CRAFTED["clusters merged"]
    sk = U.graph_sketches(n, edges, np.random.default_rng(3))
    for kind, width in KINDS:
        mp = min_pts - (kind == "minhash")
        dev = _set(ctx, sk, kind, width)
        lab, core = _full(ctx, dev, kind, U.GRAPH_EPS, mp, S)
        got, got_core = _update(ctx, dev, n, lab, core, kind, U.GRAPH_EPS, mp, S)  # nothing new: the model as it is
        assert np.array_equal(got, lab) and np.array_equal(got_core, core)
        assert ctx.dbscan_update_counts == (int(lab.max(initial=-1)) + 1, int((lab < 0).sum()))
        c = ctx.dbscan_update_counters()
        assert (c["stage1_rows"], c["stage2_rows"], c["candidate_edges"], c["kept_edges"]) == (0, 0, 0, 0)
        got, got_core = _update(ctx, dev, 0, [], [], kind, U.GRAPH_EPS, mp, S)  # nothing old: the plain call
        assert np.array_equal(got, lab) and np.array_equal(got_core, core)
        c = ctx.dbscan_update_counters()
        assert (c["stage1_rows"], c["stage2_rows"], c["promoted"], c["merged"]) == (n - 1, 0, 0, 0)


def test_empty_sketches_at_width_8(ctx):
    """the u64 brute force has no emptiness test: the empty sketches are each other's neighbours.  A new empty sketch raises
    every old one's count without a candidate pair -- at min_pts 3 two old empty sketches are noise and become core points (as
    do a and a + 1, which a + 2 joins)."""
    a = np.arange(100)
    e = np.zeros(0, dtype=np.int64)
    old, new = [a, e, a + 1, e, np.arange(5000, 5100)], [e, a + 2]
    for min_pts in (2, 3, 4, 5):
        for width in (8, 4):
            c, info, got = _check(ctx, old + new, len(old), "kssd", width, 0.05, min_pts)
            if width == 8 and min_pts == 3:
                assert c["promoted"] == 4 and c["stage2_rows"] == 4 and got[1] == got[3] == got[5] >= 0 and got[1] != got[0]
            if width == 4:
                assert got[1] == got[3] == got[5] == -1
    # old empty core points (min_pts 2) and a new empty one: it joins their cluster; no new empty one: the old ones stay noise
    c, info, got = _check(ctx, old + new, len(old), "kssd", 8, 0.05, 2)
    assert got[5] == got[1] and c["promoted"] == 0
    c, info, got = _check(ctx, old + [a + 2], len(old), "kssd", 8, 0.05, 3)
    assert c["stage2_rows"] == 2 and c["promoted"] == 2 and got[1] == got[3] == -1
    # several new empty sketches and no old one
    _check(ctx, [a, a + 1, np.arange(5000, 5100)] + [e, e, a + 2, e], 3, "kssd", 8, 0.05, 3)


def test_minhash_min_pts_zero(ctx):
    sk, n_old = U.family_sets(3, True, n_old=90, n_new=30)
    for min_pts in (0, -2):
        c, info, got = _check(ctx, sk, n_old, "minhash", 8, 0.04, min_pts, sketch_size=256)
        assert (got >= 0).all() and c["stage2_rows"] == 0 and c["promoted"] == 0  # every point is a core point, before and after


def _dense_candidates_set():
    """300 old points in 150 pairs (noise at min_pts 3) and 200 new ones, 150 of them next to one point of a pair each, which
    they promote: T has 150 points.  Two hashes lie in every sketch, so every pair of sketches is a candidate of the pair phase."""
    edges = [(2 * i + 1, 2 * i) for i in range(150)] + [(300 + i, 2 * i) for i in range(150)] + [(451 + 2 * i, 450 + 2 * i) for i in range(25)]
    return U.graph_sketches(500, edges, np.random.default_rng(12), everywhere=2), 300


def test_edge_budget_chunks_both_stages(ctx):
    sk, n_old = _dense_candidates_set()
    for kind, width in (("kssd", 4), ("minhash", 8)):
        mp = 3 - (kind == "minhash")
        with ctx.env(RTC_EDGE_BUDGET="1024"):  # raised to a 64-row block's: 64 n + 1 024 candidates, n = 500 in stage 1, 300 in stage 2
            c, info, _ = _check(ctx, sk, n_old, kind, width, U.GRAPH_EPS, mp)
        # stage 1 has 200 rows (124 750 - 44 850 = 79 900 candidates), stage 2 150 (33 675): at 64 rows per chunk at most 4 + 3 chunks,
        # so six or more means that each stage took at least two
        assert c["stage1_rows"] == 200 and c["stage2_rows"] == 150 and c["promoted"] == 150
        assert c["candidate_edges"] == 500 * 499 // 2 - 300 * 299 // 2 + 300 * 299 // 2 - 150 * 149 // 2
        assert 6 <= c["chunks"] <= 7, c
        c1, _, _ = _check(ctx, sk, n_old, kind, width, U.GRAPH_EPS, mp, restate=False)  # the default budget: one chunk per stage
        assert c1["chunks"] == 2 and c1["candidate_edges"] == c["candidate_edges"] and c1["kept_edges"] == c["kept_edges"]


def test_five_successive_updates(ctx):
    for kind, width in KINDS:
        sk, _ = U.family_sets(5, width == 8, n_old=100, n_new=100)
        eps, mp = 0.04, 4 - (kind == "minhash")
        lab, core = _full(ctx, _set(ctx, sk[:100], kind, width), kind, eps, mp, 256)
        for n_old in range(100, 200, 20):
            lab, core = _update(ctx, _set(ctx, sk[:n_old + 20], kind, width), n_old, lab, core, kind, eps, mp, 256)
        want, want_core = _full(ctx, _set(ctx, sk, kind, width), kind, eps, mp, 256)
        assert np.array_equal(lab, want) and np.array_equal(core, want_core), (kind, width)


def test_full_call_and_update_on_one_context_in_either_order(ctx):
    """the inverted join keeps a note of the tile it last found too dense, keyed by the hash buffer and the tile: the update's
    view of the same buffer, and a full call after the update, must not read each other's"""
    sk, n_old = _dense_candidates_set()
    for kind, width in (("kssd", 8), ("minhash", 8)):
        mp = 3 - (kind == "minhash")
        dev = _set(ctx, sk, kind, width)
        lab_old, core_old = _full(ctx, _set(ctx, sk[:n_old], kind, width), kind, U.GRAPH_EPS, mp, S)
        first = _full(ctx, dev, kind, U.GRAPH_EPS, mp, S)
        upd = _update(ctx, dev, n_old, lab_old, core_old, kind, U.GRAPH_EPS, mp, S)
        again = _full(ctx, dev, kind, U.GRAPH_EPS, mp, S)
        upd2 = _update(ctx, dev, n_old, lab_old, core_old, kind, U.GRAPH_EPS, mp, S)
        for x in (upd, again, upd2):
            assert np.array_equal(x[0], first[0]) and np.array_equal(x[1], first[1]), (kind,)
        old_dev = _set(ctx, sk[:n_old], kind, width)  # the very tile of the view: n_old rows of the same hashes, in the old order
        assert np.array_equal(_full(ctx, old_dev, kind, U.GRAPH_EPS, mp, S)[0], lab_old)


def test_invalid_old_labels(ctx):
    from rabbittclust_amd import api
    n_old, n, edges, min_pts = U.CRAFTED["clusters merged"]
    sk = U.graph_sketches(n, edges, np.random.default_rng(3))
    dev = _set(ctx, sk, "kssd", 4)
    lab, core = ctx.dbscan(_set(ctx, sk[:n_old], "kssd", 4), U.GRAPH_EPS, min_pts, K, return_core=True)
    assert lab.tolist() == [0, 0, 0, 1, 1, 1] and core.all()

    def fails(text, labels, flags, **kw):
        with pytest.raises(api.RtcError) as ei:
            ctx.dbscan_update(dev, n_old, labels, flags, kw.get("eps", U.GRAPH_EPS), min_pts, K, sketch_size=kw.get("sketch_size"))
        assert ei.value.status == kw.get("status", api._lib.RTC_ERR_ARG) and text in str(ei.value), str(ei.value)
    fails("core point without a cluster", [0, 0, -1, 1, 1, 1], core)
    fails("old cluster 1 of 3 has no core point", [0, 0, 0, 2, 2, 2], core)
    fails("old cluster 1 of 2 has no core point", lab, [1, 1, 1, 0, 0, 0])
    fails("old label -2", [0, 0, -2, 1, 1, 1], [1, 1, 0, 1, 1, 1])
    fails("labels or core flags are missing", None, None)
    fails("is not in [0, 1)", lab, core, eps=-0.5, sketch_size=S)
    fails("pairs without a common hash are neighbours", lab, core, eps=1.0, sketch_size=S, status=api._lib.RTC_ERR_UNSUPPORTED)
    fails("jaccard_min", lab, core, eps=5.0, status=api._lib.RTC_ERR_UNSUPPORTED)
    with pytest.raises(ValueError):
        ctx.dbscan_update(dev, n + 1, lab, core, U.GRAPH_EPS, min_pts, K)
    got, _ = ctx.dbscan_update(dev, n_old, lab, core, U.GRAPH_EPS, min_pts, K)  # and the context still works
    assert got.tolist() == [0] * 9


# ---- the command line ---------------------------------------------------------------------------------------------------
def _cli(args, cwd, env=None):
    r = subprocess.run([os.path.join(BIN, "clust-dbscan")] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.mark.parametrize("kind", ["kssd", "minhash"])
def test_cli_build_then_update_equals_build_over_both(oracle, tmp_path, kind):
    import json
    tmp = str(tmp_path)
    mash = kind == "minhash"
    L, k, s, eps, min_pts = (500_000, 19, 128, 0.08, 3) if mash else (1_000_000, 17, None, 0.08, 3)
    _, seqs, meta = _write_fastas(oracle, tmp, 4, 5, L, seed=9)
    other = os.path.join(tmp, "other"); os.makedirs(other)
    _, seqs2, meta2 = _write_fastas(oracle, other, 1, 2, L, seed=77)
    # list A: three members of families 0 - 2 and one of family 3 (noise at minPts 3); list B: the others and two of a new family
    ids_a = [g for g in range(20) if (g % 5 < 3 and g < 15) or g == 15]
    ids_b = [g for g in range(20) if g not in ids_a]
    la, lb, lab = (os.path.join(tmp, x) for x in ("a.txt", "b.txt", "ab.txt"))
    open(la, "w").write("".join(meta[g][0] + "\n" for g in ids_a))
    open(lb, "w").write("".join(meta[g][0] + "\n" for g in ids_b) + "".join(m[0] + "\n" for m in meta2))
    open(lab, "w").write(open(la).read() + open(lb).read())
    flags = ["--minhash", "-s", str(s)] if mash else ["--fast"]
    common = flags + ["-k", str(k), "--eps", str(eps), "--minpts", str(min_pts), "-t", "4", "-e", "-l"]
    both_out, both_db = os.path.join(tmp, "both.dbscan"), os.path.join(tmp, "both.db")
    _cli(common + ["-i", lab, "--db", both_db, "--build", "-o", both_out], tmp)
    db = os.path.join(tmp, "model.db")
    _cli(common + ["-i", la, "--db", db, "--build", "-o", os.path.join(tmp, "a.dbscan")], tmp)
    before = A.parse_model(open(db, "rb").read())
    upd_out, mj = os.path.join(tmp, "updated.dbscan"), os.path.join(tmp, "update.json")
    err = _cli(["--db", db, "--update", "-l", "-i", lb, "-k", "31", "--eps", "0.9", "--minpts", "40", "-t", "4", "-o", upd_out], tmp,
               env={"RTC_METRICS_JSON": mj})
    assert open(upd_out, "rb").read() == open(both_out, "rb").read()
    assert open(db, "rb").read() == open(both_db, "rb").read() and not os.path.exists(db + ".tmp")
    after = A.parse_model(open(db, "rb").read())
    assert before["n"] == 10 and after["n"] == 22 and "Genomes:     22" in err
    assert [g["file"] for g in after["genomes"]] == open(lab).read().split()
    metrics = json.load(open(mj))
    assert metrics["command"] == "clust-dbscan" and metrics["sketch"] == kind and metrics["genomes"] == 22
    for key in ("dbscan_update_join_s", "dbscan_update_predicate_s", "dbscan_update_components_s"):
        assert metrics[key] >= 0, key
    assert 12 <= metrics["dbscan_update_rows"] <= 22 and metrics["dbscan_update_promoted"] >= 0 and metrics["dbscan_update_merged"] >= 0
    # the updated model is a model: --stats reads it and --assign places genomes into it
    tsv = os.path.join(tmp, "assign.tsv")
    _cli(["--db", db, "--assign", "-l", "-i", lb, "-t", "4", "-o", tsv], tmp)
    lines = open(tsv).read().splitlines()
    assert len(lines) == 1 + 12
