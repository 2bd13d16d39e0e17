"""clust-dbscan --minhash on the GPU (rtc_dbscan_mash): the recount kernel against rtc_pair_mash_dev on every pair of sets
built around its edge cases, the labels against the restated MinHashDBSCAN (tests/refdbscan_mash.py), truncation, the core
rule, the eps boundary, the sweep, row chunks, the prefilter, the error returns and the command line end to end.  No
tolerances: counts and labels are integers, and the distances are the host's on both sides."""
import json
import os

import numpy as np
import pytest

from tests import refdbscan_mash as M
from tests.test_gpu_dbscan import BIN, _folders, _run as _run_plain, _write_fastas

pytestmark = pytest.mark.gpu

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))
K = 21


def _set(ctx, sketches, width=8):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=K, kind="minhash", width=width)


# ---- (a) the recount -------------------------------------------------------------------------------------------
def _edge_case_set(s, rng):
    """96 ascending lists of at most s distinct values below 2^31: hand-built pairs around the place of the s-th union element
    (the kernel walks the first list in chunks of 64 and ranks every element in the second), short, single and empty lists,
    and random families to fill up"""
    a = 100_000 + 10 * np.arange(s, dtype=np.int64)  # the base list
    sets = [a, a.copy(), a + 5, a + 10 * s]  # identical (the s-th element shared and the last of both), interleaved, disjoint
    for t in (1, 63, 64, 65):  # shifted windows of one progression: the s-th union element is a[s - 1], shared, the last of a
        sets.append(100_000 + 10 * (np.arange(s, dtype=np.int64) + min(t, s)))
    for idx in (0, 62, 63, 64, 65, 127, 128, s - 1):  # a[idx] is the s-th union element: s - 1 - idx values of b lie below a[0]
        if not 0 <= idx < s:
            continue
        low = np.arange(1, s - idx, dtype=np.int64)
        tail = a[idx] + 1 + 10 * np.arange(s, dtype=np.int64)
        sets.append(np.concatenate([low, [a[idx]], tail])[:s])       # ... and shared
        sets.append(np.concatenate([low, tail])[:s])                 # ... and not shared: b's next one comes after it
        sets.append(np.concatenate([low, a[idx:]])[:s])              # ... and every later one shared too
    half = max(s // 2, 1)
    sets += [a[s - 1:], a[s - 1:] + 1, a[:1], a[:1] - 1,             # length 1: a's last (shared), above all, a's first, below all
             a[:half], a[s // 4: s // 4 + max(s // 3, 1)],          # both shorter than s: denom < s
             np.concatenate([a[s - 1:], a[-1] + 7 * np.arange(1, half)]),  # the shorter list starts at a's last element
             a[half:], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)]
    while len(sets) < 96:  # families: a random base, members that keep a part of it and draw the rest anew
        base = np.sort(rng.choice(1 << 31, size=s, replace=False))
        for _ in range(min(6, 96 - len(sets))):
            keep = base[rng.random(s) < rng.choice([0.98, 0.8, 0.5])]
            new = rng.choice(1 << 31, size=s, replace=False)
            n_el = int(rng.choice([s, s, max(s - 1, 1), half]))
            sets.append(np.unique(np.concatenate([keep, new]))[:n_el] if rng.random() < 0.5 else
                        np.unique(np.concatenate([keep, new[: max(s - len(keep), 0)]]))[:n_el])
    sets = sets[:96]
    assert all(len(x) <= s and np.all(np.diff(x) > 0) and (len(x) == 0 or (x[0] >= 0 and x[-1] < 2 ** 31)) for x in sets)
    return sets


@pytest.mark.parametrize("width", [8, 4])
@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 1025])
def test_recount_equals_the_dense_estimator(ctx, s, width):
    sets = _edge_case_set(s, np.random.default_rng(1000 + s))
    sk = _set(ctx, sets, width)
    n = len(sets)
    want_c, want_d = ctx.pair_mash(sk, s)
    ctx.sync()
    want_c, want_d = want_c.cpu().numpy().astype(np.uint32), want_d.cpu().numpy().astype(np.uint32)
    # the yardstick itself against the restated merge on the hand-built lists
    for p in range(0, 40, 3):
        for q in range(40):
            assert (want_c[p, q], want_d[p, q]) == M.mash_counts(sets[p].tolist(), sets[q].tolist(), s), (p, q)
    assert want_d.min() < s or s == 1  # some pairs run out before s union elements
    pairs = np.array([(p, q) for p in range(n) for q in range(n)])
    for serial in (None, "1"):
        with ctx.env(RTC_DBSCAN_MASH_SERIAL=serial):
            got_c, got_d = ctx.pair_mash_edges(sk, s, pairs)
        bad = np.flatnonzero((got_c != want_c.ravel()) | (got_d != want_d.ravel()))
        assert bad.size == 0, (serial, [(pairs[e].tolist(), int(got_c[e]), int(got_d[e]), int(want_c.ravel()[e]), int(want_d.ravel()[e]))
                                        for e in bad[:5]])


# ---- (b) labels == the walk --------------------------------------------------------------------------------------
_FAMILY_CACHE = {}


def _families(ctx, oracle, seed, n_fam=30, per=10, L=20_000, s=128):
    """sketches of synthetic families from the oracle's sketcher, their device set and the restated distances (computed once)"""
    if seed not in _FAMILY_CACHE:
        from rabbittclust_amd import api
        desc = api.synth_family_descs(n_fam, per, global_seed=seed)
        seq = np.concatenate([oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), L) for d in desc])
        off = np.arange(len(desc) + 1, dtype=np.uint64) * L
        host = oracle.sketch_minhash_batch(seq, off, K, s)
        _FAMILY_CACHE[seed] = (host, M.distance_matrix(M.count_matrix(host, s), K))
    host, dist = _FAMILY_CACHE[seed]
    return _set(ctx, host), host, dist


EPS = [0.002, 0.01, 0.02, 0.04, 0.08]


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_labels_match_the_walk(ctx, oracle, seed):
    sk, host, dist = _families(ctx, oracle, seed)
    assert sk.n == 300 and all(len(h) == 128 for h in host)
    seen = set()
    for min_pts in (0, 1, 2, 5, 9):
        got, core = ctx.dbscan_mash(sk, 128, EPS, min_pts, K, return_core=True)
        counts = ctx.dbscan_mash_counts
        for e, eps in enumerate(EPS):
            want, want_core = M.labels_of(dist, eps, min_pts)
            assert np.array_equal(got[e], want), (eps, min_pts, got[e].tolist(), want.tolist())
            assert np.array_equal(core[e], want_core), (eps, min_pts)
            assert counts["clusters"][e] == int(want.max(initial=-1)) + 1 and counts["noise"][e] == int((want < 0).sum())
            seen.add((int(want.max(initial=-1)) + 1, int((want < 0).sum()), bool((~want_core & (want >= 0)).any())))
        if min_pts == 0:
            assert core.all() and (got >= 0).all()
    assert len(seen) >= 8 and any(b for _, _, b in seen)  # the cases differ, and some have border points
    c = ctx.dbscan_mash_counters()
    assert c["levels"] == len(EPS) and c["chunks"] == 1 and c["kept_edges"] <= c["merged"] <= c["candidate_edges"]


# ---- (c) truncation decides ---------------------------------------------------------------------------------------
def test_truncation_decides(ctx):
    s = 100
    a1 = 10_000 + 10 * np.arange(s)
    low = np.concatenate([a1[:50], a1[-1] + 1 + np.arange(50)])    # shares a1's 50 lowest: they lead the union, j = 50 / 100
    a2 = 90_000 + 10 * np.arange(s)
    high = np.concatenate([80_000 + np.arange(50), a2[50:]])       # shares a2's 50 highest: the union's first 100 hold none
    for x, y in ((a1, low), (a2, high)):
        assert len(np.intersect1d(x, y)) == 50 and len(np.union1d(x, y)) == 150  # the same set Jaccard, 1 / 3
    assert M.mash_counts(a1.tolist(), low.tolist(), s) == (50, 100) and M.mash_counts(a2.tolist(), high.tolist(), s) == (0, 100)
    eps = 0.03
    assert M.distance(50, 100, K) < eps < M.distance(50, 150, K) < 1.0  # the set Jaccard would reject both, or accept both above it
    for width in (4, 8):
        sk = _set(ctx, [a1, low, a2, high], width)
        assert ctx.dbscan_mash(sk, s, [eps], 1, K)[0].tolist() == [0, 0, -1, -1]
        assert ctx.dbscan_mash(sk, s, [0.06], 1, K)[0].tolist() == [0, 0, -1, -1]  # above the set Jaccard's distance too


# ---- (d) the core rule ------------------------------------------------------------------------------------------
def test_core_rule_counts_the_neighbours_alone(ctx):
    m = 4
    group = [1000 + np.arange(64)] * (m + 1)  # m + 1 identical sketches: every one has exactly m neighbours
    sk = _set(ctx, group + [5000 + np.arange(64)])
    lab, core = ctx.dbscan_mash(sk, 64, [0.01], m, K, return_core=True)
    assert lab[0].tolist() == [0] * (m + 1) + [-1] and core[0].tolist() == [True] * (m + 1) + [False]
    lab, core = ctx.dbscan_mash(sk, 64, [0.01], m + 1, K, return_core=True)  # |N| + 1 >= minPts would still call them core points
    assert lab[0].tolist() == [-1] * (m + 2) and not core.any()
    # a star of sliding windows (64 hashes, step 16; neighbours within two steps at eps 0.03): the centre has four neighbours,
    # the others three and two, so at minPts 4 it is the only core point and the rest are its border points
    w = [2000 + np.arange(i * 16, i * 16 + 64) for i in range(5)]
    star = [w[2], w[0], w[1], w[3], w[4]]
    want, want_core = M.labels_of(M.distance_matrix(M.count_matrix(star, 64), K), 0.03, 4)
    assert want_core.tolist() == [True, False, False, False, False] and want.tolist() == [0] * 5
    lab, core = ctx.dbscan_mash(_set(ctx, star), 64, [0.03], 4, K, return_core=True)
    assert np.array_equal(lab[0], want) and np.array_equal(core[0], want_core)
    for min_pts in (-2, 0):  # every point a core point, a lone one a cluster of its own
        lab, core = ctx.dbscan_mash(_set(ctx, [w[0], w[0], w[4]]), 64, [0.01], min_pts, K, return_core=True)
        assert lab[0].tolist() == [0, 0, 1] and core.all()


# ---- (e) the boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 37, 90, 127])
def test_eps_on_a_distance_and_just_below(ctx, c):
    s = 128
    a = 1000 + 10 * np.arange(s)
    b = np.concatenate([a[:c], a[c:] + 5])  # the c lowest shared, the rest interleaved
    assert M.mash_counts(a.tolist(), b.tolist(), s) == (c, s)
    eps = M.distance(c, s, K)
    sk = _set(ctx, [a, b])
    assert ctx.dbscan_mash(sk, s, [eps], 1, K)[0].tolist() == [0, 0]
    assert ctx.dbscan_mash(sk, s, [float(np.nextafter(eps, 0))], 1, K)[0].tolist() == [-1, -1]
    both = ctx.dbscan_mash(sk, s, [float(np.nextafter(eps, 0)), eps], 1, K)
    assert both.tolist() == [[-1, -1], [0, 0]]


# ---- (f) the sweep ------------------------------------------------------------------------------------------------
def test_32_levels_equal_32_calls(ctx, oracle):
    sk, host, dist = _families(ctx, oracle, 1)
    rng = np.random.default_rng(2)
    eps = [0.0, 0.001, 0.004, 0.01, 0.02, 0.03, 0.05, 0.08, 0.12, 0.5, 0.999]
    eps = [eps[i] for i in rng.integers(0, len(eps), 32)]
    assert len(set(eps)) >= 8 and eps != sorted(eps)
    got, core = ctx.dbscan_mash(sk, 128, eps, 3, K, return_core=True)
    assert ctx.dbscan_mash_counters()["levels"] == 32
    singles = {}
    for e, x in enumerate(eps):
        if x not in singles:
            singles[x] = ctx.dbscan_mash(sk, 128, [x], 3, K, return_core=True)
            want, want_core = M.labels_of(dist, x, 3)
            assert np.array_equal(singles[x][0][0], want) and np.array_equal(singles[x][1][0], want_core), x
        assert np.array_equal(got[e], singles[x][0][0]) and np.array_equal(core[e], singles[x][1][0]), (e, x)
    assert len({tuple(r.tolist()) for r in got}) >= 5
    from rabbittclust_amd import api
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan_mash(sk, 128, eps + [0.2], 3, K)
    assert ei.value.status == api._lib.RTC_ERR_ARG
    with pytest.raises(api.RtcError):
        ctx.dbscan_mash(sk, 128, [], 3, K)


# ---- (g) row chunks, (h) the prefilter --------------------------------------------------------------------------
def _dense_candidates(n=600):
    """every sketch shares one hash with every other (the candidate list is the whole triangle); seven families besides"""
    rng = np.random.default_rng(3)
    sets = []
    for g in range(n):
        body = (100_000 * (g % 7) + np.arange(60))[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, 10_000_000 + 1000 * g + np.arange(5)])))
    return sets


def test_row_chunks_and_prefilter(ctx):
    sets = _dense_candidates()
    n, s = len(sets), 80
    sk = _set(ctx, sets)
    eps = [0.005, 0.02]
    want, want_core = ctx.dbscan_mash(sk, s, eps, 4, K, return_core=True)
    c1 = ctx.dbscan_mash_counters()
    assert c1["chunks"] == 1 and c1["candidate_edges"] == n * (n - 1) // 2
    assert 0 < c1["kept_edges"] <= c1["merged"] < c1["candidate_edges"]  # most pairs share the one hash alone
    assert len(set(want[1].tolist())) == 7 and not np.array_equal(want[0], want[1])
    # a sample of the points against the restatement: rows of the distance matrix are enough for the degrees
    for p in (0, 1, 7, 300, 599):
        d = [M.distance(*M.mash_counts(sets[p].tolist(), sets[q].tolist(), s), K) if q != p else 9.0 for q in range(n)]
        for e, x in enumerate(eps):
            assert want_core[e][p] == (sum(v <= x for v in d) >= 4), (p, x)
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        got, core = ctx.dbscan_mash(sk, s, eps, 4, K, return_core=True)
        c2 = ctx.dbscan_mash_counters()
    assert np.array_equal(got, want) and np.array_equal(core, want_core)
    assert c2["chunks"] > 2 and all(c2[k] == c1[k] for k in ("candidate_edges", "merged", "kept_edges"))
    for serial in (None, "1"):
        with ctx.env(RTC_DBSCAN_MASH_NOPREFILTER="1", RTC_DBSCAN_MASH_SERIAL=serial):
            got, core = ctx.dbscan_mash(sk, s, eps, 4, K, return_core=True)
            c3 = ctx.dbscan_mash_counters()
        assert np.array_equal(got, want) and np.array_equal(core, want_core)
        assert c3["merged"] == c3["candidate_edges"] == c1["candidate_edges"] and c3["kept_edges"] == c1["kept_edges"]
    with ctx.env(RTC_DBSCAN_MASH_SERIAL="1"):
        got = ctx.dbscan_mash(sk, s, eps, 4, K)
    assert np.array_equal(got, want) and ctx.dbscan_mash_counters()["merged"] == c1["merged"]


# ---- (i) error returns ----------------------------------------------------------------------------------------
def test_error_returns_and_tiny_sets(ctx):
    from rabbittclust_amd import api
    sk = _set(ctx, [np.arange(10), np.arange(5, 15)])
    for eps, status in ((1.0, api._lib.RTC_ERR_UNSUPPORTED), (1.5, api._lib.RTC_ERR_UNSUPPORTED), (-0.1, api._lib.RTC_ERR_ARG),
                        (float("nan"), api._lib.RTC_ERR_ARG)):
        with pytest.raises(api.RtcError) as ei:
            ctx.dbscan_mash(sk, 10, [0.01, eps], 1, K)
        assert ei.value.status == status, eps
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan_mash(sk, 0, [0.01], 1, K)
    assert ei.value.status == api._lib.RTC_ERR_ARG
    assert ctx.dbscan_mash(sk, 10, [0.999], 1, K)[0].tolist() == [0, 0]
    for host in ([], [np.arange(10)], [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.uint64)] * 3):
        for min_pts in (0, 1):  # empty sketches are plain points: distance 1 to everything
            got = ctx.dbscan_mash(_set(ctx, host), 10, [0.01, 0.5], min_pts, K)
            assert got.shape == (2, len(host))
            assert got.tolist() == [list(range(len(host))) if min_pts == 0 else [-1] * len(host)] * 2


# ---- (j) the command line ---------------------------------------------------------------------------------------
def _run(args, cwd, env=None):
    import subprocess
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def test_cli_end_to_end(oracle, tmp_path):
    tmp = str(tmp_path)
    # -k 19: inside what the tuner keeps for genomes of 500 kbp (17 to 20)
    L, s, eps, min_pts, k = 500_000, 128, 0.03, 2, 19
    lst, seqs, meta = _write_fastas(oracle, tmp, 6, 4, L, seed=11)
    assert len(seqs) == 24
    D = os.path.join(BIN, "clust-dbscan")
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * L
    host = oracle.sketch_minhash_batch(np.concatenate(seqs), off, k, s)
    dist = M.distance_matrix(M.count_matrix(host, s), k)
    want, _ = M.labels_of(dist, eps, min_pts)
    assert 1 < int(want.max()) + 1 < 24
    d1 = os.path.join(tmp, "l"); os.makedirs(d1)
    out, mj = os.path.join(tmp, "l.out"), os.path.join(tmp, "m.json")
    common = ["-k", str(k), "-s", str(s), "--eps", str(eps), "--minpts", str(min_pts), "-t", "4"]
    err = _run([D, "--minhash", "-l", "-i", lst] + common + ["-o", out], d1, env={"RTC_METRICS_JSON": mj})
    assert "-----the kmerSize is: %d\n" % k in err and "-----Running DBSCAN clustering (MinHash)..." in err and f"-----Found {int(want.max()) + 1} clusters\n" in err
    assert open(out).read() == M.print_result(want, meta, True, eps, min_pts)
    metrics = json.load(open(mj))
    assert metrics["command"] == "clust-dbscan" and metrics["sketch"] == "minhash"
    for key in ("dbscan_s", "dbscan_mash_pair_s", "dbscan_mash_predicate_s", "dbscan_mash_components_s"):
        assert key in metrics and metrics[key] >= 0, key
    # the folder clust-mst writes for the same genomes: the same sketch files, and the same result from it
    d2 = os.path.join(tmp, "m"); os.makedirs(d2)
    _run([os.path.join(BIN, "clust-mst"), "-l", "-i", lst, "-k", str(k), "-s", str(s), "-t", "4", "-o", os.path.join(tmp, "mst.out")], d2)
    f1, f2 = _folders(d1), _folders(d2)
    assert len(f1) == 1 and len(f2) == 1
    for name in ("hash.sketch", "info.sketch", "minhash.sketch.index"):
        assert open(os.path.join(f1[0], name), "rb").read() == open(os.path.join(f2[0], name), "rb").read(), name
    out2 = os.path.join(tmp, "p.out")
    err2 = _run([D, "--minhash", "--presketched", f2[0], "-l", "--eps", str(eps), "--minpts", str(min_pts), "-o", out2], tmp)
    assert open(out2, "rb").read() == open(out, "rb").read() and "sketch format mismatch" not in err2
    # --eps-sweep: every file equals the single run at that eps
    out3 = os.path.join(tmp, "s.out")
    _run([D, "--minhash", "--presketched", f1[0], "-l", "--eps", str(eps), "--minpts", str(min_pts), "--eps-sweep", "0.01,0.06", "-o", out3], tmp)
    assert open(out3, "rb").read() == open(out, "rb").read()
    rows = open(out3 + ".eps_sweep.tsv").read().splitlines()
    assert rows[0].split("\t")[:3] == ["eps", "clusters", "noise"] and len(rows) == 3
    for x, row in zip((0.01, 0.06), rows[1:]):
        single = os.path.join(tmp, "one_%g.out" % x)
        _run_plain([D, "--minhash", "--presketched", f1[0], "-l", "--eps", str(x), "--minpts", str(min_pts), "-o", single], tmp)
        assert open(out3 + ".eps_%.6f" % x, "rb").read() == open(single, "rb").read()
        wx, wc = M.labels_of(dist, x, min_pts)
        assert open(single).read() == M.print_result(wx, meta, True, x, min_pts)
        assert row.split("\t")[:4] == ["%.6f" % x, str(int(wx.max(initial=-1)) + 1), str(int((wx < 0).sum())), str(int(wc.sum()))]
