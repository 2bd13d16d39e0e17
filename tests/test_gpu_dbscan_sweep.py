"""clust-dbscan --eps-sweep / --kdist on the GPU (rtc_dbscan_sweep): every level bit-identical to the restated KssdDBSCAN
(tests/refdbscan.py) and to Context.dbscan at that eps, the k-distance curve identical to its exact restatement
(tests/refkdist.py), one pair phase by the counters, and the command line end to end.  No tolerances."""
import os

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refkdist as KD
from tests import sweep_sets as S
from tests.test_gpu_dbscan import BIN, _folders, _run, _write_fastas

pytestmark = pytest.mark.gpu

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))


def _set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=S.KMER, kind="kssd", width=width)


def _expected(host, eps_list, min_pts, use64, max_posting=0):
    labs, cores = [], []
    for eps in eps_list:
        nb = R.neighbour_lists(host, eps, S.KMER, use64, max_posting)
        labs.append(R.labels_of(host, eps, min_pts, S.KMER, use64, max_posting))
        cores.append(np.array([len(x) + 1 >= min_pts for x in nb], dtype=bool))
    return labs, cores


def _check_sweep(ctx, sk, host, eps_list, min_pts, max_posting=0, want=None):
    """rows of dbscan_sweep == the reference walk == Context.dbscan, labels, core flags and counts"""
    use64 = sk.width == 8
    labs, cores = want if want is not None else _expected(host, eps_list, min_pts, use64, max_posting)
    got, core = ctx.dbscan_sweep(sk, eps_list, min_pts, S.KMER, max_posting=max_posting, return_core=True)
    counts = ctx.dbscan_sweep_counts
    c = ctx.dbscan_sweep_counters()
    assert got.shape == (len(eps_list), sk.n) and core.shape == got.shape and c["levels"] == len(eps_list)
    for e, eps in enumerate(eps_list):
        assert np.array_equal(got[e], labs[e]), (eps, min_pts, got[e].tolist(), labs[e].tolist())
        assert np.array_equal(core[e], cores[e]), (eps, min_pts)
        one, one_core = ctx.dbscan(sk, eps, min_pts, S.KMER, max_posting=max_posting, return_core=True)
        assert np.array_equal(got[e], one) and np.array_equal(core[e], one_core), (eps, min_pts)
        assert counts["clusters"][e] == int(one.max(initial=-1)) + 1 and counts["noise"][e] == int((one < 0).sum())
    return got, core, c


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("width,max_posting", [(4, 0), (4, 5), (8, 0), (8, 5)])
def test_every_level_matches_the_walk_and_the_single_call(ctx, seed, width, max_posting):
    # (max_posting at width 8: the brute force of the u64 path has no posting lists, the argument must change nothing)
    use64 = width == 8
    host = S.family_sets(seed, use64)
    sk = _set(ctx, host, width)
    for min_pts in (1, 2, 5):
        want = _expected(host, S.EPS, min_pts, use64, max_posting)
        # before the GPU is asked: the levels differ, or the test could pass with all levels alike.  Noise needs minPts >= 2
        # (at minPts 1 every point is a core point), a border point minPts >= 3 (with one neighbour a point is core at 2).
        distinct, noise, border = S.describe(*want)
        assert distinct >= 3 and noise == (min_pts >= 2) and border == (min_pts >= 3), (distinct, noise, border)
        _check_sweep(ctx, sk, host, S.EPS, min_pts, max_posting, want)


def test_list_orders_duplicates_and_lengths(ctx):
    host = S.family_sets(7, False)
    sk = _set(ctx, host, 4)
    rng = np.random.default_rng(5)
    shuffled = [S.EPS[i] for i in rng.permutation(len(S.EPS))]
    dup = [0.02, 0.06, 0.02, 0.002, 0.06]
    full = [0.001 + 0.004 * i for i in range(32)]
    for eps_list in (sorted(S.EPS, reverse=True), shuffled, dup, [0.04], full):
        got, _, _ = _check_sweep(ctx, sk, host, eps_list, 5)
    assert len({tuple(r.tolist()) for r in got}) >= 3  # the 32 levels are not all alike
    from rabbittclust_amd import api
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan_sweep(sk, full + [0.2], 5, S.KMER)
    assert ei.value.status == api._lib.RTC_ERR_ARG
    with pytest.raises(api.RtcError):
        ctx.dbscan_sweep(sk, [], 5, S.KMER)  # nothing asked for


@pytest.mark.parametrize("width", [4, 8])
def test_tiny_and_empty_sets(ctx, width):
    dt = np.uint32 if width == 4 else np.uint64
    for host in ([], [np.arange(10, dtype=dt)], [np.zeros(0, dtype=dt)]):
        sk = _set(ctx, host, width)
        for min_pts in (1, 2):
            got, curve = ctx.dbscan_sweep(sk, [0.01, 0.05], min_pts, S.KMER, kdist=True)
            assert got.shape == (2, len(host)) and curve.shape == (len(host),)
            if host:
                assert got[:, 0].tolist() == ([0, 0] if min_pts == 1 else [-1, -1])
                assert got[0].tolist() == ctx.dbscan(sk, 0.01, min_pts, S.KMER).tolist()
                want = KD.kdist(host, min_pts, width == 8)[0]
                assert tuple(int(curve[0][f]) for f in ("common", "size_p", "size_q", "neighbour")) == want


@pytest.mark.parametrize("width", [4, 8])
def test_sets_with_empty_sketches(ctx, width):
    use64 = width == 8
    host = S.family_sets(3, use64, n_empty=3)
    sk = _set(ctx, host, width)
    for min_pts in (1, 2, 3, 4, 5):
        got, _, _ = _check_sweep(ctx, sk, host, S.EPS, min_pts)
    empty = [g for g, s in enumerate(host) if len(s) == 0]
    lab3 = ctx.dbscan_sweep(sk, S.EPS, 3, S.KMER)
    if use64:  # the brute force's clique of empty sketches: one cluster at every eps while minPts <= their number
        assert all(len({int(lab3[e][g]) for g in empty}) == 1 and lab3[e][empty[0]] >= 0 for e in range(len(S.EPS)))
    else:
        assert all((lab3[e][empty] == -1).all() for e in range(len(S.EPS)))


@pytest.mark.parametrize("width", [4, 8])
def test_each_call_fills_its_own_counters_and_no_others(ctx, width):
    """dbscan, dbscan_sweep and dbscan_hierarchy run one implementation and keep three counter sets: a call fills its own and
    leaves the other two exactly as they were, times included (width 8: with the clique of empty sketches in play)"""
    host = S.family_sets(3, width == 8, n_empty=3)
    sk = _set(ctx, host, width)
    eps, min_pts = 0.04, 3
    sets = {"dbscan": ctx.dbscan_counters, "sweep": ctx.dbscan_sweep_counters, "hierarchy": ctx.dbscan_hierarchy_counters}

    def others_untouched(own, call):
        before = {k: f() for k, f in sets.items() if k != own}
        out = call()
        assert {k: f() for k, f in sets.items() if k != own} == before, own
        return out, sets[own]()

    (lab, core), first = others_untouched("dbscan", lambda: ctx.dbscan(sk, eps, min_pts, S.KMER, return_core=True))
    _, sweep = others_untouched("sweep", lambda: ctx.dbscan_sweep(sk, S.EPS, min_pts, S.KMER))
    (forest, _), hier = others_untouched("hierarchy", lambda: ctx.dbscan_hierarchy(sk, max(S.EPS), min_pts, S.KMER))
    (lab2, core2), second = others_untouched("dbscan", lambda: ctx.dbscan(sk, eps, min_pts, S.KMER, return_core=True))
    assert np.array_equal(lab, lab2) and np.array_equal(core, core2)
    assert {k: v for k, v in first.items() if not k.endswith("_ns")} == {k: v for k, v in second.items() if not k.endswith("_ns")}
    assert sweep["levels"] == len(S.EPS) and sweep["chunks"] == first["chunks"] == hier["chunks"] >= 1
    assert sweep["candidate_edges"] == first["candidate_edges"] == hier["candidate_edges"] > 0
    assert hier["forest_edges"] == len(forest) > 0
    ctx.dbscan_sweep(sk, [eps], min_pts, S.KMER)
    assert first["eps_edges"] == ctx.dbscan_sweep_counters()["kept_edges"] > 0
    assert first["core_points"] == int(core.sum()) > 0 and first["asymmetric_pairs"] == 0 and first["hook_rounds"] >= 1
    assert all(first[k] > 0 for k in first if k.endswith("_ns"))


def test_one_unsupported_level_fails_the_sweep_and_names_its_eps(ctx):
    from rabbittclust_amd import api
    host = S.family_sets(2, False)
    sk = _set(ctx, host, 4)
    bad = 1.5  # exp(-1.5 * 21) / 2 ~ 1e-14: jaccard_min <= 1e-12, which rtc_dbscan refuses
    assert R.jaccard_min(bad, S.KMER) <= 1e-12 < R.jaccard_min(0.12, S.KMER)
    with pytest.raises(api.RtcError) as single:
        ctx.dbscan(sk, bad, 5, S.KMER)
    assert single.value.status == api._lib.RTC_ERR_UNSUPPORTED
    msg = str(single.value).split(": ", 1)[1]  # the single call names itself and no place in a list
    assert msg.startswith("rtc_dbscan: eps 1.5 with k %d gives jaccard_min " % S.KMER) and "of the list" not in msg
    for width in (4, 8):
        s = _set(ctx, S.family_sets(2, width == 8), width)
        with pytest.raises(api.RtcError) as ei:
            ctx.dbscan_sweep(s, [0.02, bad, 0.04], 5, S.KMER)
        assert ei.value.status == api._lib.RTC_ERR_UNSUPPORTED
        assert "eps 1.5" in str(ei.value) and "jaccard_min" in str(ei.value)
    # the context is fine afterwards
    _check_sweep(ctx, sk, host, [0.02, 0.04], 5)


def _check_kdist(ctx, sk, host, min_pts, max_posting=0, eps_list=()):
    out = ctx.dbscan_sweep(sk, list(eps_list), min_pts, S.KMER, max_posting=max_posting, kdist=True)
    curve = out[-1]
    want = KD.kdist(host, min_pts, sk.width == 8, max_posting)
    got = [tuple(int(r[f]) for f in ("common", "size_p", "size_q", "neighbour")) for r in curve]
    assert got == want, [(p, g, w) for p, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    for r, w in zip(curve, want):
        d = float("inf") if w[3] == KD.NONE else KD.distance(w[0], w[1], w[2], S.KMER)
        assert r["distance"] == d
    return curve, want


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_kdist_equals_the_exact_restatement(ctx, seed):
    for width, n_empty, max_posting in ((4, 0, 0), (4, 2, 5), (8, 3, 0)):
        host = S.family_sets(seed, width == 8, n_empty)
        sk = _set(ctx, host, width)
        saw_none = saw_some = False
        for min_pts in (0, 1, 2, 3, 5, 9):  # k = -1, 0, 1, 2, 4, 8
            _, want = _check_kdist(ctx, sk, host, min_pts, max_posting, eps_list=S.EPS if min_pts == 5 else ())
            saw_none |= any(w[3] == KD.NONE for w in want)
            saw_some |= any(w[3] != KD.NONE for w in want)
        assert saw_none and saw_some  # points with fewer than k candidates, and points with a k-th one


def test_kdist_ties_go_to_the_lower_index(ctx):
    a = np.arange(1, 101, dtype=np.uint32)
    twin = np.concatenate([a[:80], np.arange(1000, 1020, dtype=np.uint32)])
    host = [twin.copy(), a, twin.copy(), np.concatenate([a[:80], np.arange(2000, 2020, dtype=np.uint32)]), a.copy()]
    sk = _set(ctx, host, 4)
    for min_pts in (2, 3, 4, 5, 6):
        _, want = _check_kdist(ctx, sk, host, min_pts)
    assert KD.kdist(host, 2, False)[1] == (100, 100, 100, 4) and KD.kdist(host, 3, False)[1] == (80, 100, 100, 0)
    assert KD.kdist(host, 4, False)[1] == (80, 100, 100, 2)


def _shared_hash_set(n, rng):
    # every sketch shares hash 1 with every other: each point has n - 1 candidates, the candidate list is the whole triangle
    sets = []
    for g in range(n):
        body = np.arange(100_000 * (g % 7), 100_000 * (g % 7) + 60, dtype=np.int64)[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, np.arange(10_000_000 + 1000 * g, 10_000_000 + 1000 * g + 5)])).astype(np.uint32))
    return sets


def test_kdist_past_256_takes_the_host_selection(ctx):
    host = _shared_hash_set(300, np.random.default_rng(11)) + [np.arange(5_000_000, 5_000_040, dtype=np.uint32)] * 2
    sk = _set(ctx, host, 4)
    for min_pts in (257, 258, 290, 301):  # k = 256: the last one on the device; 257, 289: the host; 300: nobody has that many
        _, want = _check_kdist(ctx, sk, host, min_pts)
        assert want[-1][3] == KD.NONE and (want[0][3] != KD.NONE) == (min_pts <= 300)


def test_kdist_of_a_long_candidate_segment(ctx):
    # one hub shares a private hash with each of 4 300 others: its segment is past the one-wave selection's 4 096 records
    n = 4300
    host = [np.concatenate([[10 * g + 5], np.arange(1 << 30, (1 << 30) + 20 + g % 5) + 64 * (g // 10)]).astype(np.uint32) for g in range(n)]
    host.append(np.unique(np.array([10 * g + 5 for g in range(n)], dtype=np.uint32)))
    sk = _set(ctx, host, 4)
    for min_pts in (2, 6, 200):
        _, want = _check_kdist(ctx, sk, host, min_pts)
    assert want[n][3] != KD.NONE and want[n][1] == n


def test_row_chunks_one_pair_phase_and_the_running_top_k(ctx):
    n = 600
    host = _shared_hash_set(n, np.random.default_rng(3))
    sk = _set(ctx, host, 4)
    eps_list = [0.02, 0.1, 0.3]
    want = _expected(host, eps_list, 4, False)
    ctx.dbscan(sk, 0.1, 4, S.KMER)
    single = ctx.dbscan_counters()
    _, _, c1 = _check_sweep(ctx, sk, host, eps_list, 4, want=want)
    # _check_sweep's last call was a Context.dbscan: ask the sweep's own counters again from a fresh sweep
    ctx.dbscan_sweep(sk, eps_list, 4, S.KMER)
    c1 = ctx.dbscan_sweep_counters()
    assert c1["chunks"] == single["chunks"] == 1 and c1["candidate_edges"] == single["candidate_edges"] == n * (n - 1) // 2
    assert single["eps_edges"] <= c1["kept_edges"] <= c1["candidate_edges"] and c1["hook_rounds"] >= 1
    curve1, _ = _check_kdist(ctx, sk, host, 6, eps_list=eps_list)
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        ctx.dbscan(sk, 0.1, 4, S.KMER)
        single2 = ctx.dbscan_counters()
        _check_sweep(ctx, sk, host, eps_list, 4, want=want)
        curve2, _ = _check_kdist(ctx, sk, host, 6, eps_list=eps_list)
        c2 = ctx.dbscan_sweep_counters()
        _check_kdist(ctx, sk, host, 400)  # the host selection over several chunks
    assert single2["chunks"] > 2 and c2["chunks"] == single2["chunks"] and c2["candidate_edges"] == c1["candidate_edges"]
    assert c2["kept_edges"] == c1["kept_edges"] and np.array_equal(curve1, curve2)


def _cli_files(out, eps_list):
    return {e: open(out + ".eps_%.6f" % e).read() for e in eps_list}


def test_cli_sweep_and_kdist(ctx, oracle, tmp_path):
    tmp = str(tmp_path)
    L = 1_000_000
    lst, seqs, meta = _write_fastas(oracle, tmp, 4, 4, L, seed=9)
    D = os.path.join(BIN, "clust-dbscan")
    sweep = [0.01, 0.05, 0.002]
    common = ["--eps", "0.03", "--minpts", "3"]
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]

    def runs(src, kmer, tag):
        """base run, sweep run, one separate run per sweep value; returns the sweep run's -o path"""
        d = os.path.join(tmp, tag); os.makedirs(d)
        base, sw = os.path.join(d, "base.out"), os.path.join(d, "sw.out")
        _run([D, "--fast"] + src + common + ["-o", base], d)
        _run([D, "--fast"] + src + common + ["-o", sw, "--eps-sweep", ",".join("%g" % e for e in sweep), "--kdist"], d)
        assert open(sw, "rb").read() == open(base, "rb").read()
        assert open(sw).read() == R.print_result(R.labels_of(ks, 0.03, 3, kmer, False), meta, True, 0.03, 3)
        files = _cli_files(sw, sweep)
        for e in sweep:
            sep = os.path.join(d, "sep_%g.out" % e)
            _run([D, "--fast"] + src + ["--eps", "%g" % e, "--minpts", "3", "-o", sep], d)
            assert files[e] == open(sep).read(), e
        return d, sw, files

    d1, sw1, _ = runs(["-l", "-i", lst, "-k", "17", "-t", "4"], 17, "genomes")
    folder = _folders(d1)[0]
    _, sw2, files = runs(["--presketched", folder, "-l", "-k", "17"], 18, "presketched")
    # the tables against the per-eps files and the API (from the sketch folder k is half_k * 2 = 18)
    from rabbittclust_amd import api
    sk = api.SketchSet.from_host(ks, ctx.device, k=18, kind="kssd", width=4)
    labs, cores, curve = ctx.dbscan_sweep(sk, sweep, 3, 18, return_core=True, kdist=True)
    rows = [r.split("\t") for r in open(sw2 + ".eps_sweep.tsv").read().splitlines()]
    assert rows[0] == ["eps", "clusters", "noise", "core_points", "largest_cluster", "border_points"] and len(rows) == 1 + len(sweep)
    for e, (eps, row) in enumerate(zip(sweep, rows[1:])):
        lab, core = labs[e], cores[e]
        ncl, noise = int(lab.max(initial=-1)) + 1, int((lab < 0).sum())
        largest = int(np.bincount(lab[lab >= 0]).max()) if ncl else 0
        assert row == ["%.6f" % eps, str(ncl), str(noise), str(int(core.sum())), str(largest), str(int(((lab >= 0) & ~core).sum()))]
        head = files[eps].splitlines()
        assert head[0] == "# DBSCAN clustering parameters: eps=%.6f, minPts=3" % eps and head[1] == "# Total clusters: %d" % ncl
        assert (head[2] == "# Total noise points (outliers): %d" % noise) if noise else head[2] == "#"
    assert len({tuple(x.tolist()) for x in labs}) >= 2
    krows = [r.split("\t") for r in open(sw2 + ".kdist.tsv").read().splitlines()]
    assert krows[0] == ["index", "kth_neighbour", "common", "size", "size_neighbour", "distance"] and len(krows) == 1 + len(ks)
    order = sorted(range(len(ks)), key=lambda p: (-curve[p]["distance"], p))
    for p, row in zip(order, krows[1:]):
        r = curve[p]
        if r["neighbour"] == api.KDIST_NONE:
            assert row == [str(p), "-1", "0", str(int(r["size_p"])), "0", "inf"]
        else:
            assert row == [str(p), str(int(r["neighbour"])), str(int(r["common"])), str(int(r["size_p"])), str(int(r["size_q"])),
                           "%.10g" % r["distance"]]
    want = KD.kdist(ks, 3, False)
    assert [tuple(int(r[f]) for f in ("common", "size_p", "size_q", "neighbour")) for r in curve] == want
