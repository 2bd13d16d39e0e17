"""clust-dbscan --hierarchy on the GPU (rtc_dbscan_hierarchy): the forest and the core triples bit-identical to the plain-Python
restatement (tests/refhier.py), the core triples equal to rtc_dbscan_sweep's k-distance curve, rtc_hierarchy_cut equal to
rtc_dbscan on the core points at many eps (the link to the reference-pinned path), the flat clustering equal to the
restatement's, and the command line end to end.  No tolerances."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refhier as RH
from tests import refkdist as KD
from tests import sweep_sets as S
from tests.test_gpu_dbscan import BIN, _folders, _write_fastas

pytestmark = pytest.mark.gpu

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))
EPS_MAX = 0.12
EPS_CUTS = [0.002, 0.005, 0.008, 0.011, 0.014, 0.02, 0.025, 0.03, 0.04, 0.05, 0.06, 0.08, 0.1, 0.12]


def _set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=S.KMER, kind="kssd", width=width)


def _tuples(a, fields):
    return [tuple(int(r[f]) for f in fields) for r in a]


def _check_hierarchy(ctx, sk, host, min_pts, max_posting=0, eps_max=EPS_MAX):
    """(a) forest and core triples == the restatement, (b) core triples == the sweep's curve"""
    from rabbittclust_amd import api
    forest, core = ctx.dbscan_hierarchy(sk, eps_max, min_pts, S.KMER, max_posting=max_posting)
    c = ctx.dbscan_hierarchy_counters()
    want_f, want_c = RH.hierarchy(host, eps_max, min_pts, S.KMER, sk.width == 8, max_posting)
    got_f, got_c = _tuples(forest, api.HEDGE_DT.names), _tuples(core, api.KDIST_DT.names)
    assert got_c == want_c, [(p, g, w) for p, (g, w) in enumerate(zip(got_c, want_c)) if g != w][:5]
    assert got_f == want_f, (len(got_f), len(want_f), [(i, g, w) for i, (g, w) in enumerate(zip(got_f, want_f)) if g != w][:5])
    assert c["forest_edges"] == len(want_f)
    curve = ctx.dbscan_sweep(sk, [], min_pts, S.KMER, max_posting=max_posting, kdist=True)[-1]
    assert _tuples(curve, api.KDIST_DT.names) == got_c
    return forest, core, c


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("width,n_empty,max_posting", [(4, 0, 0), (4, 2, 5), (8, 3, 0), (8, 0, 5)])
def test_forest_and_core_equal_the_restatement(ctx, seed, width, n_empty, max_posting):
    host = S.family_sets(seed, width == 8, n_empty)
    sk = _set(ctx, host, width)
    saw_none = saw_edges = False
    for min_pts in (0, 1, 2, 5, 9, 40):  # k = -1, 0: every point its own k-th; k = 39: past every point's candidates
        forest, core, c = _check_hierarchy(ctx, sk, host, min_pts, max_posting)
        saw_none |= bool((core["neighbour"] == KD.NONE).any())
        saw_edges |= len(forest) > 10
        assert c["kept_edges"] <= c["candidate_edges"] and c["chunks"] >= 1
        if len(forest):
            assert c["boruvka_rounds"] >= 1
    assert saw_none and saw_edges
    _check_hierarchy(ctx, sk, host, 5, max_posting, eps_max=0.02)  # a lower ceiling keeps fewer pairs


def test_ties_follow_the_total_order(ctx):
    a = np.arange(1, 101, dtype=np.uint32)
    twin = np.concatenate([a[:80], np.arange(1000, 1020, dtype=np.uint32)])
    host = [twin.copy(), a, twin.copy(), np.concatenate([a[:80], np.arange(2000, 2020, dtype=np.uint32)]), a.copy(), a.copy()]
    for width in (4, 8):
        sk = _set(ctx, host, width)
        for min_pts in (1, 2, 3, 4, 6):
            _check_hierarchy(ctx, sk, host, min_pts)


@pytest.mark.parametrize("width", [4, 8])
def test_tiny_and_empty_sets(ctx, width):
    dt = np.uint32 if width == 4 else np.uint64
    for host in ([], [np.arange(10, dtype=dt)], [np.zeros(0, dtype=dt)], [np.zeros(0, dtype=dt)] * 3, [np.arange(10, dtype=dt)] * 2):
        sk = _set(ctx, host, width)
        for min_pts in (1, 2, 3):
            _check_hierarchy(ctx, sk, host, min_pts)


def _shared_hash_set(n, rng):
    # every sketch shares hash 1 with every other: the candidate list is the whole triangle
    sets = []
    for g in range(n):
        body = np.arange(100_000 * (g % 7), 100_000 * (g % 7) + 60, dtype=np.int64)[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, np.arange(10_000_000 + 1000 * g, 10_000_000 + 1000 * g + 5)])).astype(np.uint32))
    return sets


def test_row_chunks_give_the_same_forest(ctx):
    n = 600
    host = _shared_hash_set(n, np.random.default_rng(3))
    sk = _set(ctx, host, 4)
    f1, c1, k1 = _check_hierarchy(ctx, sk, host, 6, eps_max=0.3)
    assert k1["chunks"] == 1 and k1["candidate_edges"] == n * (n - 1) // 2 and len(f1) > n // 2
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        f2, c2, k2 = _check_hierarchy(ctx, sk, host, 6, eps_max=0.3)
        f3, c3, _ = _check_hierarchy(ctx, sk, host, 400, eps_max=0.3)  # k past 256: the host selection over several chunks
    assert k2["chunks"] > 2 and k2["candidate_edges"] == k1["candidate_edges"] and k2["kept_edges"] == k1["kept_edges"]
    assert np.array_equal(f1, f2) and np.array_equal(c1, c2)


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("width,n_empty,max_posting", [(4, 2, 0), (4, 0, 5), (8, 3, 0)])
def test_cut_equals_dbscan_on_the_core_points(ctx, seed, width, n_empty, max_posting):
    from rabbittclust_amd import api
    use64 = width == 8
    host = S.family_sets(seed, use64, n_empty)
    sk = _set(ctx, host, width)
    sizes = [len(s) for s in host]
    pair_js = [float(KD.jaccard(c, sizes[p], sizes[q])) for (p, q), c in RH.kept_pairs(host, EPS_MAX, S.KMER, use64, max_posting).items()]
    for min_pts in (1, 2, 5):
        forest, core = ctx.dbscan_hierarchy(sk, EPS_MAX, min_pts, S.KMER, max_posting=max_posting)
        ft, ct = _tuples(forest, api.HEDGE_DT.names), _tuples(core, api.KDIST_DT.names)
        # the condition for exact order <=> double predicate: no j within 1e-9 of t(eps)
        cuts = [e for e in EPS_CUTS if RH.min_margin(ft, ct, [e], S.KMER) > 1e-9
                and all(abs(j - R.jaccard_min(e, S.KMER)) > 1e-9 for j in pair_js)]
        assert len(cuts) >= 8
        distinct = set()
        for eps in cuts:
            lab, is_core = api.hierarchy_cut(forest, core, EPS_MAX, eps, S.KMER)
            one, one_core = ctx.dbscan(sk, eps, min_pts, S.KMER, max_posting=max_posting, return_core=True)
            assert np.array_equal(is_core, one_core), (eps, min_pts)
            assert np.array_equal(lab[is_core], one[one_core]), (eps, min_pts)
            assert (lab[~is_core] == -1).all()
            distinct.add(tuple(lab.tolist()))
        assert len(distinct) >= 3 or min_pts == 1
    with pytest.raises(api.RtcError):
        api.hierarchy_cut(forest, core, EPS_MAX, 0.13, S.KMER)


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_flat_equals_the_restatement(ctx, seed):
    from rabbittclust_amd import api
    clusters = 0
    for width in (4, 8):
        host = RH.nested_sets(seed, width == 8)  # sub-families inside super-families: the condensed tree has true splits
        sk = _set(ctx, host, width)
        for min_pts, mcs in [(2, 3), (3, 4), (5, 5)]:
            forest, core = ctx.dbscan_hierarchy(sk, EPS_MAX, min_pts, S.KMER)
            ft, ct = _tuples(forest, api.HEDGE_DT.names), _tuples(core, api.KDIST_DT.names)
            want, want_stab, gap = RH.flat(len(host), ft, ct, S.KMER, mcs)
            assert gap > 1e-9, gap  # the condition: no two compared stabilities within 1e-9 relative of each other
            got, stab = api.hierarchy_flat(forest, core, S.KMER, mcs, return_stability=True)
            assert got.tolist() == want, (width, min_pts, mcs)
            assert stab.tolist() == want_stab  # the same terms summed in the same order with the same libm
            clusters = max(clusters, len(want_stab))
    assert clusters == 5  # the five sub-families, chosen over the two super-families


@pytest.mark.parametrize("width", [4, 8])
def test_combined_call_equals_the_two_calls_with_one_pair_phase(ctx, width):
    host = S.family_sets(2, width == 8, 2)
    sk = _set(ctx, host, width)
    labs, flags = ctx.dbscan_sweep(sk, S.EPS, 5, S.KMER, return_core=True)
    sweep_alone = ctx.dbscan_sweep_counters()
    forest, core = ctx.dbscan_hierarchy(sk, EPS_MAX, 5, S.KMER)
    assert ctx.dbscan_sweep_counters() == sweep_alone  # a hierarchy call leaves the last sweep's counters alone
    got = ctx.dbscan_sweep_hierarchy(sk, S.EPS, EPS_MAX, 5, S.KMER)
    assert np.array_equal(got[0], labs) and np.array_equal(got[1], flags) and np.array_equal(got[2], forest) and np.array_equal(got[3], core)
    sc, hc = ctx.dbscan_sweep_counters(), ctx.dbscan_hierarchy_counters()
    assert sc["chunks"] == hc["chunks"] >= 1 and sc["candidate_edges"] == hc["candidate_edges"] == sweep_alone["candidate_edges"]
    assert sc["pair_ns"] == hc["pair_ns"] > 0  # one measurement of one pair phase
    assert sc["kept_edges"] == sweep_alone["kept_edges"] and hc["forest_edges"] == len(forest)


def test_unsupported_eps_max_fails_and_names_it(ctx):
    from rabbittclust_amd import api
    host = S.family_sets(2, False)
    sk = _set(ctx, host, 4)
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan_hierarchy(sk, 1.5, 5, S.KMER)
    assert ei.value.status == api._lib.RTC_ERR_UNSUPPORTED and "jaccard_min" in str(ei.value) and "rtc_dbscan_hierarchy" in str(ei.value)
    _check_hierarchy(ctx, sk, host, 5)  # the context is fine afterwards


def _cli(args, cwd, env=None):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def test_cli_hierarchy(ctx, oracle, tmp_path):
    from rabbittclust_amd import api
    tmp = str(tmp_path)
    L = 1_000_000
    lst, seqs, meta = _write_fastas(oracle, tmp, 4, 4, L, seed=9)
    D = os.path.join(BIN, "clust-dbscan")
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]
    n = len(ks)
    common = ["--eps", "0.05", "--minpts", "3"]

    def check(src, kmer, tag, mcs):
        d = os.path.join(tmp, tag); os.makedirs(d)
        base, hi = os.path.join(d, "base.out"), os.path.join(d, "hi.out")
        _cli([D, "--fast"] + src + common + ["-o", base], d)
        _cli([D, "--fast"] + src + common + ["-o", hi, "--hierarchy"] + (["--min-cluster-size", str(mcs)] if mcs != 3 else []), d)
        assert open(hi, "rb").read() == open(base, "rb").read()
        assert not os.path.exists(base + ".hierarchy.tsv") and not os.path.exists(base + ".hdbscan")
        forest, core = RH.hierarchy(ks, 0.05, 3, kmer, False)
        rows = [r.split("\t") for r in open(hi + ".hierarchy.tsv").read().splitlines()]
        assert rows[0] == ["p", "q", "distance", "common", "size_p", "size_q"]
        assert rows[1:] == [[str(p), str(q), "%.6f" % RH.distance(c, a, b, kmer), str(c), str(a), str(b)] for p, q, c, a, b in forest]
        assert len(forest) >= 4
        crow = [r.split("\t") for r in open(hi + ".core.tsv").read().splitlines()]
        assert crow[0] == ["index", "core_distance"]
        assert crow[1:] == [[str(v), "inf" if t[3] == RH.NONE else "%.6f" % RH.distance(t[0], t[1], t[2], kmer)] for v, t in enumerate(core)]
        lab, _, gap = RH.flat(n, forest, core, kmer, mcs)
        assert gap > 1e-9
        text = R.print_result(lab, meta, True, 0.05, 3).split("\n", 1)
        head = "# HDBSCAN* flat clustering parameters: min_cluster_size=%d, minPts=3, eps_max=0.050000" % mcs
        assert open(hi + ".hdbscan").read() == head + "\n" + text[1]
        return d

    d1 = check(["-l", "-i", lst, "-k", "17", "-t", "4"], 17, "genomes", 3)
    folder = _folders(d1)[0]
    d2 = check(["--presketched", folder, "-l", "-k", "17"], 18, "presketched", 2)
    # with --eps-sweep and --kdist: one pair phase serves all three, and every file is what the separate runs write
    allf, mj = os.path.join(d2, "all.out"), os.path.join(d2, "all.json")
    err = _cli([D, "--fast", "--presketched", folder, "-l", "-k", "17"] + common + ["-o", allf, "--hierarchy", "--min-cluster-size", "2",
               "--eps-sweep", "0.01,0.002", "--kdist"], d2, env={"RTC_VERBOSE": "1", "RTC_METRICS_JSON": mj})
    hi = os.path.join(d2, "hi.out")
    for ext in ("", ".hierarchy.tsv", ".core.tsv", ".hdbscan"):
        assert open(allf + ext, "rb").read() == open(hi + ext, "rb").read(), ext
    assert os.path.exists(allf + ".eps_sweep.tsv") and os.path.exists(allf + ".kdist.tsv") and os.path.exists(allf + ".eps_0.010000")
    sw = re.search(r"\[sweep\] 3 levels: (\d+) candidate edges in (\d+) chunk", err)
    hr = re.search(r"\[hierarchy\] (\d+) candidate edges in (\d+) chunk", err)
    assert sw and hr and sw.groups() == hr.groups()
    m = json.load(open(mj))
    # one measurement of one pair phase: the very same nanoseconds in both counter sets
    assert m["dbscan_hierarchy_pair_s"] == m["dbscan_sweep_pair_s"] > 0
    assert m["dbscan_hierarchy_edges"] == len(RH.hierarchy(ks, 0.05, 3, 18, False)[0])
    assert m["dbscan_hierarchy_kdist_s"] >= 0 and m["dbscan_hierarchy_forest_s"] > 0
    # and the API's combined call counts its pair phase once in both counter sets
    sk = api.SketchSet.from_host(ks, ctx.device, k=18, kind="kssd", width=4)
    ctx.dbscan_hierarchy(sk, 0.05, 3, 18)
    hc = ctx.dbscan_hierarchy_counters()
    assert (str(hc["candidate_edges"]), str(hc["chunks"])) == hr.groups()
