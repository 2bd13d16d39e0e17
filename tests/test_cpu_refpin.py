"""The restatements the DBSCAN and post-processing kernels are tested against, held to the reference's own code:
tests/refdbscan.py (labels_of, print_result) against KssdDBSCAN + printKssdDBSCANResult, tests/refpost.py (tree_medoids,
dedup_candidates, select_k_reps) against build_dedup_candidates_per_cluster + select_k_reps_per_cluster_tree.  The
reference's results are the fixtures tests/golden/ref_dbscan.npz / ref_postprocess.npz (tests/golden/make_golden.py), whose
inputs tests/refpin_cases.py rebuilds; where oracle/_ref holds the reference libraries (a checkout beside the reference tree)
the reference also runs again, on the fixture's cases and on a seeded random sweep.  Every comparison is equality."""
import hashlib
import json
import os
import re
import warnings

import numpy as np
import pytest

from tests import refdbscan as R
from tests import reflib, refpin_cases as P
from tests import refpost as RP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(name):
    path = os.path.join(GOLD, name)
    if not os.path.exists(path):
        pytest.fail("tests/golden/%s is missing: run tests/golden/make_golden.py where the reference tree exists" % name)
    return np.load(path)


def _no_live(what):
    warnings.warn("oracle/_ref/%s is not built: the reference itself was not re-run, the fixture stands for it" % what)


def _cases(fx):
    return [tuple(c) for c in json.loads(str(fx["cases"]))]


def _labels(fx, i):
    return fx["labels_flat"][fx["labels_off"][i]:fx["labels_off"][i + 1]]


_nbrs = {}


def _restated(case):
    """refdbscan's labels and core count of a case (the neighbour lists are shared by the cases that differ in minPts only)"""
    gen, args, eps, min_pts, k, mp = case
    sk = P.sketches_of(gen, args)
    key = json.dumps([gen, args, eps, k, mp], sort_keys=True)
    if key not in _nbrs:
        _nbrs[key] = R.neighbour_lists(sk, eps, k, P.use64_of(sk), mp)
    lab, n_core = R.sequential_walk(_nbrs[key], min_pts)
    return np.array([x if x >= 0 else -1 for x in lab], dtype=np.int32), n_core


def test_dbscan_fixture_grid_is_what_the_generators_produce():
    fx = _fixture("ref_dbscan.npz")
    cases = P.dbscan_cases()
    assert [list(c) for c in cases] == json.loads(str(fx["cases"]))
    inputs = json.loads(str(fx["inputs"]))
    assert set(inputs) == {json.dumps([c[0], c[1]], sort_keys=True) for c in cases}
    for key, sha in inputs.items():
        gen, args = json.loads(key)
        assert P.input_sha(P.sketches_of(gen, args)) == sha, key
    # what the grid has to contain
    gens = {c[0] for c in cases}
    assert gens == set(P.GENERATORS)
    fam = [c for c in cases if c[0] == "family"]
    assert {c[3] for c in fam} >= {0, 1, 2, 100} and {c[5] for c in fam} == {0, 1, 5, 1000} and {c[1]["use64"] for c in fam} == {False, True}
    assert all(c[1]["n_empty"] == 2 and len(P.sketches_of(c[0], c[1])) == 34 for c in fam)
    assert max(len(s) for s in P.sketches_of("hub", {})) > 10_000


def test_dbscan_restatement_equals_the_reference_on_the_fixture():
    """labels_of, the core count and print_result's text against the reference's, on every case inside the bound the kernels
    accept; on the cases outside it, see test_u32_size_bound_is_where_reference_and_restatement_part"""
    fx = _fixture("ref_dbscan.npz")
    cases = _cases(fx)
    seen = set()
    compared = 0
    for i, case in enumerate(cases):
        gen, args, eps, min_pts, k, mp = case
        sk = P.sketches_of(gen, args)
        want = _labels(fx, i)
        assert len(want) == len(sk)
        assert int(fx["n_clusters"][i]) == int(want.max(initial=-1)) + 1 and int(fx["n_noise"][i]) == int((want < 0).sum())
        by_file = P.print_layout(i)
        text = R.print_result(want.tolist(), P.genomes_of(len(sk), by_file), by_file, eps, min_pts)
        assert hashlib.sha256(text.encode()).hexdigest() == str(fx["print_sha256"][i]), case
        if P.u32_bound_exceeded(sk, eps, k):
            continue
        got, n_core = _restated(case)
        assert np.array_equal(got, want), (case, got.tolist(), want.tolist())
        assert n_core == int(fx["n_core"][i]), case
        compared += 1
        nb = _nbrs[json.dumps([gen, args, eps, k, mp], sort_keys=True)]
        assert R.closed_form(nb, min_pts)[0] == want.tolist(), case  # the formulation the kernels compute
        core = np.array([len(x) + 1 >= min_pts for x in nb])
        if (want < 0).any():
            seen.add("noise")
        if ((want >= 0) & ~core).any():
            seen.add("border")
        if want.max(initial=-1) >= 1:
            seen.add("clusters")
    assert seen == {"noise", "border", "clusters"}
    assert compared == len(cases) - 8  # the 8 cases past the u32 size bound, see the next test
    # the hand-built set at minPts 4: point 6 touches both clusters and goes to the first, point 0 is absorbed after being noise
    i = cases.index(("hand", {"use64": False}, 0.04, 4, P.KMER, 0))
    assert _labels(fx, i).tolist() == [0] * 7 + [1] * 6 + [-1, -1, -1]
    # the u16 saturation: at the first eps the u32 path refuses the pair that the u64 path accepts
    flip, below, above = P.saturation_eps()
    for use64, eps, want in [(False, flip, [-1, -1]), (True, flip, [0, 0]), (False, below, [-1, -1]), (True, below, [-1, -1]),
                             (False, above, [0, 0]), (True, above, [0, 0])]:
        assert _labels(fx, cases.index(("saturation", {"use64": use64}, eps, 2, P.KMER, 0))).tolist() == want
    edge = P.saturation_edge_eps()  # between 65 535 and 65 536 common hashes: the u16 count stops below the boundary
    assert _labels(fx, cases.index(("saturation", {"use64": False}, edge, 2, P.KMER, 0))).tolist() == [-1, -1]
    assert _labels(fx, cases.index(("saturation", {"use64": True}, edge, 2, P.KMER, 0))).tolist() == [0, 0]
    # the 1e-12 tolerance: accepted just inside, refused just outside
    for a, b, c in P.NEAR_TIES:
        e_in, e_out = P.near_tie_eps(a, b, c, P.KMER)
        for use64 in (False, True):
            args = {"a": a, "b": b, "c": c, "use64": use64}
            assert _labels(fx, cases.index(("near_tie", args, e_in, 2, P.KMER, 0))).tolist() == [0, 0]
            assert _labels(fx, cases.index(("near_tie", args, e_out, 2, P.KMER, 0))).tolist() == [-1, -1]
    # the hub: more than 10 000 touched candidates, some of them neighbours
    i = cases.index(("hub", {}, P.HUB_EPS, 3, P.KMER, 0))
    nb = _nbrs[json.dumps(["hub", {}, P.HUB_EPS, P.KMER, 0], sort_keys=True)]
    assert 100 < len(nb[0]) < P.HUB_POINTS // 10 and (_labels(fx, i) == _labels(fx, i)[0]).sum() > len(nb[0])


def test_u32_size_bound_is_where_reference_and_restatement_part():
    """Why rtc_dbscan refuses a u32 set with ceil(max size / jaccard_min) past INT_MAX: there the reference converts a double
    past INT_MAX to int (its u32 size bound), its neighbour test rejects everything for the sketches that overflow, and its
    labels are no longer the restated ones.  One step inside the bound the two agree (the test above covers every such case,
    the sets of sizes 1 and 2 at the same eps among them), and the u64 path, which has no int bound, agrees everywhere."""
    fx = _fixture("ref_dbscan.npz")
    cases = _cases(fx)
    outside, differ, agree_inside = 0, [], 0
    for i, case in enumerate(cases):
        gen, args, eps, min_pts, k, mp = case
        sk = P.sketches_of(gen, args)
        if not P.u32_bound_exceeded(sk, eps, k):
            if gen in ("sizes", "lists") and not args["use64"]:
                agree_inside += 1
            continue
        assert gen in ("sizes", "lists") and not args["use64"]
        outside += 1
        got, _ = _restated(case)
        if not np.array_equal(got, _labels(fx, i)):
            differ.append((args.get("sizes", args.get("sets")), eps, min_pts))
    assert outside == 8 and agree_inside == 10  # 3000 hashes overflow at all three eps, 3 hashes at 0.9 only
    # the example: every bound overflows at eps 0.9 and the reference finds no neighbour at all; the restatement one cluster
    i = cases.index(("sizes", {"sizes": P.OVERFLOW_SIZES, "use64": False}, 0.9, 2, P.KMER, 0))
    assert _labels(fx, i).tolist() == [-1] * 4 and _restated(cases[i])[0].tolist() == [0] * 4
    assert (P.OVERFLOW_SIZES, 0.9, 2) in differ
    # one step outside: the sketches of 3 hashes overflow (ceil(3 / t) > INT_MAX >= ceil(2 / t)) and lose their neighbours
    i = cases.index(("lists", {"sets": P.OUTSIDE_SETS, "use64": False}, 0.9, 3, P.KMER, 0))
    assert _labels(fx, i).tolist() == [-1] * 3 and _restated(cases[i])[0].tolist() == [0] * 3
    assert (P.OUTSIDE_SETS, 0.9, 3) in differ
    i = cases.index(("lists", {"sets": P.INSIDE_SETS, "use64": False}, 0.9, 3, P.KMER, 0))
    assert _labels(fx, i).tolist() == [0] * 3
    t = P.jaccard_min(0.9, P.KMER)
    assert t > 1e-12 and np.ceil(2 / t) <= P.INT_MAX < np.ceil(3 / t)


def _live_print(L, case, i, threads):
    gen, args, eps, min_pts, k, mp = case
    sk = P.sketches_of(gen, args)
    by_file = P.print_layout(i)
    return reflib.kssd_dbscan_print(L, sk, P.use64_of(sk), eps, min_pts, k, P.genomes_of(len(sk), by_file), by_file, threads=threads,
                                    max_posting=mp)


def test_dbscan_reference_live_against_fixture():
    fx = _fixture("ref_dbscan.npz")
    L = reflib.ref_dbscan()
    if L is None:
        return _no_live("libref_dbscan.so")
    for i, case in enumerate(_cases(fx)):
        lab, text, log = _live_print(L, case, i, threads=4 if i % 2 else 1)
        assert np.array_equal(lab, _labels(fx, i)), case
        assert hashlib.sha256(text).hexdigest() == str(fx["print_sha256"][i]), case
        m = re.search(r"-----Core points: (\d+) ", log)
        assert (int(m.group(1)) if m else 0) == int(fx["n_core"][i])


def test_dbscan_restatement_equals_the_live_reference_on_a_random_sweep():
    L = reflib.ref_dbscan()
    if L is None:
        return _no_live("libref_dbscan.so")
    sets = 320
    # first what the sweep contains, from the restatement alone: clusters, border points, noise and empty sketches all occur
    seen, expected = set(), []
    for seed in range(sets):
        sk, use64, eps, min_pts, k, mp, threads = P.random_set(seed)
        assert not P.u32_bound_exceeded(sk, eps, k)
        nb = R.neighbour_lists(sk, eps, k, use64, mp)
        walk, n_core = R.sequential_walk(nb, min_pts)
        want = np.array([x if x >= 0 else -1 for x in walk], dtype=np.int32)
        core = np.array([len(x) + 1 >= min_pts for x in nb])
        seen |= ({"noise"} if (want < 0).any() else set()) | ({"border"} if ((want >= 0) & ~core).any() else set())
        seen |= ({"clusters"} if want.max(initial=-1) >= 1 else set()) | ({"empty"} if any(len(s) == 0 for s in sk) else set())
        expected.append((want, n_core))
    assert seen == {"noise", "border", "clusters", "empty"}
    for seed in range(sets):
        sk, use64, eps, min_pts, k, mp, threads = P.random_set(seed)
        want, n_core = expected[seed]
        by_file = seed % 2 == 0
        genomes = P.genomes_of(len(sk), by_file)
        lab, text, log = reflib.kssd_dbscan_print(L, sk, use64, eps, min_pts, k, genomes, by_file, threads=threads, max_posting=mp)
        assert np.array_equal(lab, want), (seed, lab.tolist(), want.tolist())
        assert text.decode() == R.print_result(want.tolist(), genomes, by_file, eps, min_pts), seed
        m = re.search(r"-----Core points: (\d+) ", log)
        assert (int(m.group(1)) if m else 0) == n_core, seed


def test_u32_size_bound_live_on_both_sides():
    """nested sketches with sizes around INT_MAX * jaccard_min at large eps: inside the bound the live reference equals the
    restatement on every draw; outside it some draw differs"""
    L = reflib.ref_dbscan()
    if L is None:
        return _no_live("libref_dbscan.so")
    rng = np.random.default_rng(7)
    inside = differ = 0
    for _ in range(120):
        eps = float(rng.choice([0.75, 0.8, 0.85, 0.9, 0.95]))
        t = P.jaccard_min(eps, P.KMER)
        edge = int(P.INT_MAX * t)  # the largest size with ceil(size / t) <= INT_MAX, give or take one
        sizes = [int(x) for x in rng.integers(1, max(edge, 1) + 3, size=int(rng.integers(2, 7)))]
        sk = P.gen_sizes(sizes, False)
        min_pts = int(rng.integers(1, 4))
        lab, _, _ = reflib.kssd_dbscan(L, sk, False, eps, min_pts, P.KMER)
        want = R.labels_of(sk, eps, min_pts, P.KMER, False)
        if P.u32_bound_exceeded(sk, eps, P.KMER):
            differ += not np.array_equal(lab, want)
        else:
            inside += 1
            assert np.array_equal(lab, want), (sizes, eps, min_pts)
    assert inside >= 20 and differ >= 5


# ---- the post-processing ----
def _forest_walk(fx, visit):
    """every (forest, dedup distance) of the fixture in the writer's order: visit(seed, di, n, edges, lens, clusters, dedup, ks,
    rep, cand, reps by k)"""
    rep_at = list_at = 0
    off, flat = fx["lists_off"], fx["lists_flat"]

    def take(m):
        nonlocal list_at
        out = [flat[off[j]:off[j + 1]].tolist() for j in range(list_at, list_at + m)]
        list_at += m
        return out
    for seed in P.FOREST_SEEDS:
        n, edges, lens, dedups, ks = P.forest_case(seed)
        clusters = P.components(n, edges)
        assert fx["shape"][seed].tolist() == [n, len(edges), len(clusters)]
        for di, dd in enumerate(dedups):
            rep = fx["rep_flat"][rep_at:rep_at + n].tolist()
            rep_at += n
            cand = take(len(clusters))
            visit(seed, di, n, edges, lens, clusters, dd, ks, rep, cand, {k: take(len(clusters)) for k in ks})
    assert rep_at == len(fx["rep_flat"]) and list_at == len(off) - 1


def test_postprocess_restatement_equals_the_reference_on_the_fixture():
    fx = _fixture("ref_postprocess.npz")
    seen = set()

    def visit(seed, di, n, edges, lens, clusters, dd, ks, rep, cand, reps):
        assert RP.tree_medoids(n, edges, dd, lens) == rep, (seed, dd)
        assert RP.dedup_candidates(clusters, rep, dd) == cand, (seed, dd)
        for k in ks:
            assert RP.select_k_reps(clusters, cand, edges, n, rep, k) == reps[k], (seed, dd, k)
            if any(len(r) == k < len(c) for r, c in zip(reps[k], cand)):
                seen.add("k below the candidates")
        if rep != list(range(n)):
            seen.add("collapsed")
        if dd > 0 and rep == list(range(n)) and edges:
            seen.add("nothing collapsed")
        if di in (5, 7) and edges:  # one ulp either side of an edge weight
            seen.add(("ulp", di))
    _forest_walk(fx, visit)
    assert seen >= {"collapsed", "k below the candidates", ("ulp", 5), ("ulp", 7)}
    # one ulp below an edge's weight and on it give different groups somewhere
    cut = []

    def ulp(seed, di, n, edges, lens, clusters, dd, ks, rep, cand, reps):
        cut.append(rep)
    _forest_walk(fx, ulp)
    assert any(cut[8 * s + 5] != cut[8 * s + 6] for s in P.FOREST_SEEDS)


def test_postprocess_reference_live_against_fixture():
    fx = _fixture("ref_postprocess.npz")
    L = reflib.ref_post()
    if L is None:
        return _no_live("libref_post.so")

    def visit(seed, di, n, edges, lens, clusters, dd, ks, rep, cand, reps):
        got_rep, got_cand = reflib.dedup_candidates(L, n, clusters, edges, lens, dd, by_file=(seed + di) % 2 == 0)
        assert got_rep == rep and got_cand == cand, (seed, dd)
        for k in ks:
            assert reflib.select_k_reps(L, n, clusters, cand, edges, rep, k) == reps[k], (seed, dd, k)
    _forest_walk(fx, visit)
    # node_to_rep of tests/test_gpu_postprocess.py's forests, with the cluster lists tests/test_gpu_refpin.py passes
    from tests import test_gpu_postprocess as T
    big = [(11, [10_000, 3000, 40, 2], shape, weights) for shape, weights in [("chain", "rand"), ("star", "tie"), ("random", "tie"), ("random", "rand")]]
    for name, forests in (("small", T.CASES), ("big", big)):
        for i, (seed, sizes, shape, weights) in enumerate(forests):
            n, edges, lens = T._forest(seed, sizes, shape, weights)
            rep, _ = reflib.dedup_candidates(L, n, P.components(n, edges), edges, [int(x) for x in lens], 0.01)
            assert rep == fx["%s%d_rep" % (name, i)].tolist(), (name, i)


def test_postprocess_restatement_equals_the_live_reference_on_random_forests():
    L = reflib.ref_post()
    if L is None:
        return _no_live("libref_post.so")
    for seed in range(1000, 1300):
        n, edges, lens, dedups, ks = P.forest_case(seed)
        clusters = P.components(n, edges)
        dd = dedups[seed % len(dedups)]
        k = ks[seed % len(ks)]
        rep, cand = reflib.dedup_candidates(L, n, clusters, edges, lens, dd, by_file=seed % 2 == 0)
        assert RP.tree_medoids(n, edges, dd, lens) == rep and RP.dedup_candidates(clusters, rep, dd) == cand, seed
        assert RP.select_k_reps(clusters, cand, edges, n, rep, k) == reflib.select_k_reps(L, n, clusters, cand, edges, rep, k), seed
