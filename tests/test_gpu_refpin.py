"""The DBSCAN and tree-medoid kernels against the reference itself: rtc_dbscan, rtc_dbscan_sweep, clust-dbscan's output file
and rtc_tree_medoids (GPU and host path) compared with the reference's KssdDBSCAN, printKssdDBSCANResult and
build_dedup_candidates_per_cluster, called live through oracle/_ref/libref_dbscan.so / libref_post.so (tests/reflib.py) on the
same host arrays.  Where those libraries are not built the same tests compare with what the reference recorded for the same
inputs (tests/golden/ref_dbscan.npz / ref_postprocess.npz, inputs checked by SHA-256); with neither they fail.  Every
comparison is equality.  The module's last test prints how many cases were compared live and how many with the fixture, past
pytest's capture, and fails if the libraries load and nothing was compared live."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import reflib, refpin_cases as P
from tests import sweep_sets as S
from tests import test_gpu_postprocess as TP
from tests.test_gpu_dbscan import BIN, SOAK_SEEDS, _family_sketches, _run

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNT = {"live": 0, "fixture": 0}
_fx = {}      # loaded fixture files by name
_index = {}   # ref_dbscan.npz: case key -> position, and the input hashes
_want_cache = {}


def _fixture(name):
    if name not in _fx:
        path = os.path.join(GOLD, name)
        _fx[name] = np.load(path) if os.path.exists(path) else None
    return _fx[name]


def _reference_labels(case, host):
    """the reference's labels of a refpin_cases case whose sketches are `host`: live (1 and 4 threads, which must agree) or
    from the fixture, after checking that the fixture's input is this one"""
    key = P.case_key(case)
    if key in _want_cache:
        return _want_cache[key]
    gen, args, eps, min_pts, k, mp = case
    use64 = P.use64_of(host) if len(host) else False
    L = reflib.ref_dbscan()
    if L is not None:
        want, ncl, nnoise = reflib.kssd_dbscan(L, host, use64, eps, min_pts, k, threads=1, max_posting=mp)
        want4, _, _ = reflib.kssd_dbscan(L, host, use64, eps, min_pts, k, threads=4, max_posting=mp)
        assert np.array_equal(want, want4), ("the reference's labels depend on its thread count", case)
        assert ncl == int(want.max(initial=-1)) + 1 and nnoise == int((want < 0).sum())
        COUNT["live"] += 1
    else:
        fx = _fixture("ref_dbscan.npz")
        if fx is None:
            pytest.fail("neither oracle/_ref/libref_dbscan.so nor tests/golden/ref_dbscan.npz is there")
        if not _index:
            _index["cases"] = {json.dumps(c, sort_keys=True): i for i, c in enumerate(json.loads(str(fx["cases"])))}
            _index["inputs"] = json.loads(str(fx["inputs"]))
        if key not in _index["cases"]:
            pytest.fail("the fixture holds no record of %s and the reference library is not built" % key)
        assert P.input_sha(host) == _index["inputs"][json.dumps([gen, args], sort_keys=True)], "the input is not the fixture's"
        i = _index["cases"][key]
        want = fx["labels_flat"][fx["labels_off"][i]:fx["labels_off"][i + 1]]
        COUNT["fixture"] += 1
    _want_cache[key] = want
    return want


def _set(ctx, host, k):
    from rabbittclust_amd import api
    width = 8 if len(host) and P.use64_of(host) else 4
    return api.SketchSet.from_host(host, ctx.device, k=k, kind="kssd", width=width)


def _check(ctx, sk, host, case):
    gen, args, eps, min_pts, k, mp = case
    got = ctx.dbscan(sk, eps, min_pts, k, max_posting=mp)
    want = _reference_labels(case, host)
    assert np.array_equal(got, want), (case, got.tolist(), want.tolist())
    assert ctx.dbscan_counters()["asymmetric_pairs"] == 0
    return got


def _family_args(seed):
    return dict(P.KSSD_FAMILIES[0], seed=seed)


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_kssd_families_from_the_sketch_kernel(ctx, oracle, seed):
    sk, host = _family_sketches(ctx, oracle, seed)
    assert sk.width == 4
    seen = set()
    for eps in P.FAMILY_EPS:
        for min_pts in P.FAMILY_MINPTS:
            got = _check(ctx, sk, host, ("kssd_family", _family_args(seed), eps, min_pts, 22, 0))
            seen.add(int(got.max(initial=-1)) + 1)
    assert len(seen) > 2


def test_kssd_family_u64_and_max_posting(ctx, oracle):
    a = P.KSSD_FAMILY_U64
    sk, host = _family_sketches(ctx, oracle, a["seed"], n_fam=a["n_fam"], per=a["per"], L=a["L"], k=a["k"], drlevel=a["drlevel"])
    assert sk.width == 8
    for eps in (0.01, 0.03, 0.08):
        for min_pts in (1, 2, 5):
            _check(ctx, sk, host, ("kssd_family", a, eps, min_pts, 26, 0))
    a = P.KSSD_FAMILY_POSTING
    sk, host = _family_sketches(ctx, oracle, a["seed"], n_fam=a["n_fam"], per=a["per"], L=a["L"])
    for mp in (1, 2, 3, 4, 8, 1000):
        _check(ctx, sk, host, ("kssd_family", a, 0.05, 2, 22, mp))


def _built_cases(gens):
    return [c for c in P.dbscan_cases() if c[0] in gens]


@pytest.mark.parametrize("gen", ["hand", "saturation", "near_tie", "hub", "lists", "sizes"])
def test_built_sets_both_widths(ctx, gen):
    """the hand-built sets: border point of two clusters, absorbed noise, empty sketches, the u16 saturation, the 1e-12
    tolerance, the hub past the reference's parallel evaluation threshold, the sets at the u32 size bound (those past it are
    refused: test_refusals_past_the_u32_size_bound)"""
    n = 0
    for case in _built_cases({gen}):
        host = P.sketches_of(case[0], case[1])
        if P.u32_bound_exceeded(host, case[2], case[4]):
            continue
        _check(ctx, _set(ctx, host, case[4]), host, case)
        n += 1
    assert n >= 3


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("use64", [False, True])
def test_family_sets_single_calls_and_sweep_levels(ctx, seed, use64):
    """sweep_sets.family_sets with two empty sketches: Context.dbscan, and every level of Context.dbscan_sweep, equal to one
    reference run at that eps (the sweep has no counterpart in the reference: a run per level is its definition)"""
    args = dict(seed=seed, use64=use64, n_empty=2)
    host = P.sketches_of("family", args)
    sk = _set(ctx, host, S.KMER)
    for min_pts in (0, 1, 2, 5, 100):
        for mp in ((0,) if use64 else (0, 1, 5)):
            levels = ctx.dbscan_sweep(sk, S.EPS, min_pts, S.KMER, max_posting=mp)
            assert levels.shape == (len(S.EPS), len(host))
            for e, eps in enumerate(S.EPS):
                case = ("family", args, eps, min_pts, S.KMER, mp)
                want = _check(ctx, sk, host, case)
                assert np.array_equal(levels[e], want), (case, levels[e].tolist(), want.tolist())
            # the levels are not all alike, or the comparison shows little.  Two settings make them alike by construction, in
            # the reference too: max_posting 1 drops every hash two sketches share, so no point has a neighbour at any eps, and
            # at minPts 100 > n no point is a core point.
            if mp != 1 and min_pts <= 5:
                assert len({tuple(r.tolist()) for r in levels}) >= 3, (min_pts, mp)


def test_row_chunks_equal_the_reference(ctx):
    host = P.sketches_of(*P.ROW_CHUNKS[:2])
    sk = _set(ctx, host, P.KMER)
    one = _check(ctx, sk, host, P.ROW_CHUNKS)
    assert ctx.dbscan_counters()["chunks"] == 1
    with ctx.env(RTC_EDGE_BUDGET=str(64 * len(host) + 1024)):
        cut = _check(ctx, sk, host, P.ROW_CHUNKS)
        assert ctx.dbscan_counters()["chunks"] > 2
        levels = ctx.dbscan_sweep(sk, [0.05, 0.1], 4, P.KMER)
    assert np.array_equal(one, cut) and np.array_equal(levels[1], one)
    assert one.max() >= 1 and (np.bincount(one[one >= 0]) > 50).any()


def test_refusals_past_the_u32_size_bound(ctx):
    """u32 sketches whose size bound ceil(size / jaccard_min) is past INT_MAX: refused on the host before any launch (there
    the reference's own result is an overflowed int conversion, tests/test_cpu_refpin.py); the same hashes as u64 are accepted
    and equal the reference's brute force; the context works afterwards"""
    from rabbittclust_amd import api
    case32 = ("sizes", {"sizes": P.OVERFLOW_SIZES, "use64": False}, 0.9, 2, P.KMER, 0)
    case64 = ("sizes", {"sizes": P.OVERFLOW_SIZES, "use64": True}, 0.9, 2, P.KMER, 0)
    host32, host64 = P.sketches_of(*case32[:2]), P.sketches_of(*case64[:2])
    assert P.u32_bound_exceeded(host32, 0.9, P.KMER) and P.jaccard_min(0.9, P.KMER) > 1e-12
    sk32 = _set(ctx, host32, P.KMER)
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan(sk32, 0.9, 2, P.KMER)
    assert ei.value.status == api._lib.RTC_ERR_UNSUPPORTED and "past INT_MAX" in str(ei.value)
    msg = str(ei.value).split(": ", 1)[1]  # the single call names itself and no place in a list
    assert msg.startswith("rtc_dbscan: size bound ceil(") and "of the list" not in msg
    with pytest.raises(api.RtcError) as ei:
        ctx.dbscan_sweep(sk32, [0.05, 0.9], 2, P.KMER)
    assert ei.value.status == api._lib.RTC_ERR_UNSUPPORTED and "past INT_MAX" in str(ei.value)
    sk64 = _set(ctx, host64, P.KMER)
    got = _check(ctx, sk64, host64, case64)
    assert got.tolist() == [0, 0, 0, 0]
    levels = ctx.dbscan_sweep(sk64, [0.6, 0.9], 2, P.KMER)
    assert np.array_equal(levels[1], got)
    assert np.array_equal(levels[0], _reference_labels(("sizes", case64[1], 0.6, 2, P.KMER, 0), host64))
    # the context works afterwards: one step inside the bound the u32 set is accepted
    inside = ("lists", {"sets": P.INSIDE_SETS, "use64": False}, 0.9, 3, P.KMER, 0)
    h = P.sketches_of(*inside[:2])
    _check(ctx, _set(ctx, h, P.KMER), h, inside)


def test_clust_dbscan_file_is_byte_equal_to_the_reference_print(oracle, tmp_path):
    """clust-dbscan's output file against printKssdDBSCANResult's, in the -l layout and in the sequence layout"""
    a = P.KSSD_FAMILY_CLI
    tmp = str(tmp_path)
    from rabbittclust_amd import api
    desc = api.synth_family_descs(a["n_fam"], a["per"], global_seed=a["seed"])
    seqs = [oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), a["L"]) for d in desc]
    names = []
    for g, s in enumerate(seqs):
        names.append("g%03d.fna" % g)
        with open(os.path.join(tmp, names[-1]), "wb") as f:
            f.write((">g%d synthetic family %d\n" % (g, g // a["per"])).encode() + s.tobytes() + b"\n")
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")
    with open(os.path.join(tmp, "all.fna"), "wb") as f:
        for g, s in enumerate(seqs):
            f.write((">r%d member %d\n" % (g, g)).encode() + s.tobytes() + b"\n")
    host = [oracle.kssd_sketch(s, a["k"], a["drlevel"]) for s in seqs]
    D = os.path.join(BIN, "clust-dbscan")
    L = reflib.ref_dbscan()
    fx = _fixture("ref_dbscan.npz")
    if L is None and fx is None:
        pytest.fail("neither oracle/_ref/libref_dbscan.so nor tests/golden/ref_dbscan.npz is there")
    for i, (eps, min_pts, by_file) in enumerate(P.CLI_RUNS):
        out = os.path.join(tmp, "out%d.txt" % i)
        args = [D, "--fast"] + (["-l", "-i", "list.txt"] if by_file else ["-i", "all.fna"])
        err = _run(args + ["-k", "17", "--eps", str(eps), "--minpts", str(min_pts), "-e", "-t", "4", "-o", out], tmp)
        assert "-----the kmerSize is: 17" in err
        got = open(out, "rb").read()
        if L is not None:
            lab, want, _ = reflib.kssd_dbscan_print(L, host, False, eps, min_pts, 17, P.cli_genomes(by_file), by_file, threads=4)
            assert got == want
            assert lab.max() >= 1
            COUNT["live"] += 1
        else:
            assert P.input_sha(host) == json.loads(str(fx["inputs"]))[json.dumps(["kssd_family", a], sort_keys=True)]
            assert hashlib.sha256(got).hexdigest() == str(fx["cli_sha256"][i])
            COUNT["fixture"] += 1


# ---- the tree medoid ----
def _reference_rep(name, n, edges, lens):
    L = reflib.ref_post()
    if L is not None:
        rep, _ = reflib.dedup_candidates(L, n, P.components(n, edges), edges, [int(x) for x in lens], 0.01)
        COUNT["live"] += 1
        return rep
    fx = _fixture("ref_postprocess.npz")
    if fx is None:
        pytest.fail("neither oracle/_ref/libref_post.so nor tests/golden/ref_postprocess.npz is there")
    COUNT["fixture"] += 1
    return fx[name].tolist()


@pytest.mark.parametrize("i", range(len(TP.CASES)))
def test_tree_medoids_equal_the_reference(ctx, i):
    seed, sizes, shape, weights = TP.CASES[i]
    n, edges, lens = TP._forest(seed, sizes, shape, weights)
    want = _reference_rep("small%d_rep" % i, n, edges, lens)
    gpu, p_gpu = TP._medoids(ctx, n, edges, lens, 2)
    host, p_host = TP._medoids(ctx, n, edges, lens, 0)
    assert p_gpu == 2 and p_host == 1  # rtc_dedup_last_path: the sums really came from the GPU / the host
    assert gpu.tolist() == want and host.tolist() == want
    assert want != list(range(n))


@pytest.mark.parametrize("i,shape,weights", [(0, "chain", "rand"), (1, "star", "tie"), (2, "random", "tie"), (3, "random", "rand")])
def test_tree_medoids_equal_the_reference_on_ten_thousand_members(ctx, i, shape, weights):
    n, edges, lens = TP._forest(11, [10_000, 3000, 40, 2], shape, weights)
    want = _reference_rep("big%d_rep" % i, n, edges, lens)
    gpu, p_gpu = TP._medoids(ctx, n, edges, lens, 2)
    host, p_host = TP._medoids(ctx, n, edges, lens, 0)
    assert p_gpu == 2 and p_host == 1
    assert gpu.tolist() == want and host.tolist() == want
    assert len(set(want)) <= n - 13_000


def test_zz_count_of_cases_compared_with_the_reference(capsys):
    """runs last in this module: says in the run log, past the capture, against what the tests above compared"""
    with capsys.disabled():
        print("\nrefpin: %d cases compared with the live reference, %d with the fixture's record of it"
              % (COUNT["live"], COUNT["fixture"]))
    if reflib.ref_dbscan() is not None and reflib.ref_post() is not None:
        assert COUNT["live"] > 0 and COUNT["fixture"] == 0
    else:
        assert COUNT["fixture"] > 0
