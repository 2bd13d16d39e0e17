"""clust-dbscan --knn on the GPU (rtc_dbscan_knn): labels, core flags and counts identical to the restated k-NN DBSCAN
(tests/refdbscan_knn.py: the reference's min-heap and sequential walk) on the sweep's family sets, on a set where every score
ties and the arrival order decides, on a directed chain many propagation rounds deep, the delegation of u64 sketches and
knn_k = 0 to rtc_dbscan, and the command line end to end.  Past one wave of 64 lanes (tests/knn_sets.py, whose cases
tests/test_cpu_dbscan_knn.py proves on the restatement): the star set, whose labels show every hub row's kept neighbours, with
rows of up to 147 passers, k up to 129, tied groups of 119 and first-shared indices from 63 to past 3 000 -- alone, under row
chunks and with max_posting pruning -- and bridged stars whose cluster number travels through rows longer than a wave.  Then
the binary32 eps test of the k-NN branch, u16 saturation inside the score, and the degenerate inputs (one point, no candidate
pair, knn_k = INT_MAX).  Every comparison is exact."""
import functools
import json
import os
import struct

import numpy as np
import pytest

from tests import knn_sets as K
from tests import refdbscan as R
from tests import refdbscan_knn as RK
from tests import sweep_sets as S
from tests.test_gpu_dbscan import BIN, _folders, _write_fastas
from tests.test_gpu_dbscan_mash import _run

pytestmark = pytest.mark.gpu

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))
EPS = (S.EPS[2], S.EPS[4])  # 0.02 and 0.06: between and beyond the families' distances


def _set(ctx, sketches, width=4):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=S.KMER, kind="kssd", width=width)


def _check(ctx, sk, host, eps, min_pts, knn_k, max_posting=0):
    want, want_core = RK.labels_of_knn(host, eps, min_pts, S.KMER, knn_k, max_posting, return_core=True)
    got, core = ctx.dbscan_knn(sk, eps, min_pts, S.KMER, knn_k, max_posting=max_posting, return_core=True)
    assert np.array_equal(got, want), (eps, min_pts, knn_k, max_posting, got.tolist(), want.tolist())
    assert np.array_equal(core, want_core), (eps, min_pts, knn_k, max_posting)
    assert ctx.dbscan_knn_counts == (int(want.max(initial=-1)) + 1, int((want < 0).sum()))
    c = ctx.dbscan_knn_counters()
    assert c["core_points"] == int(want_core.sum())
    return got, c


@functools.lru_cache(maxsize=None)
def _family(seed):
    return S.family_sets(seed, False, n_empty=2)


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("max_posting", [0, 5])
def test_families_match_the_heap_and_the_walk(ctx, seed, max_posting):
    host = _family(seed)
    n = len(host)
    assert any(len(s) == 0 for s in host)
    if max_posting:  # the value prunes: some hash is held by more sketches
        assert len(R.kept_hashes(host, max_posting)) < len(R.kept_hashes(host, 0))
    sk = _set(ctx, host)
    truncated = 0
    seen = set()
    for eps in EPS:
        passers = RK.passers_in_arrival_order(host, eps, S.KMER, max_posting)
        for min_pts in (2, 5):
            for knn_k in (min_pts - 1, 5, 20, n):
                got, c = _check(ctx, sk, host, eps, min_pts, knn_k, max_posting)
                k = RK.effective_k(knn_k, min_pts)
                assert c["passers"] == sum(len(p) for p in passers)
                assert c["truncated_rows"] == sum(len(p) > k for p in passers)
                truncated += c["truncated_rows"]
                seen.add(tuple(got.tolist()))
    assert truncated > 0 and len(seen) >= 3  # k cut rows, and the parameters cut the set in different ways


def tie_set(seed):
    """40 members of a base of 64 hashes, each with a different single base hash replaced by a unique one: every pair of them
    shares 62 and scores 62 / 66, and a member that lacks the base's first hash meets the others at its second, so the arrival
    order is not the id order.  Then 10 sketches of 63 base hashes each (62 / 65 against a member: higher, and with the highest
    ids they arrive last and pop tied entries), and 3 satellites of 40 base hashes and 24 of their own, which list members
    that never list them."""
    rng = np.random.default_rng(seed)

    def fresh(m):
        return rng.integers(1, (1 << 31) - 1, size=m, dtype=np.int64)
    base = np.unique(fresh(64))
    assert len(base) == 64
    members = []
    for i in rng.permutation(64)[:40]:
        s = base.copy()
        s[i] = fresh(1)[0]
        members.append(s)
    members = [members[i] for i in rng.permutation(40)]
    high = [np.delete(base, int(i)) for i in rng.permutation(64)[:10]]
    sat = [np.concatenate([base[rng.permutation(64)[:40]], fresh(24)]) for _ in range(3)]
    return [np.unique(s).astype(np.uint32) for s in members + high + sat]


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("knn_k", [5, 12])
def test_tie_set_follows_the_arrival_order(ctx, seed, knn_k):
    host = tie_set(seed)
    eps, min_pts = 0.06, knn_k + 1  # a row that keeps k neighbours is a core point, a shorter one is not
    # what the set must show on the restatement, or the comparison below proves nothing
    passers = RK.passers_in_arrival_order(host, eps, S.KMER)
    assert sum(len(p) > knn_k for p in passers) >= 1
    by_score = 0
    for p in passers:
        if len(p) > knn_k:
            held = {c for c, _ in RK.heap_select(p, knn_k)}
            best = {c for c, _ in sorted(p, key=lambda x: (-float(x[1]), x[0]))[:knn_k]}
            by_score += held != best
    assert by_score >= 1  # the kept set is not "the k best scores, ties by lowest id"
    nbrs = RK.knn_lists(host, eps, S.KMER, knn_k)
    assert any(p not in nbrs[q] for p in range(len(nbrs)) for q in nbrs[p])  # a neighbour in one direction only
    want = RK.labels_of_knn(host, eps, min_pts, S.KMER, knn_k)
    undirected, _ = R.closed_form(nbrs, min_pts)
    assert (want != np.asarray(undirected)).any()
    _, c = _check(ctx, _set(ctx, host), host, eps, min_pts, knn_k)
    assert c["arrival_rows"] >= 1 and c["truncated_rows"] == sum(len(p) > knn_k for p in passers)
    assert c["neighbour_edges"] == sum(len(x) for x in nbrs)


def test_directed_chain_is_one_cluster(ctx):
    # 64 sliding windows of 100 hashes in steps of 25, the last window first: with k = 1 every window keeps the one before it in
    # the scan of its hashes, which is the next point, so the edges run 0 -> 1 -> ... -> 63 (and 63 -> 62) and point 0's number
    # has 63 hops to travel
    n = 64
    host = [np.arange(1 << 20, (1 << 20) + 100, dtype=np.uint32) + 25 * (n - 1 - j) for j in range(n)]
    nbrs = RK.knn_lists(host, 0.04, S.KMER, 1)
    assert nbrs == [[j + 1] for j in range(n - 1)] + [[n - 2]]
    got, c = _check(ctx, _set(ctx, host), host, 0.04, 2, 1)
    assert (got == 0).all()
    print("directed chain of %d points: %d propagation rounds" % (n, c["rounds"]))
    assert 1 <= c["rounds"] <= n + 1  # a number may travel several hops within a round, never fewer than one


@pytest.mark.parametrize("max_posting", [0, 5])
def test_u64_sketches_and_k_zero_are_the_plain_call(ctx, max_posting):
    for width, knn_k in ((8, 5), (8, 0), (4, 0), (4, -3)):
        host = S.family_sets(3, width == 8, n_empty=2)
        sk = _set(ctx, host, width)
        for min_pts in (2, 5):
            want, want_core = ctx.dbscan(sk, 0.04, min_pts, S.KMER, max_posting=max_posting, return_core=True)
            got, core = ctx.dbscan_knn(sk, 0.04, min_pts, S.KMER, knn_k, max_posting=max_posting, return_core=True)
            assert np.array_equal(got, want) and np.array_equal(core, want_core), (width, knn_k, min_pts)
            assert ctx.dbscan_knn_counts == (int(want.max(initial=-1)) + 1, int((want < 0).sum()))


def test_row_chunks_keep_the_labels(ctx):
    # every sketch shares one hash with every other (as test_gpu_dbscan's chunk test builds them): the candidate list is the
    # whole triangle, the smallest edge budget cuts it, and k cuts every row
    n = 200
    rng = np.random.default_rng(3)
    host = []
    for g in range(n):
        body = np.arange(100_000 * (g % 7), 100_000 * (g % 7) + 60)[rng.random(60) < 0.9]
        host.append(np.unique(np.concatenate([[1], body, np.arange(10_000_000 + 1000 * g, 10_000_000 + 1000 * g + 5)])).astype(np.uint32))
    sk = _set(ctx, host)
    want, c1 = _check(ctx, sk, host, 0.1, 4, 6)
    assert c1["chunks"] == 1 and c1["candidate_edges"] == n * (n - 1) // 2 and c1["truncated_rows"] > 0
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        got, c2 = _check(ctx, sk, host, 0.1, 4, 6)
    assert np.array_equal(got, want) and c2["chunks"] > 1
    assert {k: c2[k] for k in ("candidate_edges", "passers", "truncated_rows", "arrival_rows", "neighbour_edges")} == \
           {k: c1[k] for k in ("candidate_edges", "passers", "truncated_rows", "arrival_rows", "neighbour_edges")}


COUNTERS = ("candidate_edges", "passers", "truncated_rows", "arrival_rows", "neighbour_edges")


def _check_rows(ctx, sk, host, eps, min_pts, knn_k, max_posting=0):
    """_check, and the counters that follow from the restatement's rows"""
    got, c = _check(ctx, sk, host, eps, min_pts, knn_k, max_posting)
    k = RK.effective_k(knn_k, min_pts)
    passers = RK.passers_in_arrival_order(host, eps, S.KMER, max_posting)
    shapes = [K.row_shape(p, k) for p in passers]
    assert c["passers"] == sum(len(p) for p in passers)
    assert c["truncated_rows"] == sum(P > k for P, *_ in shapes)
    assert c["arrival_rows"] == sum(Q > k for _, _, Q, _, _ in shapes)
    assert c["neighbour_edges"] == sum(len(x) for x in RK.knn_lists(host, eps, S.KMER, k, max_posting))
    return got, c


@functools.lru_cache(maxsize=None)
def _star(seed):
    return K.star_set(seed)[0]


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
@pytest.mark.parametrize("knn_k", K.KS)
def test_star_set_selection_is_visible_in_the_labels(ctx, seed, knn_k):
    assert K.KMER == S.KMER
    host = _star(seed)
    got, c = _check_rows(ctx, _set(ctx, host), host, K.EPS, K.MIN_PTS, knn_k)
    assert c["truncated_rows"] >= c["arrival_rows"] >= 1 and c["chunks"] == 1
    if knn_k == 64:
        assert c["truncated_rows"] > c["arrival_rows"]  # the row with exactly k passers at or above s*
    # a pair is a hub and a leaf: every leaf lists its hub, a hub lists the leaves it kept, a leaf not kept is noise
    assert c["neighbour_edges"] == 2 * c["candidate_edges"] - (got < 0).sum()


@pytest.mark.parametrize("knn_k", [64, 100])
def test_star_set_under_row_chunks(ctx, knn_k):
    host = K.chunk_star_set(1)[0]
    n = len(host)
    sk = _set(ctx, host)
    want, c1 = _check_rows(ctx, sk, host, K.CHUNK_EPS, K.MIN_PTS, knn_k)
    assert c1["chunks"] == 1 and c1["candidate_edges"] == n * (n - 1) // 2 and c1["arrival_rows"] >= 1
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        got, c2 = _check_rows(ctx, sk, host, K.CHUNK_EPS, K.MIN_PTS, knn_k)
    assert np.array_equal(got, want) and c2["chunks"] > 1
    assert {x: c2[x] for x in COUNTERS} == {x: c1[x] for x in COUNTERS}


@pytest.mark.parametrize("knn_k", [64, 128])
def test_star_set_with_pruned_postings(ctx, knn_k):
    host = K.star_set(1, decoy=True)[0]
    want = RK.labels_of_knn(host, K.EPS, K.MIN_PTS, S.KMER, knn_k, K.DECOY_MAX_POSTING)
    assert not np.array_equal(want, RK.labels_of_knn(host, K.EPS, K.MIN_PTS, S.KMER, knn_k))  # the pruning changes this result
    sk = _set(ctx, host)
    _, c = _check_rows(ctx, sk, host, K.EPS, K.MIN_PTS, knn_k, K.DECOY_MAX_POSTING)
    assert c["arrival_rows"] >= 1
    _check_rows(ctx, sk, host, K.EPS, K.MIN_PTS, knn_k)


@pytest.mark.parametrize("low,knn_k", [(False, 2), (False, 64), (False, 129), (True, 200)])
def test_bridged_stars_propagate_through_long_rows(ctx, low, knn_k):
    host, info = K.bridged_star_set(1, low)
    got, c = _check_rows(ctx, _set(ctx, host), host, K.EPS, K.MIN_PTS, knn_k)
    assert (got[info["hubs"] + info["bridges"]] == 0).all() and got.max() == 0
    print("bridged stars, k %d: %d propagation rounds" % (knn_k, c["rounds"]))
    assert 2 <= c["rounds"] <= len(host) + 1


@pytest.mark.parametrize("a,b,c", K.float_boundary_pairs())
def test_float_score_decides_the_eps_test(ctx, a, b, c):
    eps = K.float_boundary_eps(a, b, c)
    host = K.float_boundary_sketches(a, b, c)
    sk = _set(ctx, host)
    got, cnt = _check(ctx, sk, host, eps, 2, 5)
    assert got.tolist() == [-1, -1]
    assert cnt["passers"] == 2 and cnt["neighbour_edges"] == 0 and cnt["candidate_edges"] == 1
    assert ctx.dbscan(sk, eps, 2, S.KMER).tolist() == [0, 0]


def test_u16_saturation_changes_the_kept_neighbour(ctx):
    host = K.saturated_choice_set()
    got, c = _check(ctx, _set(ctx, host), host, K.SATURATED_EPS, 2, 1)
    assert got.tolist() == [0, 1, 0]  # exact counts would give 0, 0, 1 (test_cpu_dbscan_knn)
    assert c["passers"] == 6 and c["truncated_rows"] == 3 and c["neighbour_edges"] == 3


def test_degenerate_sets(ctx):
    one = [np.arange(100, 200, dtype=np.uint32)]
    got, c = _check(ctx, _set(ctx, one), one, 0.05, 2, 3)
    assert got.tolist() == [-1] and c["candidate_edges"] == 0 and c["passers"] == 0 and c["rounds"] == 0
    apart = [np.arange(1000 * g, 1000 * g + 50 + g, dtype=np.uint32) for g in range(1, 4)]
    for min_pts in (1, 2):  # at minPts 1 every point is a core point and a cluster of its own
        got, c = _check(ctx, _set(ctx, apart), apart, 0.05, min_pts, 3)
        assert got.tolist() == ([0, 1, 2] if min_pts == 1 else [-1, -1, -1])
        assert c["candidate_edges"] == 0 and c["passers"] == 0 and c["neighbour_edges"] == 0
    host = _star(1)
    _, c = _check_rows(ctx, _set(ctx, host), host, K.EPS, K.MIN_PTS, 2 ** 31 - 1)
    assert c["truncated_rows"] == 0 and c["arrival_rows"] == 0 and c["neighbour_edges"] == c["passers"]


def _folder_sketches(folder, n):
    raw = open(os.path.join(folder, "kssd.hash.sketch"), "rb").read()
    pos, out = 20, []
    for _ in range(n):
        (m,) = struct.unpack_from("<Q", raw, pos)
        pos += 8
        out.append(np.frombuffer(raw, dtype="<u4", count=m, offset=pos).copy())
        pos += 4 * m
    assert pos == len(raw)
    return out


def test_cli_end_to_end(oracle, tmp_path):
    tmp = str(tmp_path)
    # -k 18: inside what the tuner keeps for genomes of 500 kbp, and even, so a folder's half_k * 2 is the same k
    L, k, eps, min_pts, knn_k = 500_000, 18, 0.05, 3, 3
    lst, seqs, meta = _write_fastas(oracle, tmp, 8, 8, L, seed=5)
    assert len(seqs) == 64
    D = os.path.join(BIN, "clust-dbscan")
    d1 = os.path.join(tmp, "l")
    os.makedirs(d1)
    out, mj = os.path.join(tmp, "l.out"), os.path.join(tmp, "m.json")
    flags = ["--eps", str(eps), "--minpts", str(min_pts), "--knn", str(knn_k)]
    err = _run([D, "--fast", "-l", "-i", lst, "-k", str(k)] + flags + ["-t", "4", "-o", out], d1, env={"RTC_METRICS_JSON": mj})
    assert "-----the kmerSize is: %d\n" % k in err
    folder = _folders(d1)
    assert len(folder) == 1
    host = _folder_sketches(folder[0], len(seqs))
    want = RK.labels_of_knn(host, eps, min_pts, k, knn_k)
    plain = R.labels_of(host, eps, min_pts, k, False)
    assert int(want.max()) >= 1 and not np.array_equal(want, plain)  # the flag changes this result
    assert open(out).read() == R.print_result(want, meta, True, eps, min_pts)
    assert "-----DBSCAN parameters: eps=%g, minPts=%d, knn=%d\n" % (eps, min_pts, knn_k) in err
    assert "-----WARNING: knn_k (3) may be too small for stable DBSCAN. Consider knn_k >= 10.\n" in err
    assert "-----WARNING: k-NN acceleration is approximate for DBSCAN (may miss eps neighbors if k is small).\n" in err
    assert "-----Found %d clusters\n" % (int(want.max()) + 1) in err
    metrics = json.load(open(mj))
    assert metrics["dbscan_knn_k"] == knn_k
    for key in ("dbscan_s", "dbscan_knn_select_s", "dbscan_knn_propagate_s", "dbscan_knn_truncated_rows"):
        assert key in metrics and metrics[key] >= 0, key
    assert metrics["dbscan_knn_truncated_rows"] == sum(len(p) > knn_k for p in RK.passers_in_arrival_order(host, eps, k))
    # the same from the folder; --knn below minPts - 1 is raised with the reference's line
    out2 = os.path.join(tmp, "p.out")
    err2 = _run([D, "--fast", "--presketched", folder[0], "-l"] + flags + ["-o", out2], tmp)
    assert open(out2, "rb").read() == open(out, "rb").read() and "sketch format mismatch" not in err2
    out3 = os.path.join(tmp, "p3.out")
    err3 = _run([D, "--fast", "--presketched", folder[0], "-l", "--eps", str(eps), "--minpts", "5", "--knn", "2", "-o", out3], tmp)
    assert "-----WARNING: knn_k (2) < minPts-1 (4). Adjusting knn_k to 4.\n" in err3
    assert open(out3).read() == R.print_result(RK.labels_of_knn(host, eps, 5, k, 2), meta, True, eps, 5)
