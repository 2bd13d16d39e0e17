"""clust-greedy --order degree on the GPU (rtc_greedy_degree): every field of the result against the sequential restatement
(tests/refgreedy_degree.py) on the sets of tests/greedy_degree_sets.py -- families, a path whose selection takes n / 2 rounds with
and without the one-workgroup tail, small graphs that isolate one rule each, MinHash truncation, the threshold on a distance, a
clique of 4 200, a member with more than 4 096 candidate representatives, row chunks, tiny and failing inputs -- and the command
line end to end.  No tolerances: everything compared is an integer or a file."""
import json
import os

import numpy as np
import pytest

from tests import greedy_degree_sets as S
from tests import refdbscan_mash as M
from tests import refgreedy_degree as G
from tests.test_gpu_dbscan import BIN, _write_fastas

pytestmark = pytest.mark.gpu

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))
K = S.KMER
FIELDS = ("rep", "degree", "common", "denom")


def _set(ctx, sketches, width, kind):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=K, kind=kind, width=width)


def _same(got, want, what=""):
    want = G.as_arrays(want)
    for f, g, w in zip(FIELDS, got, want):
        bad = np.flatnonzero(np.asarray(g) != w)
        assert bad.size == 0, (what, f, [(int(v), int(g[v]), int(w[v])) for v in bad[:5]])
    assert got[4] == want[4], (what, got[4], want[4])


def _counters_fit(ctx, got):
    rep, deg = got[0], got[1]
    n = len(rep)
    c = ctx.greedy_degree_counters()
    assert c["kept_edges"] == int(deg.sum()) // 2 and c["representatives"] == got[4] == int((rep == np.arange(n)).sum())
    assert c["wave_rows"] + c["workgroup_rows"] == n - got[4] and c["tail_rounds"] <= c["rounds"]
    assert c["kept_edges"] <= c["candidate_edges"]
    return c


# ---- families ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_empty", [0, 3])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_family_sets(ctx, seed, width, n_empty):
    sk = S.families(seed, width == 8, n_empty)
    want = G.kssd(sk, S.FAMILY_THRESHOLD, K, width == 8)
    got = ctx.greedy_degree(_set(ctx, sk, width, "kssd"), S.FAMILY_THRESHOLD, K)
    _same(got, want)
    c = _counters_fit(ctx, got)
    assert c["chunks"] == 1 and c["merged"] == 0 and c["rounds"] >= 1
    for v, s in enumerate(sk):
        if len(s) == 0:  # an empty sketch is a cluster of its own, at both widths
            assert (got[0][v], got[1][v]) == (v, 0)
    with ctx.env(RTC_DEGREE_TAIL="0"):
        _same(ctx.greedy_degree(_set(ctx, sk, width, "kssd"), S.FAMILY_THRESHOLD, K), want, "no tail")
        assert ctx.greedy_degree_last_path() & 4 == 0 and ctx.greedy_degree_counters()["tail_rounds"] == 0


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_minhash_families(ctx, seed):
    s = 128
    sk = S.minhash_families(seed, s)
    counts = M.count_matrix(sk, s)
    for thr in (0.05, 0.01):
        want = G.minhash(sk, s, thr, K, counts=counts)
        got = ctx.greedy_degree(_set(ctx, sk, 8, "minhash"), thr, K, sketch_size=s)
        _same(got, want, thr)
        c = _counters_fit(ctx, got)
        assert c["kept_edges"] <= c["merged"] <= c["candidate_edges"]
    with ctx.env(RTC_DEGREE_TAIL="0"):
        _same(ctx.greedy_degree(_set(ctx, sk, 8, "minhash"), 0.01, K, sketch_size=s), want, "no tail")


# ---- the path: n / 2 rounds ------------------------------------------------------------------------------------------
def test_path_with_and_without_the_tail(ctx):
    from rabbittclust_amd import api
    n = 2000
    sk = S.path(n)
    want = G.kssd(sk, 0.05, K, False)
    assert want[4] == n // 2 and want[0][:5] == [1, 1, 1, 3, 3]
    dev = _set(ctx, sk, 4, "kssd")
    results = {}
    for tail in ("0", None, str(n + 1), "500"):
        with ctx.env(RTC_DEGREE_TAIL=tail):
            got = ctx.greedy_degree(dev, 0.05, K)
            c, path = _counters_fit(ctx, got), ctx.greedy_degree_last_path()
        _same(got, want, tail)
        results[tail] = got
        # every round decides the open vertex with the largest key and its two neighbours, and no other: a chain of n / 2 rounds
        assert c["rounds"] == n // 2, (tail, c)
        if tail == "0":
            assert not path & api.DEGREE_PATH_TAIL and c["tail_rounds"] == 0
        elif tail == "500":
            assert path & api.DEGREE_PATH_TAIL and 0 < c["tail_rounds"] < c["rounds"]
        else:  # the default lies above 2 000 as well: the tail kernel runs every round
            assert path & api.DEGREE_PATH_TAIL and c["tail_rounds"] == c["rounds"]
        assert path & api.DEGREE_PATH_WAVE and not path & api.DEGREE_PATH_WORKGROUP
    for tail, got in results.items():
        assert all(np.array_equal(a, b) for a, b in zip(got[:4], results["0"][:4])), tail


# ---- one rule each -------------------------------------------------------------------------------------------------
def test_small_graphs(ctx):
    for make in (S.star_and_clique, S.two_hubs, S.tie_in_j, S.both_sides):
        sk, edges = make()
        want = G.kssd(sk, S.GRAPH_THRESHOLD, K, False)
        assert want[1] == [len(x) for x in S.edges_to_lists(len(sk), edges)]
        for width in (4, 8):
            for tail in (None, "0"):
                with ctx.env(RTC_DEGREE_TAIL=tail):
                    got = ctx.greedy_degree(_set(ctx, sk, width, "kssd"), S.GRAPH_THRESHOLD, K)
                _same(got, want, (make.__name__, width, tail))
    got = ctx.greedy_degree(_set(ctx, S.star_and_clique()[0], 4, "kssd"), S.GRAPH_THRESHOLD, K)
    assert got[0].tolist() == [3, 3, 3, 3, 3, 3, 6, 6, 6, 6, 6] and got[4] == 2
    got = ctx.greedy_degree(_set(ctx, S.two_hubs()[0], 4, "kssd"), S.GRAPH_THRESHOLD, K)
    assert got[1][2] == got[1][5] == 4 and got[0].tolist() == [2, 2, 2, 2, 4, 2, 6, 7]  # the lower index wins, the other hub is a member
    got = ctx.greedy_degree(_set(ctx, S.tie_in_j()[0], 4, "kssd"), S.GRAPH_THRESHOLD, K)
    assert (got[0][2], got[2][2], got[3][2]) == (1, 2, 12)   # 2 / 12 == 4 / 24: the representative that is earlier in the order
    got = ctx.greedy_degree(_set(ctx, S.both_sides()[0], 4, "kssd"), S.GRAPH_THRESHOLD, K)
    assert (got[0][2], got[2][2], got[3][2]) == (1, 6, 12)   # the more similar representative, not the first


def test_minhash_truncation_decides(ctx):
    s = 100
    a1 = 10_000 + 10 * np.arange(s)
    low = np.concatenate([a1[:50], a1[-1] + 1 + np.arange(50)])    # shares a1's 50 lowest: they lead the union
    a2 = 90_000 + 10 * np.arange(s)
    high = np.concatenate([80_000 + np.arange(50), a2[50:]])       # shares a2's 50 highest: the union's first 100 hold none
    assert M.mash_counts(a1.tolist(), low.tolist(), s) == (50, 100) and M.mash_counts(a2.tolist(), high.tolist(), s) == (0, 100)
    sets = [a1, low, a2, high]
    for width in (4, 8):
        for thr in (0.03, 0.06):
            got = ctx.greedy_degree(_set(ctx, sets, width, "minhash"), thr, K, sketch_size=s)
            _same(got, G.minhash(sets, s, thr, K), (width, thr))
            assert got[0].tolist() == [0, 0, 2, 3] and got[1].tolist() == [1, 1, 0, 0]
            assert (got[2][1], got[3][1]) == (50, 100) and got[4] == 3


@pytest.mark.parametrize("c", [1, 37, 90, 127])
def test_threshold_on_a_distance_and_just_below(ctx, c):
    s = 128
    a = 1000 + 10 * np.arange(s)
    b = np.concatenate([a[:c], a[c:] + 5])  # the c lowest shared, the rest interleaved
    assert M.mash_counts(a.tolist(), b.tolist(), s) == (c, s)
    thr = M.distance(c, s, K)
    sk = _set(ctx, [a, b], 8, "minhash")
    got = ctx.greedy_degree(sk, thr, K, sketch_size=s)
    assert [x.tolist() for x in got[:4]] == [[0, 0], [1, 1], [0, c], [0, s]] and got[4] == 1
    got = ctx.greedy_degree(sk, float(np.nextafter(thr, 0)), K, sketch_size=s)
    assert [x.tolist() for x in got[:4]] == [[0, 1], [0, 0], [0, 0], [0, 0]] and got[4] == 2


# ---- long rows -------------------------------------------------------------------------------------------------------
def test_clique_of_4200(ctx):
    """The issue's set -- 4 200 sketches of 4 hashes sharing 2 of them.  It is a clique: one representative, and every member's
    row holds that one candidate, so it cannot reach the 256-lane path (tests/greedy_degree_sets.long_row says why no set of
    4 200 can, and test_long_row_takes_the_workgroup_path has one that does).  Kept for its 8.8 million pairs."""
    from rabbittclust_amd import api
    n = 4200
    sk = S.clique_4200(n)
    common = np.full((n, n), 2, dtype=np.int64)
    nbrs = G.neighbours_kssd_dense(common, [4] * n, 0.05, K)
    assert all(len(x) == n - 1 for x in nbrs)
    want = G.kssd(sk, 0.05, K, False, nbrs=nbrs)
    dev = _set(ctx, sk, 4, "kssd")
    got = ctx.greedy_degree(dev, 0.05, K)
    _same(got, want)
    c = _counters_fit(ctx, got)
    assert got[4] == 1 and c["kept_edges"] == n * (n - 1) // 2 and c["rounds"] == 1 and c["wave_rows"] == n - 1
    assert ctx.greedy_degree_last_path() & 3 == api.DEGREE_PATH_WAVE
    with ctx.env(RTC_DEGREE_BLOCK="1"):
        _same(ctx.greedy_degree(dev, 0.05, K), want, "block")
        assert ctx.greedy_degree_last_path() & 3 == api.DEGREE_PATH_WORKGROUP and ctx.greedy_degree_counters()["workgroup_rows"] == n - 1


def test_long_row_takes_the_workgroup_path(ctx):
    from rabbittclust_amd import api
    leaves = S.LONG_ROW_LEAVES
    assert leaves + 1 > api.DEGREE_WAVE_ROW
    sk, edges = S.long_row()
    n = len(sk)
    nbrs = G.neighbours_kssd(sk, S.LONG_ROW_THRESHOLD, K, False)
    assert nbrs == S.edges_to_lists(n, edges)
    want = G.kssd(sk, S.LONG_ROW_THRESHOLD, K, False, nbrs=nbrs)
    assert want[0][1] == 0 and want[4] == leaves + 1 and (want[2][1], want[3][1]) == (64, 2 * (64 + 2 * leaves) - 64)
    dev = _set(ctx, sk, 4, "kssd")
    got = ctx.greedy_degree(dev, S.LONG_ROW_THRESHOLD, K)
    _same(got, want)
    c = _counters_fit(ctx, got)
    # hub 1 has hub 0 and its own leaves for candidates: the one long row; the leaves of hub 0 have one candidate each
    assert (c["workgroup_rows"], c["wave_rows"], c["rounds"]) == (1, leaves, 2)
    assert ctx.greedy_degree_last_path() & 3 == api.DEGREE_PATH_WAVE | api.DEGREE_PATH_WORKGROUP
    with ctx.env(RTC_DEGREE_BLOCK="1"):
        _same(ctx.greedy_degree(dev, S.LONG_ROW_THRESHOLD, K), want, "block")
        c = ctx.greedy_degree_counters()
        assert (c["workgroup_rows"], c["wave_rows"]) == (leaves + 1, 0) and ctx.greedy_degree_last_path() & 3 == api.DEGREE_PATH_WORKGROUP


# ---- row chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kssd", "minhash"])
def test_row_chunks_keep_the_result(ctx, kind):
    n = 320
    sets = S.dense_candidates(n)
    thr, s = 0.02, 80
    dev = _set(ctx, sets, 4 if kind == "kssd" else 8, kind)
    args = dict(sketch_size=s) if kind == "minhash" else {}
    want = ctx.greedy_degree(dev, thr, K, **args)
    c1 = _counters_fit(ctx, want)
    assert c1["chunks"] == 1 and c1["candidate_edges"] == n * (n - 1) // 2 and 0 < c1["kept_edges"] < c1["candidate_edges"]
    if kind == "kssd":
        _same(want, G.kssd(sets, thr, K, False))
    assert 1 < want[4] < n
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        got = ctx.greedy_degree(dev, thr, K, **args)
        c2 = ctx.greedy_degree_counters()
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4] == want[4]
    assert c2["chunks"] >= 3 and all(c2[k] == c1[k] for k in ("candidate_edges", "merged", "kept_edges", "representatives", "rounds"))


def test_tail_leaves_a_dense_remainder_to_the_host(ctx):
    """320 genomes are open before the first round, with some 7 000 pairs between them: at the default the one workgroup takes
    them, at RTC_DEGREE_TAIL=400 they are few enough but their pairs (more than 4 * 400) are not, and the host's rounds go on"""
    from rabbittclust_amd import api
    sets = S.dense_candidates(320)
    dev = _set(ctx, sets, 4, "kssd")
    want = ctx.greedy_degree(dev, 0.02, K)
    c1 = _counters_fit(ctx, want)
    assert 4 * 400 < c1["kept_edges"] <= 4 * 4096 and c1["tail_rounds"] == c1["rounds"] >= 1
    assert ctx.greedy_degree_last_path() & api.DEGREE_PATH_TAIL
    with ctx.env(RTC_DEGREE_TAIL="400"):
        got = ctx.greedy_degree(dev, 0.02, K)
        c2 = _counters_fit(ctx, got)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4] == want[4]
    assert c2["rounds"] == c1["rounds"] and c2["rounds"] - c2["tail_rounds"] >= 1


# ---- tiny and failing inputs -----------------------------------------------------------------------------------------
def test_tiny_sets_and_error_returns(ctx):
    from rabbittclust_amd import api
    for width, kind, args in ((4, "kssd", {}), (8, "kssd", {}), (8, "minhash", dict(sketch_size=10))):
        empty = np.zeros(0, dtype=np.uint64)
        for host in ([], [np.arange(1, 11)], [np.arange(1, 11), np.arange(6, 16)], [np.arange(1, 11), np.arange(100, 110)],
                     [empty], [empty] * 5):
            got = ctx.greedy_degree(_set(ctx, host, width, kind), 0.05, K, **args)
            want = G.minhash(host, 10, 0.05, K) if kind == "minhash" else G.kssd(host, 0.05, K, width == 8)
            _same(got, want, (width, kind, len(host)))
            assert all(len(x) == len(host) for x in got[:4])
        got = ctx.greedy_degree(_set(ctx, [np.arange(1, 11), np.arange(6, 16)], width, kind), 0.05, K, **args)
        assert got[0].tolist() == [0, 0] and (got[2][1], got[3][1]) == ((5, 10) if kind == "minhash" else (5, 15))
        assert ctx.greedy_degree(_set(ctx, [empty] * 5, width, kind), 0.05, K, **args)[4] == 5
    sk = _set(ctx, [np.arange(10), np.arange(5, 15)], 8, "minhash")
    for thr, status in ((-0.1, api._lib.RTC_ERR_ARG), (float("nan"), api._lib.RTC_ERR_ARG), (1.0, api._lib.RTC_ERR_UNSUPPORTED)):
        with pytest.raises(api.RtcError) as ei:
            ctx.greedy_degree(sk, thr, K, sketch_size=10)
        assert ei.value.status == status, thr
    assert ctx.greedy_degree(sk, 0.999, K, sketch_size=10)[0].tolist() == [0, 0]
    for width in (4, 8):  # exp(-2 * 21) / (2 - ...) = 2.9e-19: jaccard_min <= 1e-12
        with pytest.raises(api.RtcError) as ei:
            ctx.greedy_degree(_set(ctx, [np.arange(1, 11), np.arange(6, 16)], width, "kssd"), 2.0, K)
        assert ei.value.status == api._lib.RTC_ERR_UNSUPPORTED and "1e-12" in str(ei.value)


# ---- the command line ------------------------------------------------------------------------------------------------
def _run(args, cwd, env=None):
    import subprocess
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _partition(path):
    clusters, cur = [], None
    for ln in open(path):
        if ln.startswith("the cluster"):
            cur = []
            clusters.append(cur)
        elif ln.startswith("\t"):
            cur.append(int(ln.split("\t")[2]))
    return sorted(tuple(sorted(c)) for c in clusters)


def _by_rep(rep):
    want = {}
    for i, r in enumerate(rep):
        want.setdefault(int(r), []).append(i)
    return sorted(tuple(sorted(c)) for c in want.values())


def test_cli_fast(oracle, tmp_path):
    tmp = str(tmp_path)
    L, thr = 2_000_000, 0.05  # large enough that the tuner keeps -k 21
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 3, L, seed=8)
    ks = [oracle.kssd_sketch(s, 21, 3) for s in seqs]
    order = sorted(range(len(ks)), key=lambda i: -len(ks[i]))  # the command line's size sort
    assert len({len(x) for x in ks}) == len(ks), "the sketch sizes must not tie (an unstable sort order)"
    sk = [np.asarray(ks[i], dtype=np.uint32) for i in order]
    want = G.kssd(sk, thr, 22, False)  # the command line's k for KSSD sketches: twice the half k-mer
    assert 1 < want[4] < len(sk)
    G_BIN = os.path.join(BIN, "clust-greedy")
    out, mj = os.path.join(tmp, "deg.out"), os.path.join(tmp, "m.json")
    base = [G_BIN, "--fast", "-l", "-i", lst, "-k", "21", "-d", str(thr), "-t", "4", "-e"]
    err = _run(base + ["--order", "degree", "-o", out], tmp, env={"RTC_METRICS_JSON": mj})
    smeta = [meta[i] for i in order]
    assert open(out).read() == G.print_result(G.clusters(want[0]), smeta)
    assert open(out + ".order.tsv").read() == G.order_tsv(want, [m[0] for m in smeta], 22, False)
    assert "-----write the processing order into: " + out + ".order.tsv" in err
    metrics = json.load(open(mj))
    for key in ("greedy_degree_pair_s", "greedy_degree_select_s", "greedy_degree_assign_s", "greedy_degree_rounds", "greedy_degree_edges"):
        assert key in metrics and metrics[key] >= 0, key
    assert metrics["greedy_degree_edges"] == sum(want[1]) // 2 and metrics["clusters"] == want[4] and metrics["greedy_degree_rounds"] >= 1
    # without the flag: the run as it was, and no order file
    plain = os.path.join(tmp, "plain.out")
    _run(base + ["-o", plain], tmp)
    flat, start, lens = oracle.to_csr(sk, dtype=np.uint32)
    ncl, rep = oracle.greedy_kssd(flat, start, lens, 22, thr)
    assert _partition(plain) == _by_rep(rep) and not os.path.exists(plain + ".order.tsv")


def test_cli_minhash(oracle, tmp_path):
    tmp = str(tmp_path)
    L, thr, s = 2_000_000, 0.05, 1000
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 3, L, seed=8)
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * L
    sk = oracle.sketch_minhash_batch(np.concatenate(seqs), off, 21, s)
    want = G.minhash(sk, s, thr, 21)  # from genome files the genomes keep the order of the list
    assert 1 < want[4] < len(sk)
    G_BIN = os.path.join(BIN, "clust-greedy")
    out = os.path.join(tmp, "deg.out")
    base = [G_BIN, "-l", "-i", lst, "-k", "21", "-s", str(s), "-d", str(thr), "-t", "4"]
    _run(base + ["--order", "degree", "-o", out], tmp)
    assert open(out).read() == G.print_result(G.clusters(want[0]), meta)
    assert open(out + ".order.tsv").read() == G.order_tsv(want, [m[0] for m in meta], 21, True)
    # the sketch folder it saved, --presketched: all genomes have one length, so the size sort keeps the order
    folder = [os.path.join(tmp, d) for d in os.listdir(tmp) if os.path.isdir(os.path.join(tmp, d)) and d[:2] == "20"]
    assert len(folder) == 1
    out2 = os.path.join(tmp, "pre.out")
    _run([G_BIN, "-l", "--presketched", folder[0], "-d", str(thr), "--order", "degree", "-o", out2], tmp)
    assert open(out2, "rb").read() == open(out, "rb").read()
    assert open(out2 + ".order.tsv", "rb").read() == open(out + ".order.tsv", "rb").read()
    # without the flag: the run as it was, and no order file
    plain = os.path.join(tmp, "plain.out")
    _run([G_BIN, "-l", "--presketched", folder[0], "-d", str(thr), "-o", plain], tmp)
    flat, start, lens = oracle.to_csr(sk)
    ncl, rep = oracle.greedy_minhash(flat, start, lens, s, 21, False, thr)
    assert _partition(plain) == _by_rep(rep) and not os.path.exists(plain + ".order.tsv")
