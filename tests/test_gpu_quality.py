"""clust-mst --quality on the GPU: rtc_silhouette record for record, all eight fields, against the restatement (tests/refquality.py)
on the sets of tests/quality_sets.py -- rows at the path boundaries, tables whose probe chains wrap, the arithmetic's edges, means
that need 128 bits, more rows than a path's grid has workgroups -- with and without RTC_SIL_GLOBAL=1; rtc_cluster_quality against brute force over all pairs of sketches; and
the command line end to end."""
import ctypes as C
import functools
import json
import math
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from tests import quality_sets as S
from tests import refquality as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
ONE, NONE = R.ONE, R.NONE


@pytest.fixture
def switch(ctx, monkeypatch):
    def set_switch(name, v):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
        ctx.reload_options()
    set_switch("RTC_SIL_GLOBAL", None)
    yield set_switch
    monkeypatch.delenv("RTC_SIL_GLOBAL", raising=False)
    ctx.reload_options()


def _assert_same(got, want, what):
    assert got.dtype == want.dtype == R.SIL_DT and got.shape == want.shape, what
    if got.tobytes() == want.tobytes():
        return
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        if len(bad):
            x = int(bad[0])
            raise AssertionError("%s: %d records differ in %s, the first is vertex %d: got %s, want %s" % (what, len(bad), f, x, got[x], want[x]))


def _expected_rows(n, edges, labels, all_global):
    deg = np.zeros(n, dtype=np.int64)
    for u, v, _ in edges:
        deg[u] += 1
        deg[v] += 1
    rows = {S.WAVE: 0, S.WORKGROUP: 0, S.GLOBAL: 0}
    for x in np.flatnonzero((deg > 0) & (np.asarray(labels) >= 0)).tolist():
        rows[S.path_of(int(deg[x]), all_global)] += 1
    return rows


def _run_both(ctx, switch, n, edges, labels, want, what):
    """the set with and without RTC_SIL_GLOBAL=1: the same records, and the rows on the paths their lengths say"""
    for all_global in (False, True):
        switch("RTC_SIL_GLOBAL", 1 if all_global else None)
        got = ctx.silhouette(n, edges, labels)
        _assert_same(got, want, (what, all_global))
        rows = _expected_rows(n, edges, labels, all_global)
        c = ctx.silhouette_counters()
        assert (c["wave_rows"], c["workgroup_rows"], c["global_rows"]) == (rows[S.WAVE], rows[S.WORKGROUP], rows[S.GLOBAL]), (what, all_global, c)
        assert ctx.silhouette_last_path() == sum(p for p in rows if rows[p]), (what, all_global)
        assert c["records"] == len(edges) and c["entries"] == 2 * len(edges) and c["clustered"] == int((np.asarray(labels) >= 0).sum())
    switch("RTC_SIL_GLOBAL", None)


@functools.lru_cache(maxsize=None)
def _want(name, arg=None):
    n, edges, labels = getattr(S, name)() if arg is None else getattr(S, name)(arg)
    return n, edges, labels, R.silhouette(n, edges, labels)


# ---- rtc_silhouette ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", S.BOUNDARY_LENGTHS)
def test_rows_at_the_path_boundaries(ctx, switch, length):
    n, edges, labels, want = _want("boundary_star", length)
    switch("RTC_SIL_GLOBAL", None)
    ctx.silhouette(n, edges, labels)
    centre = S.path_of(length)
    assert centre == {128: S.WAVE, 129: S.WORKGROUP, 1024: S.WORKGROUP, 1025: S.GLOBAL}[length]
    c = ctx.silhouette_counters()
    assert ctx.silhouette_last_path() == S.WAVE | centre  # the leaves' rows are short
    assert (c["workgroup_rows"], c["global_rows"]) == (int(centre == S.WORKGROUP), int(centre == S.GLOBAL))
    _run_both(ctx, switch, n, edges, labels, want, ("boundary_star", length))


@pytest.mark.parametrize("log2_slots", sorted(S.COLLIDING_ROWS))
def test_tables_with_shared_home_slots_and_wrapping_chains(ctx, switch, log2_slots):
    n, edges, labels, want = _want("colliding_star", log2_slots)
    assert int(want[n - 1]["b_cluster"]) != NONE
    _run_both(ctx, switch, n, edges, labels, want, ("colliding_star", log2_slots))


@pytest.mark.parametrize("name", ["many_short_rows", "many_long_rows"])
def test_a_workgroup_scores_a_second_row(ctx, switch, name):
    """more rows on a path than row_kernel's grid there has workgroups (tests/test_cpu_quality.py: a table, a count array or a wave
    slot left from the turn before would show): short rows on the wave path and, under RTC_SIL_GLOBAL=1, the global one; rows of
    130 entries on the workgroup path"""
    num_cu = ctx.num_cu()
    t0 = time.perf_counter()
    n, edges, labels, want = _want(name, num_cu)
    t1 = time.perf_counter()
    _run_both(ctx, switch, n, edges, labels, want, name)
    t2 = time.perf_counter()
    rows = _expected_rows(n, edges, labels, False)  # _run_both held the counters of both calls to these
    assert ctx.silhouette_counters()["global_rows"] == sum(rows.values())  # the last call: every row on the global path
    print("%s: n %d, %d records, rows %s, all on the global path %d; set and restatement %.2f s, both GPU calls with their checks %.3f s"
          % (name, n, len(edges), rows, sum(rows.values()), t1 - t0, t2 - t1))
    if name == "many_short_rows":
        assert rows[S.WAVE] > S.WGS_PER_CU[S.WAVE] * num_cu and rows[S.WORKGROUP] == rows[S.GLOBAL] == 0
        assert rows[S.WAVE] > S.WGS_PER_CU[S.GLOBAL] * num_cu  # the rows of the global path under RTC_SIL_GLOBAL=1
    else:
        assert rows[S.WORKGROUP] > S.WGS_PER_CU[S.WORKGROUP] * num_cu and rows[S.WAVE] == rows[S.GLOBAL] == 0


@pytest.mark.parametrize("name", ["arithmetic", "one_cluster", "singletons"])
def test_arithmetic_and_labels(ctx, switch, name):
    n, edges, labels, want = _want(name)
    if name == "one_cluster":
        assert (want["b_den"] == 0).all() and (want["a_den"] == n - 1).all()
    if name == "singletons":
        assert (want["a_den"] == 0).all() and (want["far_q"] == 0).all() and (want["b_den"] > 0).all()
    _run_both(ctx, switch, n, edges, labels, want, name)


def test_random_graphs_with_noise_and_the_empty_input(ctx, switch):
    for seed, n in ((1, 3), (3, 12), (6, 40), (7, 40), (100, 36)):
        n, edges, labels = S.random_graph(seed, n, p_edge=(0.1, 0.3, 0.6, 1.0)[seed % 4], n_clusters=1 + seed % 5, lonely_cluster=seed == 100)
        _run_both(ctx, switch, n, edges, labels, R.silhouette(n, edges, labels), ("random", seed))
    # records, but every vertex unclustered; vertices, but no record; nothing at all
    n, edges, _ = S.random_graph(3, 12)
    _run_both(ctx, switch, n, edges, np.full(n, -1), R.silhouette(n, edges, np.full(n, -1)), "all noise")
    lab = np.array([4, 4, -1, 0, 4])
    _run_both(ctx, switch, 5, [], lab, R.silhouette(5, [], lab), "no record")
    assert len(ctx.silhouette(0, [], np.zeros(0, dtype=np.int32))) == 0
    c = ctx.silhouette_counters()
    assert c["records"] == c["clustered"] == c["clusters"] == 0 and ctx.silhouette_last_path() == 0


def test_means_that_need_128_bits(ctx, switch):
    """n = 2^23 + 260, the size the issue names: a GPU call takes well under a second, most of it the copy of the records.  The
    cross products of vertex 0 straddle 2^64 (tests/test_cpu_quality.py shows that a 64-bit product and a double each pick the
    other cluster)."""
    n, edges, labels, want = _want("past_64_bits")
    p1, p2 = S.big_products(n, edges, labels, 0)
    assert p2 < (1 << 64) < p1 and (p1 & ((1 << 64) - 1)) < (p2 & ((1 << 64) - 1)) and float(p1) == float(p2)
    assert int(want[0]["b_cluster"]) == 3 and int(want[0]["b_den"]) == (1 << 22) + 2
    _run_both(ctx, switch, n, edges, labels.astype(np.int32), want, "past_64_bits")
    c = ctx.silhouette_counters()
    assert c["clustered"] == n and c["clusters"] == 3


def test_argument_errors_leave_the_context_usable(ctx, switch):
    from rabbittclust_amd import _lib, api
    n, edges, labels, want = _want("arithmetic")
    lab = np.zeros(4, dtype=np.int32)
    bad = [([(0, 0, 1)], lab, "record 0"), ([(0, 1, 1), (0, 4, 1)], lab, "record 1"), ([(4, 0, 1)], lab, "record 0"),
           ([(0, 1, 3), (2, 3, ONE + 1)], lab, "record 1"), ([(0, 1, 5), (2, 3, 1), (1, 0, 6)], lab, "record 2"),
           ([(0, 1, 5), (0, 1, 5)], lab, "record 1"), ([(0, 1, 5)], np.array([0, 1, 4, -1], dtype=np.int32), "vertex 2"),
           ([(0, 1, 5), (1, 0, 5)], np.array([-1, -1, 0, 0], dtype=np.int32), "record 1")]  # a pair given twice between unclustered vertices too
    for e, l, names in bad:
        with pytest.raises(ValueError):
            R.silhouette(4, e, l)
        with pytest.raises(_lib.RtcError) as err:
            ctx.silhouette(4, e, l)
        assert err.value.status == _lib.RTC_ERR_ARG and names in str(err.value), (e, str(err.value))
        _assert_same(ctx.silhouette(n, edges, labels), want, "after an error")
    out = np.zeros(4, dtype=api.SIL_DT)
    e = np.array([(0, 1, 5)], dtype=api.WEDGE_DT)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert ctx.lib.rtc_silhouette(ctx.h, 0x7fffffff, p(e), 1, p(lab), p(out)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_silhouette(ctx.h, 4, None, 1, p(lab), p(out)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_silhouette(ctx.h, 4, p(e), 1, None, p(out)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_silhouette(ctx.h, 4, p(e), 1, p(lab), None) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_silhouette(None, 4, p(e), 1, p(lab), p(out)) == _lib.RTC_ERR_ARG
    _assert_same(ctx.silhouette(n, edges, labels), want, "after the argument errors")


# ---- rtc_cluster_quality -------------------------------------------------------------------------------------------------------
SKETCH_SEED = {4: 41, 8: 42}  # chosen on the CPU so that the preconditions below hold
THRESHOLD, KMER = 0.05, 21


def _cut_labels(n, mst, threshold):
    """the clusters of an MST cut at the threshold, every genome labelled by the smallest member of its cluster"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in mst:
        if float(e["dist"]) <= threshold:
            a, b = find(int(e["preNode"])), find(int(e["sufNode"]))
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


@pytest.mark.parametrize("width,kind", [(4, "kssd"), (8, "minhash")])
def test_cluster_quality_against_brute_force(ctx, switch, width, kind):
    from rabbittclust_amd import _lib, api
    sketches, small, big = S.family_sketches(SKETCH_SEED[width], width)
    n = len(sketches)
    assert n == 60 and min(len(s) for s in sketches) == 0
    # the pair the MST's size-ratio rule drops: one sketch inside another more than ten times its size
    assert len(sketches[small]) == 12 and len(sketches[big]) > 120 and len(np.intersect1d(sketches[small], sketches[big])) == 12
    assert int(2.0 * math.exp(THRESHOLD * (KMER - 1)) - 1.0) * 12 < len(sketches[big])  # max <= radio * min fails
    sk = api.SketchSet.from_host(sketches, ctx.device, k=KMER, kind=kind, width=width)
    labels = _cut_labels(n, ctx.mst(sk, THRESHOLD), THRESHOLD)
    noisy = labels.copy()
    noisy[[1, 17, 33, small]] = -1
    for lab in (labels, noisy):
        want, edges = R.cluster_quality(sketches, lab, KMER, api.linkage_distance)
        sizes = np.bincount(lab[lab >= 0])
        assert (sizes >= 2).sum() >= 2 and (want["b_cluster"] != NONE).any() and ((want["far_q"] < ONE) & (want["a_den"] > 0)).any()
        assert any({u, v} == {small, big} and q < ONE for u, v, q in edges)
        for all_global, threads in ((False, 1), (True, 3)):
            switch("RTC_SIL_GLOBAL", 1 if all_global else None)
            ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, threads))
            got = ctx.cluster_quality(sk, lab, KMER)
            ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 1))
            _assert_same(got, want, (kind, all_global))
            c = ctx.cluster_quality_counters()
            rows = _expected_rows(n, edges, lab, all_global)
            assert c["chunks"] >= 1 and c["candidates"] == len(edges) and c["clusters"] == len(sizes[sizes > 0])
            assert (c["wave_rows"], c["workgroup_rows"], c["global_rows"]) == (rows[S.WAVE], rows[S.WORKGROUP], rows[S.GLOBAL])
            assert c["total_ns"] >= c["pair_ns"] + c["distance_ns"] + c["score_ns"] > 0
        switch("RTC_SIL_GLOBAL", None)
        # the same records from the same pairs through rtc_silhouette
        _assert_same(ctx.silhouette(n, edges, lab), want, (kind, "records"))
    with pytest.raises(_lib.RtcError) as e:
        ctx.cluster_quality(sk, labels, 0)
    assert e.value.status == _lib.RTC_ERR_ARG
    bad = labels.copy()
    bad[5] = n
    with pytest.raises(_lib.RtcError) as e:
        ctx.cluster_quality(sk, bad, KMER)
    assert e.value.status == _lib.RTC_ERR_ARG and "vertex 5" in str(e.value)
    sk.width = 3
    with pytest.raises(_lib.RtcError) as e:
        ctx.cluster_quality(sk, labels, KMER)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = width
    _assert_same(ctx.cluster_quality(sk, labels, KMER), R.cluster_quality(sketches, labels, KMER, api.linkage_distance)[0], "after the errors")


def test_cluster_quality_in_row_chunks(ctx, switch):
    """every sketch shares a hash with every other: under RTC_EDGE_BUDGET=1 (raised to 64 n + 1 024) the whole triangle of
    candidates comes in several row chunks, every pair once"""
    from rabbittclust_amd import api
    sketches, labels = S.dense_sketches()
    n = len(sketches)
    want, edges = R.cluster_quality(sketches, labels, KMER, api.linkage_distance, matrix=True)
    assert len(edges) == n * (n - 1) // 2 > 2 * (64 * n + 1024)
    sk = api.SketchSet.from_host(sketches, ctx.device, k=KMER, kind="kssd", width=4)
    _assert_same(ctx.cluster_quality(sk, labels, KMER), want, "one chunk")
    assert ctx.cluster_quality_counters()["chunks"] == 1
    with ctx.env(RTC_EDGE_BUDGET="1"):
        got = ctx.cluster_quality(sk, labels, KMER)
        c = ctx.cluster_quality_counters()
    _assert_same(got, want, "row chunks")
    assert c["chunks"] > 2 and c["candidates"] == len(edges)
    assert c["workgroup_rows"] == int((labels >= 0).sum()) and c["wave_rows"] == c["global_rows"] == 0  # rows of n - 1 entries


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 500_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """12 genomes of 0.5 Mbp, listed in an order that scatters them: families of 4, 3 and 2 whose bases are copies of one root,
    6 % mutated each -- so the families share k-mers but lie apart -- every member 0.4 % from its base, and three strangers"""
    tmp = str(tmp_path_factory.mktemp("quality_fa"))
    rng = np.random.default_rng(29)
    root = rng.integers(0, 4, size=L)
    seqs = []
    for size in (4, 3, 2):
        base = _mutate(rng, root, 0.06)
        seqs += [_mutate(rng, base, 0.004) for _ in range(size)]
    seqs += [rng.integers(0, 4, size=L) for _ in range(3)]
    order = rng.permutation(len(seqs)).tolist()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths = []
    for g, o in enumerate(order):
        p = os.path.join(tmp, f"g{g:02d}.fna")
        with open(p, "wb") as f:
            f.write(f">s{g} genome {g}\n".encode() + acgt[seqs[o]].tobytes() + b"\n")
        paths.append(p)
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return {"list": lst, "paths": paths}


def _run(args, cwd, env=None):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _parse_clusters(path):
    clusters = []
    for ln in open(path):
        if ln.startswith("the cluster"):
            clusters.append([])
        elif ln.startswith("\t"):
            clusters[-1].append(int(ln.split("\t")[2]))
    return clusters


def _saved_sketches(folder, fast, n):
    """the hash sets of a sketch folder: kssd.hash.sketch (20 bytes, then a u64 count and u32 hashes a genome) or hash.sketch (13
    bytes, then a u64 count and u64 hashes a genome)"""
    raw = open(os.path.join(folder, "kssd.hash.sketch" if fast else "hash.sketch"), "rb").read()
    pos, out = (20 if fast else 13), []
    for _ in range(n):
        (cnt,) = struct.unpack_from("<Q", raw, pos)
        pos += 8
        out.append(np.frombuffer(raw, dtype="<u4" if fast else "<u8", count=cnt, offset=pos).copy())
        pos += (4 if fast else 8) * cnt
    assert pos == len(raw)
    return out


def _check_reports(out, metrics, sketches, names):
    from rabbittclust_amd import api
    m = json.load(open(metrics))
    clusters = _parse_clusters(out)
    labels = np.zeros(len(names), dtype=np.int32)
    for c, mem in enumerate(clusters):
        labels[mem] = c
    want, edges = R.cluster_quality(sketches, labels, int(m["kmer_size"]), api.linkage_distance)
    want_q, want_s = R.reports(names, clusters, want)
    assert open(out + ".quality.tsv").read() == want_q
    assert open(out + ".silhouette.tsv").read() == want_s
    for key in ("quality_pair_s", "quality_distance_s", "quality_score_s", "quality_candidates", "quality_silhouette_mean"):
        assert key in m, key
    assert m["quality_candidates"] == len(edges)
    mean = sum(R.value(want[g]) for g in range(len(names))) / len(names)
    assert abs(m["quality_silhouette_mean"] - mean) < 1e-9
    return clusters, want


@pytest.mark.parametrize("mode", ["fast", "minhash"])
def test_cli_writes_the_reports(genomes, tmp_path, mode):
    tmp = str(tmp_path)
    fast = mode == "fast"
    M = os.path.join(BIN, "clust-mst")
    paths = genomes["paths"]
    args = ["-l", "-i", genomes["list"], "-d", "0.05", "-t", "4"] + (["--fast", "-k", "17"] if fast else ["-k", "21", "-s", "1000"])
    d1 = os.path.join(tmp, "plain"); os.makedirs(d1)
    d2 = os.path.join(tmp, "q"); os.makedirs(d2)
    plain, out, mj = os.path.join(tmp, "plain.cluster"), os.path.join(tmp, "result.cluster"), os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", plain, "-e"], d1)
    err = _run([M] + args + ["-o", out, "--quality"], d2, env={"RTC_METRICS_JSON": mj})
    assert open(out, "rb").read() == open(plain, "rb").read()  # the plain result, byte for byte
    assert not os.path.exists(plain + ".quality.tsv") and not os.path.exists(plain + ".silhouette.tsv")
    assert out + ".quality.tsv\n" in err and out + ".silhouette.tsv\n" in err
    folder = [os.path.join(d2, x) for x in os.listdir(d2) if os.path.isdir(os.path.join(d2, x))]
    assert len(folder) == 1
    sketches = _saved_sketches(folder[0], fast, len(paths))
    clusters, want = _check_reports(out, mj, sketches, paths)
    assert sorted(len(c) for c in clusters) == [1, 1, 1, 2, 3, 4]
    # the families share k-mers, so each sees a nearest cluster; a cluster names none exactly when it shares no hash with another (a
    # stranger may share a chance hash or two with a family)
    rows = [ln.split("\t") for ln in open(out + ".quality.tsv").read().split("\n")[1:-2]]
    assert all(r[7] != "-" for r in rows if int(r[1]) > 1) and all((r[7] == "-") == (r[6] == "1.000000") for r in rows), rows
    assert any(r[7] == "-" for r in rows)
    assert all(float(r[2]) > 0.5 for r in rows if int(r[1]) > 1)  # tight families far from each other
    # the same from the saved folder, with the tree flags and the other refinements beside it
    out2, mj2 = os.path.join(tmp, "p.cluster"), os.path.join(tmp, "p.json")
    extra = ["--linkage", "complete", "--nj-tree", "--linkage-matrix"] + (["--dedup-dist", "0.01"] if fast else [])
    pre = [M] + (["--fast"] if fast else []) + ["--presketched", folder[0], "-l", "-d", "0.05"]
    plain2 = os.path.join(tmp, "plain2.cluster")
    _run(pre + ["-o", plain2], tmp)
    _run(pre + ["-o", out2, "--quality"] + extra, tmp, env={"RTC_METRICS_JSON": mj2})
    for suffix in ("", ".quality.tsv", ".silhouette.tsv", ".complete", ".complete.linkage.txt", ".nj.newick", ".linkage.txt") + ((".dedup",) if fast else ()):
        assert os.path.exists(out2 + suffix), suffix
    assert open(out2, "rb").read() == open(plain2, "rb").read()
    _check_reports(out2, mj2, sketches, paths)
    assert open(out2 + ".quality.tsv").read() == open(out + ".quality.tsv").read()
