"""clust-leiden --minhash on the GPU: rtc_graph_build_mash against tests/refgraph_mash.py (the edge rule and the rank restated
on the union-truncated counts) on one set built around its edge cases (tests/graph_mash_sets.py) for both widths and a sketch
size on either side of the merge kernel's LDS staging, the row chunks, the strict threshold, the switches, the error returns,
and the command line end to end.  No tolerances: counts and labels are integers, the distances the host's on both sides."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import graph_mash_sets as S
from tests import refdbscan_mash as M
from tests import refgraph_mash as G

pytestmark = pytest.mark.gpu

K, T = S.KMER, S.THRESHOLD


@pytest.fixture(scope="module", params=[(256, 4), (256, 8), (1200, 4), (1200, 8)], ids=lambda p: "s%d-w%d" % p)
def case(request, ctx):
    from rabbittclust_amd import api
    s, width = request.param
    lists, trio, counts, want = S.case(s)
    sk = api.SketchSet.from_host(S.typed(lists, width), ctx.device, k=K, kind="minhash", width=width)
    return s, lists, trio, counts, want, sk


def _got(edges):
    from rabbittclust_amd import api
    return [(int(u), int(v), int(c), int(d)) for u, v, c, d in zip(edges["u"], edges["v"], edges["common"], api.graph_denom(edges))]


@pytest.mark.parametrize("s", [256, 1200])
def test_graph_mash_sets_hold_the_cases(s):
    lists, (p, r, q), counts, want = S.case(s)
    sizes = [len(x) for x in lists]
    assert len(lists) == 193 and sizes.count(0) == 2 and sizes[r] == 1 and sizes[p] == 2 and max(sizes) == s
    assert (s > 1024) == (sum(1 for x in sizes if x > 1024) >= 12)  # past the LDS staging, or all inside it
    live = 191
    assert len(counts) == live * (live - 1) // 2  # every pair of non-empty lists shares a hash
    per_node = {}
    for u, v, c, d in want[0]:
        per_node.setdefault(u, []).append((c, d))
    assert max(len(x) for x in per_node.values()) > 70
    assert any(len(x) > 70 and len(set(x)) < len(x) for x in per_node.values()), "no equal ranks in a long row"
    assert len(want[70]) < len(want[0]) and len(want[3]) < len(want[70]) and len(want[1]) < len(want[3])
    dist = {pair: M.distance(c, d, K) for pair, (c, d) in counts.items()}
    assert any(0.0 < x < T for x in dist.values()) and any(T <= x < 1.0 for x in dist.values())  # loose families on both sides
    assert any(d < s for _, _, _, d in want[0]) and any(d == s for _, _, _, d in want[0])  # short unions, and cut ones
    # P meets R at 1/2 and Q at 2/4: equal ratios from different counts; P is the first of the three
    assert p < r and p < q and counts[(p, r)] == (1, 2) and counts[(p, q)] == (2, 4)
    assert Fraction(1, 2) == Fraction(2, 4) and (p, min(r, q)) in {(u, v) for u, v, _, _ in want[1]}
    assert (p, max(r, q)) not in {(u, v) for u, v, _, _ in want[1]} and (p, max(r, q)) in {(u, v) for u, v, _, _ in want[3]}
    # a shared hash beyond the truncation alone: no edge at any threshold
    beyond = [pair for pair, (c, d) in counts.items() if c == 0]
    assert beyond and all(len(np.intersect1d(lists[u], lists[v])) >= 1 for u, v in beyond[:50])
    assert not {(u, v) for u, v, _, _ in G.edges(counts, 1.0, K)} & set(beyond)
    # 200 and 99 hashes: an edge, where the KSSD graph's size-ratio rule (99 / 200 < 0.5) would skip the pair
    a, b = sizes.index(200), sizes.index(99)
    assert (min(a, b), max(a, b)) in {(u, v) for u, v, _, _ in want[0]} and float(99) / 200 < 0.5


@pytest.mark.parametrize("knn_k", S.KNN)
def test_graph_build_mash_equals_the_restatement(ctx, case, knn_k):
    s, lists, trio, counts, want, sk = case
    edges = ctx.graph_build_mash(sk, s, T, K, knn_k)
    assert _got(edges) == want[knn_k]
    assert edges["pad"].tolist() == [d for _, _, _, d in want[knn_k]]  # the record's pad is the truncated denom
    c = ctx.graph_counters()
    live = sum(1 for x in lists if len(x))
    assert c["chunks"] == 1 and c["candidates"] == live * (live - 1) // 2
    assert c["passing"] == len(want[0]) and c["edges"] == len(want[knn_k])
    assert (c["nodes_cut"] > 0) == (knn_k > 0)
    assert c["passing"] <= c["merged"] <= c["candidates"]


def test_graph_build_mash_in_row_chunks(ctx, case):
    s, lists, trio, counts, want, sk = case
    with ctx.env(RTC_EDGE_BUDGET=str(64 * 193 + 1024)):
        for knn_k in (0, 3):
            assert _got(ctx.graph_build_mash(sk, s, T, K, knn_k)) == want[knn_k]
            c = ctx.graph_counters()
            assert c["chunks"] >= 3 and c["passing"] == len(want[0])


def test_graph_mash_threshold_is_strict(ctx, case):
    s, lists, trio, counts, want, sk = case
    u, v, c, d = want[0][len(want[0]) // 2]
    on = M.distance(c, d, K)
    expect = G.edges(counts, on, K)
    assert (u, v, c, d) not in expect and len(expect) > 0
    assert _got(ctx.graph_build_mash(sk, s, on, K)) == expect
    above = float(np.nextafter(on, 1.0))
    expect = G.edges(counts, above, K)
    assert (u, v, c, d) in expect
    assert _got(ctx.graph_build_mash(sk, s, above, K)) == expect
    # 1.0: every pair with a shared hash among the first s of its union, and none of those without
    every = sorted((a, b, x, y) for (a, b), (x, y) in counts.items() if x >= 1)
    assert G.edges(counts, 1.0, K) == every and len(every) < len(counts)
    assert _got(ctx.graph_build_mash(sk, s, 1.0, K)) == every


def test_graph_mash_switches_change_nothing(ctx, case):
    s, lists, trio, counts, want, sk = case
    ctx.graph_build_mash(sk, s, T, K, 3)
    base = ctx.graph_counters()
    assert base["merged"] < base["candidates"]  # the prefilter drops the pairs that share the top hash alone
    for serial, nopre in (("1", None), (None, "1"), ("1", "1")):
        with ctx.env(RTC_DBSCAN_MASH_SERIAL=serial, RTC_DBSCAN_MASH_NOPREFILTER=nopre):
            for knn_k in (0, 3):
                assert _got(ctx.graph_build_mash(sk, s, T, K, knn_k)) == want[knn_k], (serial, nopre, knn_k)
            c = ctx.graph_counters()
        assert c["merged"] == (c["candidates"] if nopre else base["merged"])
        assert all(c[k] == base[k] for k in ("candidates", "passing", "edges", "nodes_cut"))


def test_graph_mash_small_sets_overflow_and_refusals(ctx, case):
    from rabbittclust_amd import api, _lib
    s, lists, trio, counts, want, sk = case
    for n in (0, 1):
        small = api.SketchSet.from_host(S.typed(lists[:n], sk.width), ctx.device, k=K, kind="minhash", width=sk.width)
        assert len(ctx.graph_build_mash(small, s, T, K)) == 0
    with pytest.raises(_lib.RtcError) as e:
        ctx.graph_build_mash(sk, s, T, K, cap=len(want[0]) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.graph_edges_needed == len(want[0])
    assert _got(ctx.graph_build_mash(sk, s, T, K, cap=len(want[0]))) == want[0]
    for bad, status in ((0.0, _lib.RTC_ERR_ARG), (-0.1, _lib.RTC_ERR_ARG), (float("nan"), _lib.RTC_ERR_ARG),
                        (float(np.nextafter(1.0, 2.0)), _lib.RTC_ERR_UNSUPPORTED), (1.5, _lib.RTC_ERR_UNSUPPORTED)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.graph_build_mash(sk, s, bad, K)
        assert e.value.status == status, bad
    for size, kmer in ((0, K), (s, 0), (s, -3)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.graph_build_mash(sk, size, T, kmer)
        assert e.value.status == _lib.RTC_ERR_ARG, (size, kmer)


def test_kssd_call_after_a_minhash_call_reports_no_merges(ctx, case):
    s, lists, trio, counts, want, sk = case
    ctx.graph_build_mash(sk, s, T, K)
    assert ctx.graph_counters()["merged"] > 0
    ctx.graph_build(sk, T, K)  # the KSSD rule on the same lists: the call is what matters here
    c = ctx.graph_counters()
    assert c["merged"] == 0 and c["candidates"] == 191 * 190 // 2


def test_weights_helper_equals_the_restatement(ctx, case):
    from rabbittclust_amd import api
    import reflouvain
    s, lists, trio, counts, want, sk = case
    edges = ctx.graph_build_mash(sk, s, T, K, 70)
    rec, w = api.graph_weights_mash(edges, s, K, return_weights=True)
    expect = G.weighted(want[70], K)
    assert w.tolist() == [x for _, _, x in expect] and min(w) > 0.0
    assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in rec] == [(u, v, reflouvain.quantise(x)) for u, v, x in expect]


# ---- the command line ----
@pytest.fixture(scope="module")
def genomes(oracle, tmp_path_factory):
    """39 synthetic genomes in three families of 13 (a row of twelve higher-numbered neighbours is past --knn 10), their FASTA
    files, the oracle's MinHash sketches and the restated counts"""
    from tests.test_gpu_dbscan import _write_fastas
    tmp = str(tmp_path_factory.mktemp("graph_mash_cli"))
    L, s, k = 500_000, 128, 19  # -k 19: inside what the tuner keeps for genomes of 500 kbp (17 to 20)
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 13, L, seed=11)
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * L
    host = oracle.sketch_minhash_batch(np.concatenate(seqs), off, k, s)
    return tmp, lst, meta, s, k, G.counts(host, s)


def _cli(args, cwd, env=None):
    import subprocess
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


D, KNN = 0.1, 10  # --knn below 10 becomes 50


def test_cli_louvain_presketched_save_graph_and_pregraph(genomes):
    import reflouvain
    from tests.test_gpu_dbscan import BIN, _folders
    from tests.test_gpu_leiden import _print_result
    tmp, lst, meta, s, k, counts = genomes
    exe = os.path.join(BIN, "clust-leiden")
    n = len(meta)
    edges = G.edges(counts, D, k, KNN)
    assert len(edges) > 30 and len(edges) < len(G.edges(counts, D, k))  # the k-NN filter cuts
    weighted = G.weighted(edges, k)
    labels, ncl, levels, _, _ = reflouvain.louvain(n, [(u, v, reflouvain.quantise(w)) for u, v, w in weighted], 1.0)
    assert 1 < ncl < n
    d1 = os.path.join(tmp, "lv"); os.makedirs(d1)
    out, mj = os.path.join(tmp, "lv.out"), os.path.join(tmp, "lv.json")
    err = _cli([exe, "--minhash", "--louvain", "-l", "-i", lst, "-k", str(k), "-s", str(s), "-d", str(D), "--knn", str(KNN), "--save-graph", "-t", "4",
                "-o", out], d1, env={"RTC_METRICS_JSON": mj})
    assert "-----the kmerSize is: %d\n" % k in err and "(k=%d)" % KNN in err and "-----Building similarity graph (MinHash)..." in err
    assert open(out).read() == _print_result(reflouvain.clusters_of(labels), meta)
    m = json.load(open(mj))
    assert m["command"] == "clust-leiden" and m["sketch"] == "minhash"
    assert m["leiden_edges"] == len(edges) and m["leiden_clusters"] == ncl and m["leiden_levels"] == levels
    assert 0 < m["leiden_graph_merged"] <= n * (n - 1) // 2 and m["leiden_graph_s"] > 0
    # the folder clust-mst writes for the same genomes: the same sketch files, and the same result from it
    d2 = os.path.join(tmp, "mst"); os.makedirs(d2)
    _cli([os.path.join(BIN, "clust-mst"), "-l", "-i", lst, "-k", str(k), "-s", str(s), "-t", "4", "-o", os.path.join(tmp, "mst.out")], d2)
    f1, f2 = _folders(d1), _folders(d2)
    assert len(f1) == 1 and len(f2) == 1
    for name in ("hash.sketch", "info.sketch", "minhash.sketch.index"):
        assert open(os.path.join(f1[0], name), "rb").read() == open(os.path.join(f2[0], name), "rb").read(), name
    out2 = os.path.join(tmp, "lv2.out")
    _cli([exe, "--minhash", "--louvain", "--presketched", f2[0], "-d", str(D), "--knn", str(KNN), "-o", out2], tmp)
    assert open(out2, "rb").read() == open(out, "rb").read()
    # the graph file: the existing text layout, six significant digits; --pregraph is defined on those
    lines = open(os.path.join(f1[0], "leiden.graph")).read().splitlines()
    assert lines[0] == "%d %d" % (n, len(edges))
    assert lines[1:] == ["%d %d %s" % (u, v, "%g" % w) for u, v, w in weighted]
    parsed = [(int(a), int(b), reflouvain.quantise(float(w))) for a, b, w in (ln.split() for ln in lines[1:])]
    labels3 = reflouvain.louvain(n, parsed, 2.0)[0]
    out3 = os.path.join(tmp, "lv3.out")
    _cli([exe, "--minhash", "--louvain", "--pregraph", f1[0], "--resolution", "2.0", "-o", out3], tmp)
    assert open(out3).read() == _print_result(reflouvain.clusters_of(labels3), meta)


def test_cli_leiden_modularity(genomes):
    import refleiden
    from tests.test_gpu_dbscan import BIN
    from tests.test_gpu_leiden import _print_result
    tmp, lst, meta, s, k, counts = genomes
    exe = os.path.join(BIN, "clust-leiden")
    n = len(meta)
    edges = G.edges(counts, D, k, KNN)
    records, _ = refleiden.normalise_and_quantise(G.weighted(edges, k), refleiden.MODULARITY)
    labels, ncl, counters = refleiden.leiden(n, records, 1.0, refleiden.MODULARITY)
    assert 1 < ncl < n
    d1 = os.path.join(tmp, "ld"); os.makedirs(d1)
    out, mj = os.path.join(tmp, "ld.out"), os.path.join(tmp, "ld.json")
    err = _cli([exe, "--minhash", "--leiden", "--objective", "modularity", "-l", "-i", lst, "-k", str(k), "-s", str(s), "-d", str(D), "--knn", str(KNN),
                "-t", "4", "-o", out], d1, env={"RTC_METRICS_JSON": mj})
    assert "-----Algorithm: Leiden" in err
    assert open(out).read() == _print_result(refleiden.clusters_of(labels), meta)
    m = json.load(open(mj))
    assert m["leiden_edges"] == len(edges) and m["leiden_clusters"] == ncl and m["leiden_iterations"] == counters[0]
    assert "leiden_graph_merged" in m and m["sketch"] == "minhash"
