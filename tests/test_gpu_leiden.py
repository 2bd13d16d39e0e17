"""GPU suite: rtc_graph_build against tests/refgraph.py (the reference's edge rule restated) and rtc_louvain against
tests/reflouvain.py (the header's definition restated), both exactly."""
import numpy as np
import pytest

import community_sets
import refgraph
import reflouvain

pytestmark = pytest.mark.gpu

KMER = 21
THRESHOLD = 0.05  # an edge needs common / union above ~0.212


def _graph_sets(use64):
    """193 sketches (not a multiple of 64) that all share one hash, so every pair of non-empty ones is a candidate: a family
    of 80 close members with exact copies among them (one node with more than 70 passing neighbours, equal ranks), looser
    families, a sketch with its halves at size ratio exactly 1/2 and just under, unrelated sketches and two empty ones."""
    rng = np.random.default_rng(20240 + use64)
    everywhere = 5

    def fresh(m):
        return rng.integers(1000, (1 << 31) - 1, size=m, dtype=np.int64)

    def members(count, size, rate):
        base = fresh(size)
        out = []
        for _ in range(count):
            s = base.copy()
            flip = rng.random(size) < rate
            s[flip] = fresh(int(flip.sum()))
            out.append(s)
        return out
    big = members(74, 240, 0.04)
    big += [big[3].copy(), big[3].copy(), big[10].copy(), big[10].copy(), big[11].copy(), big[40].copy()]
    out = big + members(30, 200, 0.2) + members(30, 260, 0.45) + members(20, 150, 0.7)
    whole = np.sort(fresh(199))
    out += [whole, whole[:99], whole[:98]]  # with the shared hash: 200, 100 and 99 hashes
    out += [fresh(int(rng.integers(310, 400))) for _ in range(193 - 2 - len(out))]
    out = [np.append(s, everywhere) for s in out] + [np.zeros(0, dtype=np.int64)] * 2
    out = [out[i] for i in rng.permutation(len(out))]
    assert len(out) == 193
    hi = (1 << 40) if use64 else 0
    return [np.unique(s).astype(np.uint64 if use64 else np.uint32) + (np.uint64(hi) if use64 else np.uint32(0)) for s in out]


@pytest.fixture(scope="module", params=[4, 8])
def graph_case(request, ctx):
    from rabbittclust_amd import api
    width = request.param
    host = _graph_sets(width == 8)
    sk = api.SketchSet.from_host(host, ctx.device, k=KMER, kind="kssd", width=width)
    want = {k: refgraph.edges(host, THRESHOLD, KMER, k) for k in (0, 1, 3, 70)}
    return width, host, sk, want


def _got(edges):
    return [(int(e["u"]), int(e["v"]), int(e["common"])) for e in edges]


def test_graph_sets_hold_the_cases(graph_case):
    _, host, _, want = graph_case
    sizes = [len(s) for s in host]
    per_node = {}
    for u, v, c in want[0]:
        per_node.setdefault(u, []).append((c, sizes[u] + sizes[v] - c))
    assert max(len(r) for r in per_node.values()) > 70
    assert any(len(set(r)) < len(r) for r in per_node.values()), "no equal ranks"
    assert len(want[70]) < len(want[0]) and len(want[3]) < len(want[70]) and len(want[1]) < len(want[3])
    assert sizes.count(0) == 2
    by_size = {s: i for i, s in enumerate(sizes)}
    a, b, c = by_size[200], by_size[100], by_size[99]
    pairs = {(u, v) for u, v, _ in want[0]}
    assert (min(a, b), max(a, b)) in pairs and (min(a, c), max(a, c)) not in pairs  # ratio exactly 1/2 stays, 99 / 200 goes


@pytest.mark.parametrize("knn_k", [0, 1, 3, 70])
def test_graph_build_equals_the_restatement(ctx, graph_case, knn_k):
    width, host, sk, want = graph_case
    got = _got(ctx.graph_build(sk, THRESHOLD, KMER, knn_k))
    assert got == want[knn_k]
    c = ctx.graph_counters()
    n_live = sum(1 for s in host if len(s))
    assert c["chunks"] == 1 and c["candidates"] == n_live * (n_live - 1) // 2
    assert c["passing"] == len(want[0]) and c["edges"] == len(want[knn_k])
    assert (c["nodes_cut"] > 0) == (knn_k > 0)


def test_graph_build_in_row_chunks(ctx, graph_case):
    width, host, sk, want = graph_case
    with ctx.env(RTC_EDGE_BUDGET=str(64 * 193 + 1024)):
        for knn_k in (0, 3):
            assert _got(ctx.graph_build(sk, THRESHOLD, KMER, knn_k)) == want[knn_k]
            assert ctx.graph_counters()["chunks"] >= 3


def test_graph_threshold_is_strict(ctx, graph_case):
    width, host, sk, want = graph_case
    sizes = [len(s) for s in host]
    u, v, c = want[0][len(want[0]) // 2]
    on = refgraph.distance(c, sizes[u], sizes[v], KMER)
    expect = refgraph.edges(host, on, KMER)
    assert (u, v, c) not in expect and len(expect) > 0
    assert _got(ctx.graph_build(sk, on, KMER)) == expect
    above = np.nextafter(on, 1.0)
    expect = refgraph.edges(host, above, KMER)
    assert (u, v, c) in expect
    assert _got(ctx.graph_build(sk, above, KMER)) == expect
    # a threshold every sharing pair passes: only the size ratio is left
    assert _got(ctx.graph_build(sk, 1.5, KMER)) == refgraph.edges(host, 1.5, KMER)


def test_graph_small_sets_overflow_and_refusals(ctx, graph_case):
    from rabbittclust_amd import api, _lib
    width, host, sk, want = graph_case
    for n in (0, 1):
        small = api.SketchSet.from_host(host[:n], ctx.device, k=KMER, kind="kssd", width=width)
        assert len(ctx.graph_build(small, THRESHOLD, KMER)) == 0
    with pytest.raises(_lib.RtcError) as e:
        ctx.graph_build(sk, THRESHOLD, KMER, cap=len(want[0]) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.graph_edges_needed == len(want[0])
    assert _got(ctx.graph_build(sk, THRESHOLD, KMER, cap=len(want[0]))) == want[0]
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(_lib.RtcError) as e:
            ctx.graph_build(sk, bad, KMER)
        assert e.value.status == _lib.RTC_ERR_ARG


def test_graph_weight_equals_the_restatement_on_the_edges(graph_case):
    from rabbittclust_amd import api
    _, host, _, want = graph_case
    sizes = [len(s) for s in host]
    for u, v, c in want[0][::7]:
        assert api.graph_weight(c, sizes[u], sizes[v], KMER) == refgraph.weight(c, sizes[u], sizes[v], KMER)


# ---- Louvain ----
def _clique(vs, q):
    vs = list(vs)
    return [(a, b, q) for i, a in enumerate(vs) for b in vs[i + 1:]]


def _louvain_cases():
    one = 1 << 20
    cases = {}
    cases["empty"] = (5, [])
    cases["single_edge"] = (3, [(2, 1, 77)])
    cases["matching"] = (128, [(2 * i, 2 * i + 1, 5 + i % 3) for i in range(64)])  # the synchronous swap
    # the centre's row is past one wave's table; it has the highest number, so in round 0 it chooses among 300 communities
    cases["star_300"] = (301, [(300, i, 1 + (i * 7919) % 13) for i in range(300)])
    # past the workgroup's LDS table (rows of up to 2 048 entries): the table in global memory
    cases["star_2100"] = (2101, [(2100, i, 1 + (i * 7919) % 13) for i in range(2100)] + [(i, i + 1, 3) for i in range(0, 600, 2)])
    cases["two_cliques"] = (12, _clique(range(6), one) + _clique(range(6, 12), one) + [(5, 6, one)])
    ring = []
    for c in range(30):
        ring += _clique(range(5 * c, 5 * c + 5), one) + [(5 * c + 4, (5 * c + 5) % 150, one)]
    cases["ring"] = (150, ring)
    cases["duplicates_and_loops"] = community_sets.loops_and_duplicates()
    return cases


_CASES = _louvain_cases()
_RANDOM = {}


def _random_graph():
    if not _RANDOM:
        rng = np.random.default_rng(77)
        n, m = 2000, 20000
        u = rng.integers(0, n, size=m)  # 40 planted blocks by residue, seven edges in ten inside one
        v = np.where(rng.random(m) < 0.7, u % 40 + 40 * rng.integers(0, 50, size=m), rng.integers(0, n, size=m))
        q = rng.integers(1, 1 << 20, size=m)
        _RANDOM["edges"] = list(zip(u.tolist(), v.tolist(), q.tolist()))
        _RANDOM["n"] = n
    return _RANDOM["n"], _RANDOM["edges"]


def _check_louvain(ctx, n, edges, resolution):
    from rabbittclust_amd import api
    labels, ncl, levels, rounds, mod = reflouvain.louvain(n, edges, resolution)
    rec = np.array(edges, dtype=np.int64).reshape(-1, 3)
    arr = np.zeros(len(edges), dtype=api.WEDGE_DT)
    arr["u"], arr["v"], arr["q"] = rec[:, 0], rec[:, 1], rec[:, 2]
    got, got_mod = ctx.louvain(n, arr, resolution, return_modularity=True)
    c = ctx.louvain_counters()
    assert got.tolist() == labels
    assert ctx.louvain_clusters == ncl
    assert (c["levels"], c["rounds"]) == (levels, rounds)
    assert abs(got_mod - mod) <= 1e-12
    return c, labels


@pytest.mark.parametrize("name", sorted(_CASES))
def test_louvain_equals_the_restatement(ctx, name):
    n, edges = _CASES[name]
    c, labels = _check_louvain(ctx, n, edges, 1.0)
    if name == "star_300":
        assert c["long_rows"] > 0 and c["global_rows"] == 0
    if name == "star_2100":
        assert c["global_rows"] > 0
    if name == "ring":
        assert c["levels"] > 2 and len(set(labels)) == 15  # tests/test_cpu_leiden.py: the cliques merge in pairs
    if name == "two_cliques":
        assert labels == [0] * 6 + [1] * 6


@pytest.mark.parametrize("resolution", [0.5, 1.0, 2.0])
def test_louvain_random_graph(ctx, resolution):
    n, edges = _random_graph()
    c, labels = _check_louvain(ctx, n, edges, resolution)
    assert c["levels"] >= 2 and (resolution < 1.0 or len(set(labels)) == 40)  # at 0.5 the blocks merge into one


def test_louvain_refusals(ctx):
    from rabbittclust_amd import _lib
    for bad in (0.0, -1.0, float("nan"), 70000.0):
        with pytest.raises(_lib.RtcError) as e:
            ctx.louvain(3, np.array([(0, 1, 1)], dtype=[("u", "<u4"), ("v", "<u4"), ("q", "<u4")]), bad)
        assert e.value.status == _lib.RTC_ERR_ARG
    for rec in ((0, 3, 1), (0, 1, 0)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.louvain(3, np.array([rec], dtype=[("u", "<u4"), ("v", "<u4"), ("q", "<u4")]), 1.0)
        assert e.value.status == _lib.RTC_ERR_ARG


def test_graph_then_louvain_on_families(ctx, graph_case):
    """the two calls as the command line chains them: weights from rtc_graph_weight, quantised, against both restatements"""
    from rabbittclust_amd import api
    width, host, sk, want = graph_case
    sizes = [len(s) for s in host]
    edges = ctx.graph_build(sk, THRESHOLD, KMER, 70)
    rec = api.graph_weights(edges, sizes, KMER)
    expect = [(u, v, reflouvain.quantise(w)) for u, v, w in refgraph.weighted(want[70], host, KMER)]
    assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in rec] == expect
    labels = ctx.louvain(len(host), rec, 1.0)
    assert labels.tolist() == reflouvain.louvain(len(host), expect, 1.0)[0]


# ---- the command line ----
def _print_result(clusters, meta):
    """printKssdResult with -l: clusters in the order given, members as listed"""
    out = []
    for i, c in enumerate(clusters):
        out.append("the cluster %d is: \n" % i)
        out.extend("\t%5d\t%6d\t%12dnt\t%20s\t%20s\t%s\n" % (j, cur, meta[cur][1], meta[cur][0], meta[cur][2], meta[cur][3]) for j, cur in enumerate(c))
        out.append("\n")
    return "".join(out)


def test_cli_louvain_save_graph_and_pregraph(oracle, tmp_path):
    import json
    import os
    from tests.test_gpu_dbscan import BIN, _folders, _run, _write_fastas
    tmp = str(tmp_path)
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 12, 1_000_000, seed=9)  # 36 genomes in three families
    exe = os.path.join(BIN, "clust-leiden")
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]  # -k 17: what the KSSD tuner keeps for genomes of 1 Mbp
    out = os.path.join(tmp, "a.out")
    metrics = os.path.join(tmp, "metrics.json")
    os.environ["RTC_METRICS_JSON"] = metrics
    try:
        err = _run([exe, "--fast", "--louvain", "-l", "-i", lst, "-k", "17", "-d", "0.08", "--knn", "10", "--save-graph", "-t", "4", "-o", out], tmp)
    finally:
        del os.environ["RTC_METRICS_JSON"]
    assert "-----the kmerSize is: 17" in err and "(k=10)" in err
    edges = refgraph.edges(ks, 0.08, 17, 10)
    assert len(edges) > 30 and len(edges) < len(refgraph.edges(ks, 0.08, 17))  # the k-NN filter cuts
    weighted = refgraph.weighted(edges, ks, 17)
    labels, ncl, levels, _, _ = reflouvain.louvain(len(ks), [(u, v, reflouvain.quantise(w)) for u, v, w in weighted], 1.0)
    assert 1 < ncl < len(ks)
    assert open(out).read() == _print_result(reflouvain.clusters_of(labels), meta)
    m = json.load(open(metrics))
    assert m["command"] == "clust-leiden" and m["leiden_edges"] == len(edges) and m["leiden_levels"] == levels and m["leiden_clusters"] == ncl
    assert m["leiden_graph_s"] > 0 and m["leiden_louvain_s"] > 0 and -0.5 <= m["leiden_modularity"] <= 1.0
    # the graph file: the reference's text layout, six significant digits
    folder = _folders(tmp)
    assert len(folder) == 1
    lines = open(os.path.join(folder[0], "leiden.graph")).read().splitlines()
    assert lines[0] == "%d %d" % (len(ks), len(edges))
    assert lines[1:] == ["%d %d %s" % (u, v, "%g" % w) for u, v, w in weighted]
    # --pregraph: Louvain on the file's weights at another resolution
    parsed = [(int(a), int(b), reflouvain.quantise(float(w))) for a, b, w in (ln.split() for ln in lines[1:])]
    labels2, ncl2, _, _, _ = reflouvain.louvain(len(ks), parsed, 2.0)
    out2 = os.path.join(tmp, "b.out")
    _run([exe, "--louvain", "--pregraph", folder[0], "--resolution", "2.0", "-o", out2], tmp)
    assert open(out2).read() == _print_result(reflouvain.clusters_of(labels2), meta)
    # --presketched: k is the folder's half_k * 2 = 18
    out3 = os.path.join(tmp, "c.out")
    _run([exe, "--fast", "--louvain", "--presketched", folder[0], "-d", "0.08", "--knn", "10", "-o", out3], tmp)
    e3 = refgraph.edges(ks, 0.08, 18, 10)
    l3 = reflouvain.louvain(len(ks), [(u, v, reflouvain.quantise(w)) for u, v, w in refgraph.weighted(e3, ks, 18)], 1.0)[0]
    assert open(out3).read() == _print_result(reflouvain.clusters_of(l3), meta)
