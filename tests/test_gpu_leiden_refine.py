"""GPU suite: rtc_leiden against tests/refleiden.py (the header's definition restated): labels, cluster count and the counters
that are no times, exactly, for both objectives."""
import numpy as np
import pytest

import leiden_sets
import refgraph
import refleiden
import reflouvain
from refleiden import CPM, MODULARITY

pytestmark = pytest.mark.gpu

RESOLUTIONS = (0.25, 0.5, 1.0, 2.0)
_SETS = dict(leiden_sets.hand_graphs(), paths=leiden_sets.paths_set(), random=leiden_sets.random_graph())
_WANT = {}


def _want(name, objective, resolution):
    """the restatement's answer, computed once"""
    key = (name, objective, resolution)
    if key not in _WANT:
        n, edges = _SETS[name]
        stats = {}
        labels, ncl, counters = refleiden.leiden(n, edges, resolution, objective, stats)
        _WANT[key] = (labels, ncl, counters, stats)
    return _WANT[key]


def _connected(n, edges, labels):
    """every community is connected over the records (all of them carry q >= 1)"""
    adj = [[] for _ in range(n)]
    for u, v, _ in edges:
        adj[u].append(v)
        adj[v].append(u)
    members = {}
    for x, c in enumerate(labels):
        members.setdefault(c, []).append(x)
    for ms in members.values():
        inside, seen, todo = set(ms), {ms[0]}, [ms[0]]
        while todo:
            for y in adj[todo.pop()]:
                if y in inside and y not in seen:
                    seen.add(y)
                    todo.append(y)
        if len(seen) != len(ms):
            return False
    return True


def _records(edges):
    from rabbittclust_amd import api
    rec = np.array(edges, dtype=np.int64).reshape(-1, 3)
    arr = np.zeros(len(edges), dtype=api.WEDGE_DT)
    arr["u"], arr["v"], arr["q"] = rec[:, 0], rec[:, 1], rec[:, 2]
    return arr


def test_sets_hold_the_cases():
    """on the CPU, through the restatement: the sets reach what the kernels have to get right"""
    labels, ncl, C, stats = _want("paths", MODULARITY, 1.0)
    assert C[0] >= 2 and C[1] >= 2 * C[0] and C[6] > 0 and stats["split"] > 0
    rows = stats["row_lengths"]
    assert max(rows) > 2100 and any(128 < r <= 2048 for r in rows) and any(0 < r <= 128 for r in rows)
    assert 1 < ncl < _SETS["paths"][0]
    assert _want("random", CPM, 0.5)[3]["ineligible"] > 0 and _want("pendant", CPM, 0.25)[3]["ineligible"] > 0
    labels, ncl, C, stats = _want("paths", CPM, 0.5)
    assert C[0] >= 2 and C[1] >= 2 * C[0] and C[6] > 0 and stats["split"] > 0 and max(stats["row_lengths"]) > 2100
    assert _want("path", MODULARITY, 1.0)[2][6] > 0


@pytest.mark.parametrize("resolution", RESOLUTIONS)
@pytest.mark.parametrize("objective", [CPM, MODULARITY])
@pytest.mark.parametrize("name", sorted(_SETS))
def test_leiden_equals_the_restatement(ctx, name, objective, resolution):
    n, edges = _SETS[name]
    labels, ncl, counters, _ = _want(name, objective, resolution)
    assert _connected(n, edges, labels)  # a property of these inputs, not of the definition
    got, quality = ctx.leiden(n, _records(edges), resolution, objective, return_quality=True)
    c = ctx.leiden_counters()
    print(name, objective, resolution, ctx.leiden_clusters, ncl, list(c.values())[:7], counters[:7])
    assert got.tolist() == labels
    assert ctx.leiden_clusters == ncl
    assert [c[k] for k in ("iterations", "levels", "move_rounds", "moves", "refine_rounds", "merges", "rejected")] == counters[:7]
    assert abs(quality - refleiden.quality(n, edges, labels, resolution, objective)) <= 1e-9
    assert c["total_ns"] >= c["move_ns"] + c["refine_ns"] > 0
    if objective == CPM and resolution >= 1.0:
        assert ncl == n and c["moves"] == 0


def test_leiden_small_inputs_and_refusals(ctx):
    from rabbittclust_amd import _lib
    dt = [("u", "<u4"), ("v", "<u4"), ("q", "<u4")]
    one = np.array([(0, 1, 1 << 19)], dtype=dt)
    assert ctx.leiden(3, np.zeros(0, dtype=dt), 1.0).tolist() == [0, 1, 2] and ctx.leiden_clusters == 3  # m = 0
    assert ctx.leiden_counters()["iterations"] == 0
    assert ctx.leiden(3, one, 0.25).tolist() == [0, 0, 1]
    for objective in (2, -1):
        with pytest.raises(_lib.RtcError) as e:
            ctx.leiden(3, one, 0.5, objective)
        assert e.value.status == _lib.RTC_ERR_ARG
    for bad in (0.0, -1.0, float("nan"), 70000.0):
        with pytest.raises(_lib.RtcError) as e:
            ctx.leiden(3, one, bad)
        assert e.value.status == _lib.RTC_ERR_ARG
    for rec in ((0, 3, 1), (0, 1, 0)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.leiden(3, np.array([rec], dtype=dt), 1.0)
        assert e.value.status == _lib.RTC_ERR_ARG
    heavy = np.array([(0, 1, 0xffffffff)] * ((1 << 13) + 1), dtype=dt)  # M2 = 2 (2^32 - 1) (2^13 + 1) >= 2^46
    with pytest.raises(_lib.RtcError) as e:
        ctx.leiden(3, heavy, 1.0)
    assert e.value.status == _lib.RTC_ERR_UNSUPPORTED
    below = np.array([(0, 1, 0xffffffff)] * (1 << 13), dtype=dt)  # 2^46 - 2^14
    assert ctx.leiden(3, below, 1.0, "modularity").tolist() == [0, 0, 1]


def test_louvain_is_unchanged_beside_leiden(ctx):
    """the two share their kernels: a Louvain call after a Leiden call still answers as its own restatement does"""
    n, edges = leiden_sets.paths_set()
    ctx.leiden(n, _records(edges), 0.5)
    labels, ncl, levels, rounds, _ = reflouvain.louvain(n, edges, 1.0)
    assert ctx.louvain(n, _records(edges), 1.0).tolist() == labels
    c = ctx.louvain_counters()
    assert (c["levels"], c["rounds"], ctx.louvain_clusters) == (levels, rounds, ncl) and c["global_rows"] > 0


def test_graph_then_leiden_on_families(ctx):
    """rtc_graph_build, the host's quantisation and rtc_leiden as the command line chains them"""
    from rabbittclust_amd import api, host
    from tests.test_gpu_leiden import KMER, THRESHOLD, _graph_sets
    for width in (4, 8):
        sets = _graph_sets(width == 8)
        sk = api.SketchSet.from_host(sets, ctx.device, k=KMER, kind="kssd", width=width)
        sizes = [len(s) for s in sets]
        edges = ctx.graph_build(sk, THRESHOLD, KMER, 70)
        weighted = refgraph.weighted(refgraph.edges(sets, THRESHOLD, KMER, 70), sets, KMER)
        assert [(int(e["u"]), int(e["v"])) for e in edges] == [(u, v) for u, v, _ in weighted]
        for objective, resolution in ((CPM, 0.5), (MODULARITY, 1.0)):
            rec, _ = host.leiden_quantise(edges["u"], edges["v"], [w for _, _, w in weighted], objective)
            expect, _ = refleiden.normalise_and_quantise(weighted, objective)
            assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in rec] == expect
            labels, ncl, counters = refleiden.leiden(len(sets), expect, resolution, objective)
            assert ctx.leiden(len(sets), rec, resolution, objective).tolist() == labels
            assert 1 < ncl < len(sets) and ctx.leiden_clusters == ncl


# ---- the command line ----
@pytest.mark.parametrize("objective", ["cpm", "modularity"])
def test_cli_leiden_save_graph_and_pregraph(oracle, tmp_path, objective):
    import json
    import os
    from tests.test_gpu_dbscan import BIN, _folders, _run, _write_fastas
    from tests.test_gpu_leiden import _print_result
    tmp = str(tmp_path)
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 12, 1_000_000, seed=9)  # 36 genomes in three families
    exe = os.path.join(BIN, "clust-leiden")
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]  # -k 17: what the KSSD tuner keeps for genomes of 1 Mbp
    obj = CPM if objective == "cpm" else MODULARITY
    out = os.path.join(tmp, "a.out")
    metrics = os.path.join(tmp, "metrics.json")
    os.environ["RTC_METRICS_JSON"] = metrics
    try:
        err = _run([exe, "--fast", "--leiden", "--objective", objective, "--resolution", "0.5", "-l", "-i", lst, "-k", "17", "-d", "0.08", "--knn", "10",
                    "--save-graph", "-t", "4", "-o", out], tmp)
    finally:
        del os.environ["RTC_METRICS_JSON"]
    assert "-----Algorithm: Leiden" in err and "(k=10)" in err
    assert ("-----Edge weights normalized: [" in err) == (objective == "cpm")
    edges = refgraph.edges(ks, 0.08, 17, 10)
    weighted = refgraph.weighted(edges, ks, 17)
    records, _ = refleiden.normalise_and_quantise(weighted, obj)
    labels, ncl, counters = refleiden.leiden(len(ks), records, 0.5, obj)
    assert open(out).read() == _print_result(refleiden.clusters_of(labels), meta)
    m = json.load(open(metrics))
    assert m["command"] == "clust-leiden" and m["leiden_edges"] == len(edges) and m["leiden_clusters"] == ncl
    assert m["leiden_iterations"] == counters[0] and m["leiden_levels"] == counters[1] and m["leiden_merges"] == counters[5]
    assert m["leiden_refine_s"] > 0 and m["leiden_louvain_s"] >= m["leiden_refine_s"] and m["leiden_graph_s"] > 0
    # --pregraph: Leiden on the file's weights at another resolution
    folder = _folders(tmp)
    assert len(folder) == 1
    lines = open(os.path.join(folder[0], "leiden.graph")).read().splitlines()
    assert lines[0] == "%d %d" % (len(ks), len(edges))
    parsed = [(int(a), int(b), float(w)) for a, b, w in (ln.split() for ln in lines[1:])]
    records2, _ = refleiden.normalise_and_quantise(parsed, obj)
    labels2, ncl2, _ = refleiden.leiden(len(ks), records2, 0.25, obj)
    out2 = os.path.join(tmp, "b.out")
    _run([exe, "--leiden", "--objective", objective, "--pregraph", folder[0], "--resolution", "0.25", "-o", out2], tmp)
    assert open(out2).read() == _print_result(refleiden.clusters_of(labels2), meta)
    assert ncl < len(ks)
