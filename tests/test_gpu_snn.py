"""rtc_graph_snn on the GPU against tests/refsnn.py, record for record: the cases on paper, records as a file may hold them,
random graphs, rows past one and two strides of a wave, hub rows on both sides of the two path boundaries, every set again with
the switch that forces the global path, the counters, the errors, and clust-leiden --snn through the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import refsnn as R
from tests import snn_sets as S

pytestmark = pytest.mark.gpu

SETS = sorted(S.every_set())


def _got(ctx, n, rec):
    u = np.array([r[0] for r in rec], dtype=np.uint32)
    v = np.array([r[1] for r in rec], dtype=np.uint32)
    shared, du, dv, fl = ctx.graph_snn(n, u, v)
    return list(zip(shared.tolist(), du.tolist(), dv.tolist(), fl.tolist()))


def _check(ctx, name):
    n, rec = S.every_set()[name]
    assert _got(ctx, n, rec) == S.expected(name), name
    c = ctx.graph_snn_counters()
    edges, triangles, probes, proper = S.expected_counters(name)
    assert (c["records"], c["edges"], c["triangles"], c["probes"]) == (len(rec), edges, triangles, probes), name
    assert c["wave_records"] + c["workgroup_records"] + c["global_records"] == proper, name
    assert c["total_ns"] >= c["adjacency_ns"] + c["count_ns"] > 0
    return c


@pytest.mark.parametrize("name", SETS)
def test_snn_equals_the_restatement(ctx, name):
    from rabbittclust_amd import api
    c = _check(ctx, name)
    assert (c["wave_records"], c["workgroup_records"], c["global_records"]) == S.expected_paths(name)
    want = (api.SNN_PATH_WAVE if c["wave_records"] else 0) | (api.SNN_PATH_WORKGROUP if c["workgroup_records"] else 0) | \
           (api.SNN_PATH_GLOBAL if c["global_records"] else 0)
    assert ctx.graph_snn_last_path() == want


def test_paper_weights(ctx):
    from rabbittclust_amd import api
    for name, (num, den) in S.PAPER_WEIGHTS.items():
        n, rec = S.every_set()[name]
        for s, du, dv, fl in _got(ctx, n, rec):
            assert api.snn_weight(s, du, dv) == num / den and fl == 0, name
    n, rec = S.every_set()["two_k40"]
    got = _got(ctx, n, rec)
    assert got[-1] == (0, 40, 40, 0) and api.snn_weight(*got[-1][:3]) == 2 / 80  # the bridge
    assert all(g == (38, 39, 39, 0) or g[:3] in ((38, 39, 40), (38, 40, 39)) for g in got[:-1])
    assert all(s == 128 for s, _, _, _ in _got(ctx, *S.every_set()["k130"]))
    assert all(g == (0, 65, 65, 0) for g in _got(ctx, *S.every_set()["k65_65"]))


@pytest.mark.parametrize("row", S.hub_rows())
def test_hub_rows_at_the_path_boundaries(ctx, row):
    name = "hub_%d" % row
    n, rec = S.every_set()[name]
    want = S.expected(name)
    assert want[0] == (4, row, 5, 0) and sum(1 for w in want[:row] if w[0] == 4) == row - row % 5  # every hub edge into a K5
    assert all(w[0] == 0 for w in want[row - row % 5:row])  # the leaves that fill the row
    _check(ctx, name)
    assert ctx.graph_snn_last_path() == S.hub_path(row)


@pytest.mark.parametrize("name", SETS)
def test_global_switch_gives_identical_counts(ctx, name):
    from rabbittclust_amd import api
    with ctx.env(RTC_SNN_GLOBAL="1"):
        c = _check(ctx, name)
        assert c["wave_records"] == 0 and c["workgroup_records"] == 0 and c["global_records"] == S.expected_counters(name)[3]
        assert ctx.graph_snn_last_path() == api.SNN_PATH_GLOBAL
    _check(ctx, "k5")
    assert ctx.graph_snn_last_path() == api.SNN_PATH_WAVE


def _tiled(ctx, name, keep, reps):
    """the records of a set for which keep(u, v) holds, reps times over, behind the others: the graph is the set's, so every copy
    of a record has the record's answer"""
    n, rec = S.every_set()[name]
    want = S.expected(name)
    many = [i for i, r in enumerate(rec) if keep(*r)]
    once = sorted(set(range(len(rec))) - set(many))
    order = np.array(once + many * reps)
    u = np.array([r[0] for r in rec], dtype=np.uint32)[order]
    v = np.array([r[1] for r in rec], dtype=np.uint32)[order]
    got = np.stack(ctx.graph_snn(n, u, v), axis=1)
    assert np.array_equal(got, np.array(want, dtype=np.uint32)[order]), name
    c = ctx.graph_snn_counters()
    edges, triangles, _, _ = S.expected_counters(name)
    assert (c["records"], c["edges"], c["triangles"]) == (len(order), edges, triangles)  # the copies are no new edges
    return c, len(many) * reps


def test_more_slices_than_workgroups(ctx):
    """every count launch strides its workgroups over the slices of its path: enough copies of a set's records give every
    workgroup of a launch a second slice, on the device's own CU count"""
    k = S.constants()
    cus = ctx.num_cu()
    n_k130 = len(S.every_set()["k130"][1])
    wave_room = cus * k["SNN_WAVE_WGS_PER_CU"] * 64
    c, copies = _tiled(ctx, "k130", lambda u, v: True, wave_room // n_k130 + 1)
    assert c["wave_records"] == copies > wave_room and c["workgroup_records"] == c["global_records"] == 0
    row = S.boundaries()[0] + 1  # the hub's records take the workgroup path, the K5 edges one wave
    block_room = cus * k["SNN_BLOCK_WGS_PER_CU"] * 256
    c, copies = _tiled(ctx, "hub_%d" % row, lambda u, v: u == 0, block_room // row + 1)
    assert c["workgroup_records"] == copies > block_room and c["wave_records"] == 10 * (row // 5) and c["global_records"] == 0
    global_room = cus * k["SNN_GLOBAL_WGS_PER_CU"] * 256
    with ctx.env(RTC_SNN_GLOBAL="1"):
        c, copies = _tiled(ctx, "k130", lambda u, v: True, global_room // n_k130 + 1)
        assert c["global_records"] == copies > global_room and c["wave_records"] == c["workgroup_records"] == 0


def test_nothing_to_do_and_errors(ctx):
    from rabbittclust_amd import _lib, api
    empty = np.zeros(0, dtype=np.uint32)
    assert all(a.size == 0 for a in ctx.graph_snn(5, empty, empty))  # m == 0
    assert ctx.graph_snn_counters()["records"] == 0 and ctx.graph_snn_last_path() == 0
    for u, v in (([0, 2], [1, 0]), ([0, 0], [1, 2]), ([0], [0xffffffff])):
        with pytest.raises(_lib.RtcError) as e:
            ctx.graph_snn(2, u, v)
        assert e.value.status == _lib.RTC_ERR_ARG
    with pytest.raises(_lib.RtcError) as e:
        ctx.graph_snn((1 << 31) - 1, [0], [1])
    assert e.value.status == _lib.RTC_ERR_ARG
    rec = np.zeros(1, dtype=api.WEDGE_DT)
    rec["v"] = 1
    out = np.full(1, 0xee, dtype=api.SNN_DT)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctx.lib.rtc_graph_snn(ctx.h, 2, None, 1, ptr(out)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_graph_snn(ctx.h, 2, ptr(rec), 1, None) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_graph_snn(ctx.h, 0, ptr(rec), 1, ptr(out)) == _lib.RTC_OK and out["shared"][0] == 0xee  # n == 0: nothing is written
    assert ctx.lib.rtc_graph_snn(ctx.h, 2, ptr(rec), 1, ptr(out)) == _lib.RTC_OK
    assert (int(out["shared"][0]), int(out["deg_u"][0]), int(out["deg_v"][0]), int(out["flags"][0])) == (0, 1, 1, 0)


# ---- the command line ----
K, D, KNN = 17, "0.08", "10"


@pytest.fixture(scope="module")
def families(oracle, tmp_path_factory):
    """36 genomes in three families, their KSSD graph restated: (directory, list file, meta, n, records (u, v), weights)"""
    import refgraph
    from tests.test_gpu_dbscan import _write_fastas
    tmp = str(tmp_path_factory.mktemp("snn"))
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 12, 1_000_000, seed=9)
    ks = [oracle.kssd_sketch(s, K, 3) for s in seqs]
    weighted = refgraph.weighted(refgraph.edges(ks, float(D), K, int(KNN)), ks, K)
    return tmp, lst, meta, len(ks), [(u, v) for u, v, _ in weighted], [w for _, _, w in weighted]


def _cli(families, name, args):
    """one run in a directory of its own: (stderr, the result file's text, the directory, the metrics)"""
    from tests.test_gpu_dbscan import BIN, _run
    cwd = os.path.join(families[0], name)
    os.makedirs(cwd)
    out, mj = os.path.join(cwd, "result.out"), os.path.join(cwd, "metrics.json")
    os.environ["RTC_METRICS_JSON"] = mj
    try:
        err = _run([os.path.join(BIN, "clust-leiden")] + args + ["-t", "4", "-o", out], cwd)
    finally:
        del os.environ["RTC_METRICS_JSON"]
    return err, open(out).read(), cwd, json.load(open(mj))


def _quantised(reweighted):
    import reflouvain
    return [(u, v, max(1, round(w * 2 ** 20))) for u, v, w in reweighted], [(u, v, reflouvain.quantise(w)) for u, v, w in reweighted]


def test_cli_fast_louvain_snn(families):
    import reflouvain
    from tests.test_gpu_dbscan import _folders
    from tests.test_gpu_leiden import _print_result
    tmp, lst, meta, n, rec, w0 = families
    src = ["--fast", "-l", "-i", lst, "-k", str(K), "-d", D, "--knn", KNN]
    err, text, cwd, m = _cli(families, "louvain_snn", src + ["--louvain", "--resolution", "2.0", "--snn", "--save-graph"])
    rw, pruned = R.reweighted(n, rec, w0)
    by_round, records = _quantised(rw)
    assert by_round == records and pruned == 0  # max(1, round(w 2^20)) and the callers' llround agree on these weights
    labels, ncl, levels, _, _ = reflouvain.louvain(n, records, 2.0)
    assert text == _print_result(reflouvain.clusters_of(labels), meta)
    ws = [w for _, _, w in rw]
    assert "-----SNN: %d edge(s), %d triangle(s), 0 pruned, weights [%g, %g]\n" % (len(rec), R.triangles(n, rec), min(ws), max(ws)) in err
    assert m["leiden_edges"] == len(rec) and m["leiden_snn_triangles"] == R.triangles(n, rec) and m["leiden_snn_pruned"] == 0
    assert m["leiden_snn_s"] > 0 and m["leiden_clusters"] == ncl
    # without the flag: the similarity weights' clusters, which differ here -- the flag acts -- and the same leiden.graph
    err0, text0, cwd0, m0 = _cli(families, "louvain", src + ["--louvain", "--resolution", "2.0", "--save-graph"])
    labels0 = reflouvain.louvain(n, [(u, v, reflouvain.quantise(w)) for (u, v), w in zip(rec, w0)], 2.0)[0]
    assert text0 == _print_result(reflouvain.clusters_of(labels0), meta) and text0 != text
    assert "-----SNN" not in err0 and not any(k.startswith("leiden_snn") for k in m0) and m0["leiden_edges"] == len(rec)
    (f1,), (f0,) = _folders(cwd), _folders(cwd0)
    graph = open(os.path.join(f1, "leiden.graph"), "rb").read()
    assert graph == open(os.path.join(f0, "leiden.graph"), "rb").read() and len(graph.splitlines()) == len(rec) + 1
    # --pregraph --snn: the direct run's result, byte for byte; --pregraph alone: the run without the flag
    assert _cli(families, "pre_snn", ["--louvain", "--resolution", "2.0", "--pregraph", f1, "--snn"])[1] == text
    # --snn-prune 0.5: exactly the records the restatement drops
    rw5, pruned5 = R.reweighted(n, rec, w0, 0.5)
    assert 0 < pruned5 < len(rec)
    labels5 = reflouvain.louvain(n, _quantised(rw5)[1], 2.0)[0]
    err5, text5, _, m5 = _cli(families, "prune", ["--louvain", "--resolution", "2.0", "--pregraph", f1, "--snn", "--snn-prune", "0.5"])
    assert m5["leiden_snn_pruned"] == pruned5 and m5["leiden_edges"] == len(rec) - pruned5 and m5["leiden_snn_triangles"] == R.triangles(n, rec)
    assert text5 == _print_result(reflouvain.clusters_of(labels5), meta)
    assert "-----SNN: %d edge(s), %d triangle(s), %d pruned, weights [0.5, 1]\n" % (len(rec), R.triangles(n, rec), pruned5) in err5


def test_cli_fast_mcl_snn(families):
    from tests import refmcl
    from tests.test_gpu_leiden import _print_result
    tmp, lst, meta, n, rec, w0 = families
    err, text, _, m = _cli(families, "mcl_snn", ["--fast", "-l", "-i", lst, "-k", str(K), "-d", D, "--knn", KNN, "--mcl", "--snn"])
    by_round, records = _quantised(R.reweighted(n, rec, w0)[0])
    assert by_round == records
    labels, iterations, converged, M = refmcl.mcl(n, records, 4, 1024, 100)
    assert converged == 1 and 1 < len(set(labels)) < n
    assert text == _print_result(refmcl.clusters_of(labels), meta)
    assert "-----MCL: %d iteration(s), converged, " % iterations in err and "-----SNN: %d edge(s), " % len(rec) in err
    assert m["mcl_iterations"] == iterations and m["leiden_snn_pruned"] == 0


def test_cli_minhash_leiden_snn_equals_its_pregraph_rerun(families):
    from tests.test_gpu_dbscan import _folders
    tmp, lst, meta, n, rec, w0 = families
    alg = ["--minhash", "--leiden", "--objective", "modularity", "--snn"]
    err, text, cwd, m = _cli(families, "minhash_snn", alg + ["-l", "-i", lst, "-k", "19", "-s", "128", "-d", "0.1", "--knn", KNN, "--save-graph"])
    assert "-----Building similarity graph (MinHash)..." in err and "-----SNN: %d edge(s), " % m["leiden_edges"] in err
    assert m["leiden_edges"] > 0 and 1 < m["leiden_clusters"] < n
    (folder,) = _folders(cwd)
    err2, text2, _, m2 = _cli(families, "minhash_pre_snn", alg + ["--pregraph", folder])
    assert text2 == text and len(text) > 0
    assert (m2["leiden_edges"], m2["leiden_snn_triangles"], m2["leiden_clusters"]) == (m["leiden_edges"], m["leiden_snn_triangles"], m["leiden_clusters"])
