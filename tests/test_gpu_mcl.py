"""rtc_mcl on the GPU against tests/refmcl.py, entry for entry: every set of tests/mcl_sets.py at inflation 1.5, 2 and 2.5 after
1, 2 and 3 iterations and at the fixed point, the three column paths and the switch that forces the long one, the errors, and
clust-leiden --mcl through the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import mcl_sets as S
from tests import refmcl as R

pytestmark = pytest.mark.gpu

SETS = sorted(S.every_set())


def _records(rec):
    from rabbittclust_amd import api
    return np.array(rec, dtype=api.WEDGE_DT) if rec else np.zeros(0, dtype=api.WEDGE_DT)


def _got(ctx, n, rec, h, sel, T):
    labels, mat = ctx.mcl(n, _records(rec), h / 2.0, sel, T, return_matrix=True)
    assert not mat["pad"].any()
    return labels.tolist(), ctx.mcl_iterations, ctx.mcl_converged, list(zip(mat["col"].tolist(), mat["row"].tolist(), mat["value"].tolist()))


def _check(ctx, name, h, T, rec=None, sets=None):
    n, records, sel = (sets or S.every_set())[name]
    want = S.expected(name, h, T, sets)
    got = _got(ctx, n, records if rec is None else rec, h, sel, T)
    assert got[3] == want[3], (name, h, T)
    assert got[:3] == want[:3], (name, h, T)
    c = ctx.mcl_counters()
    assert (c["iterations"], c["converged"], c["entries"]) == (want[1], want[2], len(want[3]))
    assert c["attractors"] == sum(1 for col, row, _ in want[3] if col == row)
    assert ctx.mcl_clusters == len(set(want[0]))
    return c


@pytest.mark.parametrize("h", [3, 4, 5])
@pytest.mark.parametrize("name", SETS)
def test_mcl_equals_the_restatement(ctx, name, h):
    for T in (1, 2, 3, 100):
        c = _check(ctx, name, h, T)
    n = S.every_set()[name][0]
    paths = c["wave_columns"] + c["workgroup_columns"] + c["global_columns"]
    assert paths == (n * c["iterations"] if S.every_set()[name][1] else 0)
    assert c["total_ns"] > 0


def test_start_matrix(ctx):
    """T == 0: the start matrix, not converged, clusters by the fallback rule"""
    for name in ("hub_star_s8", "duplicates", "tied_clique_s8", "families_12x15_s8", "empty"):
        c = _check(ctx, name, 4, 0)
        assert c["iterations"] == 0 and c["converged"] == 0


def test_boundary_sets_take_all_three_paths(ctx):
    from rabbittclust_amd import api
    wave, block = S.boundaries()
    seen = 0
    for B in (wave, block):
        name = "boundary_%d" % B
        (n, rec, sel), probes = S.boundary(B)
        W = S.work(S.trajectory(name, 4)[0][0])
        c = _check(ctx, name, 4, 1)
        assert c["wave_columns"] == sum(w <= wave for w in W)
        assert c["workgroup_columns"] == sum(wave < w <= block for w in W)
        assert c["global_columns"] == sum(w > block for w in W)
        want = (api.MCL_PATH_WAVE if c["wave_columns"] else 0) | (api.MCL_PATH_WORKGROUP if c["workgroup_columns"] else 0) | \
               (api.MCL_PATH_GLOBAL if c["global_columns"] else 0)
        assert ctx.mcl_last_path() == want
        seen |= want
    assert seen == api.MCL_PATH_WAVE | api.MCL_PATH_WORKGROUP | api.MCL_PATH_GLOBAL


def test_select_cuts_are_counted(ctx):
    for name in ("tied_clique_s8", "hub_star_s8", "families_12x15_s8"):
        n, rec, sel = S.every_set()[name]
        mats = S.trajectory(name, 4)[0]
        cut_start = sum(len(a) + 1 > sel for a in R.adjacency(n, rec))
        assert cut_start > 0
        c = _check(ctx, name, 4, 0)
        assert c["cut_columns"] == cut_start
        c = _check(ctx, name, 4, 1)
        assert c["cut_columns"] >= cut_start
    # the families at S = 8: an iteration's expansion reaches more than 8 rows, so select cuts there too
    assert c["cut_columns"] > cut_start
    c = _check(ctx, "families_12x15", 4, 100)
    assert c["cut_columns"] == 0


@pytest.fixture
def global_path(ctx):
    os.environ["RTC_MCL_GLOBAL"] = "1"
    ctx.reload_options()
    yield
    del os.environ["RTC_MCL_GLOBAL"]
    ctx.reload_options()


@pytest.mark.parametrize("name", ["path9_equal", "tied_clique_s8", "hub_star_s8", "duplicates", "families_12x15_s8", "families_6x40_s16",
                                  "boundary_%d" % S.boundaries()[0]])
def test_global_switch_gives_identical_matrices(ctx, global_path, name):
    from rabbittclust_amd import api
    for h in (3, 4):
        for T in (1, 100):
            c = _check(ctx, name, h, T)
            assert c["wave_columns"] == 0 and c["workgroup_columns"] == 0 and c["global_columns"] > 0
            assert ctx.mcl_last_path() == api.MCL_PATH_GLOBAL


@pytest.mark.parametrize("name", ["duplicates", "families_12x15_s8", "families_6x40_s16"])
def test_record_order_does_not_matter(ctx, name):
    rec = S.shuffled(S.every_set()[name][1])
    for T in (1, 100):
        _check(ctx, name, 5, T, rec=rec)


def test_early_stop_takes_the_fallback_rule(ctx):
    """max_iter below the convergence count: converged = 0; on the chain at S = 1 the upper columns then name a row that is no
    attractor and take it"""
    for T in (0, 1, 2):
        M = S.trajectory("chain_s1", 4)[0][T]
        assert any(not M[j].get(j) and not any(M[i].get(i) for i in M[j]) for j in range(len(M)))  # the rule is needed
        c = _check(ctx, "chain_s1", 4, T)
        assert c["converged"] == 0 and c["iterations"] == T
    for name in ("path9_equal", "ring40", "families_12x15"):
        c = _check(ctx, name, 4, 2)
        assert c["converged"] == 0 and c["iterations"] == 2


def test_errors(ctx):
    from rabbittclust_amd import _lib, api
    one = _records([(0, 1, S.UNIT)])
    for bad in (1.0, 8.5):
        with pytest.raises(_lib.RtcError) as e:
            ctx.mcl(2, one, bad)
        assert e.value.status == _lib.RTC_ERR_ARG
    with pytest.raises(ValueError):
        ctx.mcl(2, one, 2.25)
    for bad in (0, 4097):
        with pytest.raises(_lib.RtcError) as e:
            ctx.mcl(2, one, 2.0, bad)
        assert e.value.status == _lib.RTC_ERR_ARG
    for rec in ([(0, 1, 0)], [(0, 2, 5)], [(2, 0, 5)]):
        with pytest.raises(_lib.RtcError) as e:
            ctx.mcl(2, _records(rec))
        assert e.value.status == _lib.RTC_ERR_ARG
    n, rec, sel = S.summed(1 << 32)
    with pytest.raises(_lib.RtcError) as e:
        ctx.mcl(n, _records(rec))
    assert e.value.status == _lib.RTC_ERR_UNSUPPORTED
    # room for fewer entries than the matrix has: the count comes back
    n, rec, sel = S.two_cliques()
    want = S.expected("two_cliques", 4, 100)
    e = _records(rec)
    labels = np.zeros(n, dtype=np.int32)
    ncl, its, conv, nnz = C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_uint64(0)
    mat = np.zeros(len(want[3]), dtype=api.MCL_ENTRY_DT)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda cap: ctx.lib.rtc_mcl(ctx.h, n, ptr(e), len(e), 4, sel, 100, ptr(labels), C.byref(ncl), C.byref(its), C.byref(conv), ptr(mat), cap,
                                       C.byref(nnz))
    assert call(len(want[3]) - 1) == _lib.RTC_ERR_OVERFLOW and nnz.value == len(want[3])
    assert b"entries" in ctx.lib.rtc_last_error(ctx.h)
    assert call(len(want[3])) == _lib.RTC_OK and nnz.value == len(want[3])
    assert list(zip(mat["col"].tolist(), mat["row"].tolist(), mat["value"].tolist())) == want[3] and labels.tolist() == want[0]


# ---- the command line ----
def _expect(n, records, h, sel, T=100):
    labels, iterations, converged, M = R.mcl(n, records, h, sel, T)
    return labels, iterations, converged, sum(len(c) for c in M), sum(1 for a in range(n) if M[a].get(a, 0) > 0)


def test_cli_fast_mcl_save_graph_and_pregraph(oracle, tmp_path):
    import refgraph
    import reflouvain
    from tests.test_gpu_dbscan import BIN, _folders, _run, _write_fastas
    from tests.test_gpu_leiden import _print_result
    tmp = str(tmp_path)
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 12, 1_000_000, seed=9)  # 36 genomes in three families
    exe = os.path.join(BIN, "clust-leiden")
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]
    out, metrics = os.path.join(tmp, "a.out"), os.path.join(tmp, "metrics.json")
    os.environ["RTC_METRICS_JSON"] = metrics
    try:
        err = _run([exe, "--fast", "--mcl", "-l", "-i", lst, "-k", "17", "-d", "0.08", "--knn", "10", "--save-graph", "-t", "4", "-o", out], tmp)
    finally:
        del os.environ["RTC_METRICS_JSON"]
    edges = refgraph.edges(ks, 0.08, 17, 10)
    weighted = refgraph.weighted(edges, ks, 17)
    records = [(u, v, reflouvain.quantise(w)) for u, v, w in weighted]
    labels, iterations, converged, entries, attractors = _expect(len(ks), records, 4, 1024)
    assert converged == 1 and 1 < len(set(labels)) < len(ks)
    assert "-----Algorithm: MCL (inflation 2, select 1024)\n" in err and "(k=10)" in err
    assert "-----MCL: %d iteration(s), converged, %d attractor(s)\n" % (iterations, attractors) in err and "Warning" not in err
    assert open(out).read() == _print_result(R.clusters_of(labels), meta)
    m = json.load(open(metrics))
    assert m["command"] == "clust-leiden" and m["leiden_edges"] == len(edges) and m["leiden_clusters"] == len(set(labels))
    assert m["mcl_iterations"] == iterations and m["mcl_converged"] == 1 and m["mcl_entries"] == entries
    assert m["mcl_expand_s"] > 0 and m["leiden_louvain_s"] >= m["mcl_expand_s"] and m["leiden_graph_s"] > 0
    assert "leiden_levels" not in m and "leiden_modularity" not in m
    # --pregraph: the restatement on the file's weights, at another inflation and a selection that cuts; stopped early it warns
    folder = _folders(tmp)
    assert len(folder) == 1
    lines = open(os.path.join(folder[0], "leiden.graph")).read().splitlines()
    parsed = [(int(a), int(b), reflouvain.quantise(float(w))) for a, b, w in (ln.split() for ln in lines[1:])]
    labels2, its2, conv2, _, att2 = _expect(len(ks), parsed, 5, 4)
    out2 = os.path.join(tmp, "b.out")
    err2 = _run([exe, "--mcl", "--inflation", "2.5", "--mcl-select", "4", "--pregraph", folder[0], "-o", out2], tmp)
    assert "-----Algorithm: MCL (inflation 2.5, select 4)\n" in err2
    assert "-----MCL: %d iteration(s), %s, %d attractor(s)\n" % (its2, "converged" if conv2 else "NOT converged", att2) in err2
    assert open(out2).read() == _print_result(R.clusters_of(labels2), meta)
    labels3, its3, conv3, _, att3 = _expect(len(ks), parsed, 4, 1024, T=2)
    assert conv3 == 0
    out3 = os.path.join(tmp, "c.out")
    err3 = _run([exe, "--mcl", "--mcl-iterations", "2", "--pregraph", folder[0], "-o", out3], tmp)
    assert "-----MCL: 2 iteration(s), NOT converged, %d attractor(s)\n" % att3 in err3 and "-----Warning: MCL did not converge in 2 iteration(s)" in err3
    assert open(out3).read() == _print_result(R.clusters_of(labels3), meta)
    # --louvain on the same input: what it was before --mcl existed
    out4 = os.path.join(tmp, "d.out")
    _run([exe, "--fast", "--louvain", "--presketched", folder[0], "-d", "0.08", "--knn", "10", "-o", out4], tmp)
    e4 = refgraph.edges(ks, 0.08, 18, 10)  # --presketched: k is the folder's half_k * 2 = 18
    l4 = reflouvain.louvain(len(ks), [(u, v, reflouvain.quantise(w)) for u, v, w in refgraph.weighted(e4, ks, 18)], 1.0)[0]
    assert open(out4).read() == _print_result(reflouvain.clusters_of(l4), meta)


def test_cli_minhash_mcl(oracle, tmp_path):
    import reflouvain
    from tests import refgraph_mash as G
    from tests.test_gpu_dbscan import BIN, _run, _write_fastas
    from tests.test_gpu_leiden import _print_result
    tmp = str(tmp_path)
    L, s, k, D, KNN = 500_000, 128, 19, 0.1, 10
    lst, seqs, meta = _write_fastas(oracle, tmp, 3, 13, L, seed=11)
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * L
    counts = G.counts(oracle.sketch_minhash_batch(np.concatenate(seqs), off, k, s), s)
    weighted = G.weighted(G.edges(counts, D, k, KNN), k)
    records = [(u, v, reflouvain.quantise(w)) for u, v, w in weighted]
    labels, iterations, converged, _, attractors = _expect(len(meta), records, 3, 1024)
    assert converged == 1 and 1 < len(set(labels)) < len(meta)
    out = os.path.join(tmp, "m.out")
    err = _run([os.path.join(BIN, "clust-leiden"), "--minhash", "--mcl", "--inflation", "1.5", "-l", "-i", lst, "-k", str(k), "-s", str(s), "-d", str(D),
                "--knn", str(KNN), "-t", "4", "-o", out], tmp)
    assert "-----Building similarity graph (MinHash)..." in err and "-----Algorithm: MCL (inflation 1.5, select 1024)\n" in err
    assert "-----MCL: %d iteration(s), converged, %d attractor(s)\n" % (iterations, attractors) in err
    assert open(out).read() == _print_result(R.clusters_of(labels), meta)
