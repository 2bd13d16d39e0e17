"""clust-leiden --db without a GPU: the placement rule (tests/refleiden_assign.py) on cases small enough to check on paper, the
host's model sums and its per-weight quantisation against Python, the model file byte for byte with every refusal of its
loader, the command line's flag errors, and the proof that the hold-out input of the GPU suite places every held-out genome in
its family's community.  Integers and bytes only: no tolerances."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import leiden_assign_sets as S
from tests import leiden_sets
from tests import refgraph
from tests import refleiden
from tests import refleiden_assign as A
from tests import reflouvain
from tests.refleiden_assign import CPM, MODULARITY

ONE = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEIDEN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-leiden")


def _g(resolution):
    return A._llround(resolution * 65536.0)


# ---- the rule on paper --------------------------------------------------------------------------------------------------
def test_cpm_and_modularity_disagree():
    """A query with 6 units into community 0 (10 members, tot 20 units) and 3 units into community 1 (2 members, tot 40 units).
    CPM at 0.5: S(0) ~ 6 - 0.5 * 10 = 1, S(1) ~ 3 - 0.5 * 2 = 2: community 1, runner-up 0.
    Modularity at 1.0 with M2 = 60, k_x = 9: S(0) ~ 6 * 78 - 9 * 26 = 234, S(1) ~ 3 * 78 - 9 * 43 = -153: community 0 alone."""
    labels = [0] * 10 + [1] * 2
    records = [(p, ONE) for p in range(6)] + [(10, 2 * ONE), (11, ONE)]
    assert A.place(records, labels, CPM, _g(0.5), [10, 2]) == (1, 0, 8, 2, 9 * ONE, 3 * ONE, 6 * ONE)
    assert A.place(records, labels, MODULARITY, _g(1.0), [20 * ONE, 40 * ONE], 60 * ONE) == (0, -1, 8, 2, 9 * ONE, 6 * ONE, 0)
    # the scores themselves, in the units of the definition
    assert 6 * ONE * 65536 - _g(0.5) * ONE * 10 == ONE * 65536 and 3 * ONE * 65536 - _g(0.5) * ONE * 2 == 2 * ONE * 65536
    assert (6 * 78 - 9 * 26, 3 * 78 - 9 * 43) == (234, -153)


def test_equal_scores_go_to_the_smaller_community():
    labels = [5, 2, 7]
    assert A.place([(0, 2 * ONE), (1, 2 * ONE), (2, ONE)], labels, CPM, _g(0.5), [0, 0, 1, 0, 0, 1, 0, 1]) == (2, 5, 3, 3, 5 * ONE, 2 * ONE, 2 * ONE)
    assert A.place_all(2, [(1, 0, 2 * ONE), (1, 1, ONE), (1, 1, ONE)], labels, CPM, 0.5, [0, 0, 1, 0, 0, 1, 0, 1])[1][:2] == (2, 5)  # duplicates are summed


def test_a_score_of_exactly_zero_is_novel():
    # one unit into a community of two at resolution 0.5: 1 - 0.5 * 2 = 0, not above it
    assert A.place([(0, ONE)], [0, 0], CPM, _g(0.5), [2]) == (-1, -1, 1, 1, ONE, 0, 0)
    assert A.place([(0, ONE + 1)], [0, 0], CPM, _g(0.5), [2]) == (0, -1, 1, 1, ONE + 1, ONE + 1, 0)
    assert A.place([], [0, 0], CPM, _g(0.5), [2]) == (-1, -1, 0, 0, 0, 0, 0)
    # CPM at resolution 1 with weights of at most one unit: nothing is positive
    assert A.place([(0, ONE), (1, ONE)], [0, 1], CPM, _g(1.0), [1, 1]) == (-1, -1, 2, 2, 2 * ONE, 0, 0)
    with pytest.raises(ValueError):
        A.place([(0, 1 << 44)], [0], MODULARITY, _g(1.0), [1 << 45], 1 << 45)


def test_a_cpm_record_quantised_to_zero_drops_out():
    """a model whose run scaled its weights from [0.9, 1.0]: a query's weight at or below 0.9 gives q < 1 and drops out, so the
    query next to one such genome alone is novel without an edge; under modularity the same weight is a record"""
    assert A.quantise(0.9, CPM, True, 0.9, 0.1) == 0 and A.quantise(0.85, CPM, True, 0.9, 0.1) == 0
    assert A.quantise(0.9 + 0.1 * 0.4 / ONE, CPM, True, 0.9, 0.1) == 0 and A.quantise(0.95, CPM, True, 0.9, 0.1) in (ONE // 2, ONE // 2 + 1, ONE // 2 - 1)
    assert A.quantise(1.05, CPM, True, 0.9, 0.1) > ONE  # outside [0, 1]: the same lines
    assert A.quantise(1e-9, CPM) == 0 and A.quantise(1e-9, MODULARITY) == 1 and A.quantise(5000.0, MODULARITY) == 0xFFFFFFFF
    model = [np.arange(100), np.arange(1000, 1100)]
    query = [np.concatenate([np.arange(60), np.arange(5000, 5040)])]  # 60 of 140: weight 1 + ln(0.6)/21 = 0.9757

    def fixed(common, a, b, k):
        return refgraph.weight(common, a, b, k)
    w = fixed(60, 100, 100, 21)
    got, near, records = A.assign(model, [0, 1], query, 0.2, 21, 0, CPM, 0.01, [1, 1], 0, True, w, 0.01, fixed)
    assert records == [] and got == [(-1, -1, 0, 0, 0, 0, 0)] and near == [(0, 60, 140, 1, 1, 1)]
    got, _, records = A.assign(model, [0, 1], query, 0.2, 21, 0, MODULARITY, 1.0, [ONE, ONE], 2 * ONE, False, 0.0, 1.0, fixed)
    assert len(records) == 1 and got[0][0] == 0


def test_knn_cuts_the_edge_that_would_have_changed_the_label():
    """the query shares 80 of its 100 hashes with A1, A2 (community 0; weight 1 + ln(0.8)/21 = 0.9894 each) and 50 with B1, B2,
    B3 (community 1; 1 + ln(0.5)/21 = 0.9670 each).  CPM at 0.3: S(0) ~ 1.979 - 0.6 = 1.379, S(1) ~ 2.901 - 0.9 = 2.001 with every
    edge; with knn_k = 4 the third B is cut (equal ranks go to the lower index) and S(1) ~ 1.934 - 0.9 = 1.034"""
    from rabbittclust_amd import api
    q = np.arange(100)
    model = [np.concatenate([np.arange(80), np.arange(1000 + 20 * i, 1020 + 20 * i)]) for i in range(2)]
    model += [np.concatenate([np.arange(50), np.arange(2000 + 50 * i, 2050 + 50 * i)]) for i in range(3)]
    labels = [0, 0, 1, 1, 1]
    args = (CPM, 0.3, [2, 3], 0, False, 0.0, 1.0, api.graph_weight)
    full, near, rec = A.assign(model, labels, [q], 0.2, 21, 0, *args)
    assert full[0][:4] == (1, 0, 5, 2) and near[0] == (0, 80, 120, 5, 5, 5)
    cut, near, rec = A.assign(model, labels, [q], 0.2, 21, 4, *args)
    assert cut[0][:4] == (0, 1, 4, 2) and near[0] == (0, 80, 120, 5, 5, 4) and [p for _, p, _ in rec] == [0, 1, 2, 3]
    assert A.assign(model, labels, [q], 0.2, 21, 2, *args)[0][0][:4] == (0, -1, 2, 1)


# ---- the host's pieces --------------------------------------------------------------------------------------------------
def test_model_sums_equal_python():
    from rabbittclust_amd import host
    graphs = dict(leiden_sets.hand_graphs())
    graphs["loops"] = (4, [(0, 1, 5), (1, 0, 5), (2, 3, 4), (1, 2, 1), (3, 3, 2)])
    for name, (n, edges) in graphs.items():
        labels, ncl, _ = refleiden.leiden(n, edges, 0.25, CPM)
        k, tot, m2, size = A.model_sums(n, edges, labels, ncl)
        gk, gtot, gm2, gsize = host.leiden_model_sums(edges, labels, ncl)
        assert (gk.tolist(), gtot.tolist(), gm2, gsize.tolist()) == (k, tot, m2, size), name
        assert m2 == 2 * sum(q for _, _, q in edges) and sum(size) == n
    assert A.model_sums(4, graphs["loops"][1], [0, 0, 1, 1], 2) == ([10, 11, 5, 8], [21, 13], 34, [2, 2])
    with pytest.raises(ValueError):
        host.leiden_model_sums([(0, 9, 1)], [0, 0], 1)
    with pytest.raises(ValueError):
        host.leiden_model_sums([(0, 1, 1)], [0, 3], 2)


def test_per_weight_quantisation_equals_the_run_s():
    """leiden_quantise_weight with the (scale, lo, range) of leiden_quantiser reproduces rtch_leiden_quantise record for record,
    on the inputs of tests/test_cpu_leiden_refine.py::test_host_quantise_equals_python, and equals the restatement"""
    from rabbittclust_amd import host
    rng = np.random.default_rng(3)
    narrow = [(int(a), int(b), float(w)) for a, b, w in zip(rng.integers(0, 50, 200), rng.integers(0, 50, 200), 0.9 + 0.1 * rng.random(200))]
    cases = {"narrow": narrow, "wide": [(0, 1, 0.2), (1, 2, 0.95), (2, 3, 0.5), (3, 4, 1e-9)], "flat": [(0, 1, 0.75), (1, 2, 0.75), (2, 3, 0.75 + 5e-7)],
             "half": [(0, 1, 0.5), (1, 2, 1.0)], "empty": []}
    for name, records in cases.items():
        u, v, w = ([r[i] for r in records] for i in range(3))
        for objective in (CPM, MODULARITY):
            run, narrow_flag = host.leiden_quantise(u, v, w, objective)
            scale, lo, span, flag = host.leiden_quantiser(w, objective)
            assert flag == narrow_flag and scale == (name == "narrow" and objective == CPM), (name, objective)
            mine = [(a, b, host.leiden_quantise_weight(x, objective, scale, lo, span)) for a, b, x in records]
            assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in run] == [r for r in mine if r[2]], (name, objective)
            assert [r[2] for r in mine] == [A.quantise(x, objective, scale, lo, span) for x in w], (name, objective)
    # a query's weight outside the run's range, both sides
    assert host.leiden_quantise_weight(0.85, CPM, True, 0.9, 0.1) == 0 and host.leiden_quantise_weight(1.05, CPM, True, 0.9, 0.1) == A.quantise(1.05, CPM, True, 0.9, 0.1)


def test_assign_weights_on_threads_equal_the_restatement():
    from rabbittclust_amd import api, host
    model, queries = S.query_case()
    edges, _ = A.graph_query(model, queries, S.THRESHOLD, S.K, 3)
    e = np.array([(q, p, c, 0) for q, p, c in edges], dtype=api.QEDGE_DT)
    ms, qs = [len(s) for s in model], [len(s) for s in queries]
    w = A.weights(edges, model, queries, S.K, api.graph_weight)
    for objective, scale, lo, span in ((CPM, True, min(w) + 0.001, 0.02), (CPM, False, 0.0, 1.0), (MODULARITY, False, 0.0, 1.0)):
        want = [(q, p, A.quantise(x, objective, scale, lo, span)) for (q, p, _), x in zip(edges, w)]
        want = [r for r in want if r[2]]
        for threads in (1, 3):
            got = host.leiden_assign_weights(e, ms, qs, S.K, objective, scale, lo, span, threads)
            assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in got] == want, (objective, threads)
        assert (len(want) < len(edges)) == scale


# ---- the model file -----------------------------------------------------------------------------------------------------
def _model_file(path, width=4, objective=CPM):
    from rabbittclust_amd import host
    sk = [np.arange(5, 15), np.arange(0), np.arange(100, 103)]
    head = [1, objective, width, 1, 21, 10, 6, 3, 500, 2, 1]
    assert host.leiden_model_save(path, head, 10000, 0.05, 0.3, 0.91, 0.07, 12345 if objective else 0, [0, 1, 0], [2, 1], ["a.fna", "b.fna", "c.fna"],
                                  [1000, 2000, 3000], sk) == 0
    return sk


@pytest.mark.parametrize("width", [4, 8])
def test_model_file_round_trip_and_refusals(tmp_path, width):
    from rabbittclust_amd import host
    path, again = str(tmp_path / "m.ldb"), str(tmp_path / "again.ldb")
    sk = _model_file(path, width)
    blob = open(path, "rb").read()
    assert not os.path.exists(path + ".tmp")
    m = A.parse_model(blob)
    assert [m[k] for k in ("version", "algorithm", "objective", "width", "by_file", "kmer_size", "half_k", "half_subk", "drlevel", "knn", "n_clusters",
                           "scale")] == [1, 1, 0, width, 1, 21, 10, 6, 3, 500, 2, 1]
    assert (m["min_len"], m["n"], m["threshold"], m["resolution"], m["lo"], m["range"], m["m2"]) == (10000, 3, 0.05, 0.3, 0.91, 0.07, 0)
    assert m["labels"].tolist() == [0, 1, 0] and m["tot"].tolist() == [2, 1] and [g["file"] for g in m["genomes"]] == ["a.fna", "b.fna", "c.fna"]
    assert [g["total_length"] for g in m["genomes"]] == [1000, 2000, 3000] and all(np.array_equal(a, b) for a, b in zip(m["sketches"], sk))
    assert host.leiden_model_resave(path, again) == (0, "") and open(again, "rb").read() == blob and not os.path.exists(again + ".tmp")

    def refused(data, text):
        bad = str(tmp_path / "bad.ldb")
        open(bad, "wb").write(data)
        rc, why = host.leiden_model_resave(bad, again)
        assert rc == -1 and text in why, (why, text)
        r = subprocess.run([LEIDEN, "--db", bad, "--stats"], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and "ERROR: --db " + bad + ": " + why in r.stderr and "no MI355X context" not in r.stderr
    refused(b"RTCDBSM1" + blob[8:], "bad magic")
    refused(blob[:5], "bad magic")
    refused(blob[:8] + struct.pack("<i", 2) + blob[12:], "has version 2")
    sec = m["sections"]
    for cut in (20, sec["header"] - 1, sec["header"] + 5, sec["labels"] + 3, sec["tot"] + 9, sec["genomes"] + 2, sec["lengths"] + 1, len(blob) - 1):
        refused(blob[:cut], "is truncated")
    refused(blob + b"\0", "has 1 bytes after its end")
    refused(blob[:sec["header"]] + struct.pack("<i", 7) + blob[sec["header"] + 4:], "label 7")
    assert host.leiden_model_resave(str(tmp_path / "none.ldb"), again) == (-1, "cannot open")


def test_cli_stats_needs_no_gpu(tmp_path):
    path = str(tmp_path / "m.ldb")
    _model_file(path, 8, MODULARITY)
    r = subprocess.run([LEIDEN, "--db", path, "--stats"], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stderr
    for line in ("Algorithm:   Leiden", "Objective:   modularity", "Hash width:  8", "Kmer size:   21", "Half k:      10", "Drlevel:     3",
                 "Min length:  10000", "Threshold:   0.05", "Resolution:  0.3", "Knn:         500", "Total weight: 12345", "Genomes:     3",
                 "Clusters:    2", "Largest:     2", "Singletons:  1"):
        assert line in r.stdout, (line, r.stdout)
    assert "no MI355X context" not in r.stderr
    _model_file(path, 4, CPM)
    r = subprocess.run([LEIDEN, "--db", path, "--stats"], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "Objective:   cpm" in r.stdout and "Weights:     scaled from [0.91, 0.98]" in r.stdout


@pytest.mark.parametrize("args,msg", [
    (["--fast", "--leiden", "--db", "m.ldb", "--build", "--assign", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --build, --assign and --stats exclude each other"),
    (["--db", "m.ldb", "--assign", "--stats", "-i", "q.fna", "-o", "o.txt"], "ERROR: --build, --assign and --stats exclude each other"),
    (["--fast", "--leiden", "--build", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --build / --assign / --stats require --db"),
    (["--assign", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --build / --assign / --stats require --db"),
    (["--stats"], "ERROR: --build / --assign / --stats require --db"),
    (["--fast", "--leiden", "--db", "m.ldb", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --db requires one of --build, --assign, --stats"),
    (["--db", "m.ldb", "--assign", "-o", "o.txt"], "ERROR: --assign requires -i <input_file>"),
    (["--db", "m.ldb", "--assign", "--pregraph", "dir", "-i", "q.fna", "-o", "o.txt"], "ERROR: --assign does not go with --pregraph"),
    (["--db", "m.ldb", "--assign", "--save-graph", "-i", "q.fna", "-o", "o.txt"], "ERROR: --assign does not go with --save-graph"),
    (["--leiden", "--db", "m.ldb", "--build", "--pregraph", "dir", "-o", "o.txt"], "ERROR: --db --build does not go with --pregraph"),
    (["--db", "none.ldb", "--assign", "-i", "q.fna", "-o", "o.txt"], "ERROR: --db none.ldb: cannot open"),
])
def test_cli_refusals_need_no_gpu(tmp_path, args, msg):
    r = subprocess.run([LEIDEN] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert "no MI355X context" not in r.stderr and r.stderr.count("ERROR:") == 1
    assert not os.path.exists(str(tmp_path / "o.txt"))


def test_cli_help_names_the_actions(tmp_path):
    r = subprocess.run([LEIDEN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(x in r.stdout for x in ("--db FILE --build", "--db FILE --assign", "--db FILE --stats"))


# ---- the inputs of the GPU suite ----------------------------------------------------------------------------------------
def test_query_case_holds_its_cases():
    model, queries = S.query_case()
    cut = {}
    for knn in (0, 1, 3, 50):
        edges, near = A.graph_query(model, queries, S.THRESHOLD, S.K, knn)
        cut[knn] = sum(1 for x in near if x[4] > x[5])
        if knn == 1:
            assert [e for e in edges if e[0] == S.COPY] == [(S.COPY, 3, 200)]  # model genomes 3 and 300 tie: the lower one
    assert cut[0] == 0 and cut[50] == 0 and 0 < cut[3] < 40 and cut[1] >= cut[3]
    assert near[S.COPY][:3] == (3, 200, 200) and near[S.COPY][4] >= 2
    assert near[S.EMPTY] == (A.NONE, 0, 0, 0, 0, 0) and all(near[q][0] == A.NONE for q in S.UNRELATED)
    assert near[S.RATIO][3] == 10 and near[S.RATIO][4] == 0  # ten candidates, none passes: the size ratio alone
    n, c, d = near[S.RATIO][:3]
    assert float(c) / d >= A.jstar(S.THRESHOLD, S.K) and 2 * len(model[n]) < len(queries[S.RATIO])
    assert {(3 if p == 300 else p) // 10 for q, p, _ in edges if q == S.STRADDLE} == {0, 3}  # genome 300 is the copy of genome 3
    assert any(x[3] > x[4] > 0 for x in near)  # a query some of whose candidates fail the threshold


def test_holdout_case_places_every_genome_in_its_family():
    from rabbittclust_amd import api
    model, queries, fam = S.holdout_case()
    n = len(model)
    weighted = refgraph.weighted(refgraph.edges(model, S.THRESHOLD, S.K, 50), model, S.K)
    runs = [("leiden", CPM, 0.3), ("leiden", MODULARITY, 1.0), ("louvain", MODULARITY, 1.0)]
    for algorithm, objective, resolution in runs:
        records, _ = refleiden.normalise_and_quantise(weighted, objective)
        if algorithm == "leiden":
            labels, ncl, _ = refleiden.leiden(n, records, resolution, objective)
        else:
            labels, ncl = reflouvain.louvain(n, records, resolution)[:2]
        assert ncl == 10 and all(labels[p] == fam[p] for p in range(n)), (algorithm, objective)
        w = [x for _, _, x in weighted]
        lo, hi = min([1.0] + w), max([0.0] + w)
        scale = objective == CPM and hi - lo < 0.5 and hi - lo > 1e-6
        _, tot, m2, size = A.model_sums(n, records, labels, ncl)
        got, near, _ = A.assign(model, labels, queries, S.THRESHOLD, S.K, 50, objective, resolution, size if objective == CPM else tot,
                                m2 if objective else 0, scale, lo, hi - lo, api.graph_weight)
        assert [g[0] for g in got] == list(range(10)) + [-1], (algorithm, objective, got)
        assert near[10][0] == A.NONE and all(near[f][0] // 6 == f for f in range(10))
