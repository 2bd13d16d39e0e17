"""clust-leiden --db --assign on the GPU: rtc_graph_query and rtc_leiden_place field for field against the brute-force restatement
(tests/refleiden_assign.py) -- both hash widths, segments past TK_LONG, knn_k past 256, the three row paths of the placement
kernel, query chunks and the edge budget, the chain from rtc_graph_build to the placement, the error returns -- and the command
line end to end.  Integers and bytes only; the printed %.6f values are the host's own function on both sides."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import leiden_assign_sets as S
from tests import refgraph
from tests import refleiden
from tests import refleiden_assign as A
from tests import reflouvain
from tests.refleiden_assign import CPM, MODULARITY
from tests.test_gpu_dbscan import BIN, _write_fastas

pytestmark = pytest.mark.gpu

LV_WAVE_ROW, LV_WAVE_SLOTS, LV_BLOCK_ROW = 128, 256, 2048  # rtc_community.h


def _set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=S.K, kind="kssd", width=width)


def _edges(e):
    return [(int(r["q"]), int(r["p"]), int(r["common"])) for r in e]


def _near(n):
    return [tuple(int(x) for x in r) for r in n.tolist()]


_REF = {}


def _query_ref(knn):
    """the restatement on the 40-query case, once per knn_k"""
    if knn not in _REF:
        model, queries = S.query_case()
        _REF[knn] = A.graph_query(model, queries, S.THRESHOLD, S.K, knn)
    return _REF[knn]


def _counters_match(c, near, n_edges):
    assert c["candidates"] == sum(x[3] for x in near) and c["passing"] == sum(x[4] for x in near) and c["kept"] == sum(x[5] for x in near) == n_edges
    assert c["queries_cut"] == sum(1 for x in near if x[4] > x[5]) and c["queries_alone"] == sum(1 for x in near if x[3] == 0)


# ---- 1. rtc_graph_query against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_graph_query_equals_the_restatement(ctx, width):
    model, queries = S.query_case()
    sk = _set(ctx, model + queries, width)
    for knn in (0, 1, 3, 50):
        want_e, want_n = _query_ref(knn)
        got_e, got_n = ctx.graph_query(sk, len(model), S.THRESHOLD, S.K, knn)
        assert _edges(got_e) == want_e, (width, knn)
        assert _near(got_n) == want_n, (width, knn)
        assert got_e["pad"].tolist() == [0] * len(want_e)
        c = ctx.graph_query_counters()
        assert c["chunks"] == 1
        _counters_match(c, want_n, len(want_e))


# ---- 2. a segment longer than TK_LONG, knn_k above 256 -------------------------------------------------------------------
def test_long_segment_and_large_knn(ctx):
    model, queries = S.long_case()
    sk = _set(ctx, model + queries, 4)
    for knn in (0, 300, 1000):
        want_e, want_n = A.graph_query(model, queries, 0.2, S.K, knn)
        for q in (0, 3):  # 4 200 candidates each, past TK_LONG = 4 096, and they all pass
            assert want_n[q][3] == 4200 > 4096 and want_n[q][4] == 4200 and want_n[q][5] == (knn or 4200)
        assert want_n[1] == (4250, len(model[4250]), len(model[4250]), 1, 1, 1) and want_n[2][0] == A.NONE  # the short ones beside them
        got_e, got_n = ctx.graph_query(sk, len(model), 0.2, S.K, knn)
        assert _edges(got_e) == want_e, knn
        assert _near(got_n) == want_n, knn
        _counters_match(ctx.graph_query_counters(), want_n, len(want_e))


# ---- 3. rtc_leiden_place alone ---------------------------------------------------------------------------------------------
def _placements(p):
    return [tuple(int(x) for x in r) for r in p.tolist()]


def test_place_equals_the_restatement_on_every_row_path(ctx):
    from rabbittclust_amd import api
    labels, ncl, nq, records = S.place_case(LV_WAVE_ROW, LV_BLOCK_ROW, LV_WAVE_SLOTS)
    rec = np.array(records, dtype=api.WEDGE_DT)
    size = np.bincount(labels, minlength=ncl).astype(np.uint64)
    rng = np.random.default_rng(1)
    tot = (rng.integers(1, 1 << 24, ncl).astype(np.uint64) * size)
    m2 = int(tot.sum())
    for objective, t in ((CPM, size), (MODULARITY, tot)):
        for resolution in (0.001, 0.02, 60000.0):
            want = A.place_all(nq, records, labels, objective, resolution, t.tolist(), m2 if objective else 0)
            got = ctx.leiden_place(labels, ncl, nq, rec, resolution, objective, tot=tot if objective else None, m2=m2 if objective else 0)
            assert _placements(got) == want, (objective, resolution)
            c = ctx.leiden_place_counters()
            assert c["row_paths"] == 7 and c["records"] == len(records) and c["entries"] == sum(w[2] for w in want)
            assert (c["wave_rows"], c["workgroup_rows"], c["global_rows"]) == (4, 3, 2)
            assert c["placed"] == sum(1 for w in want if w[0] >= 0) and c["novel"] == nq - c["placed"]
            if resolution == 60000.0:  # 60 000 units a member, or 60 000 k_x tot_d against e_d M2: nothing is positive
                assert all(w == (-1, -1, w[2], w[3], w[4], 0, 0) for w in want), objective
            else:
                assert any(w[1] >= 0 for w in want)
    want = A.place_all(nq, records, labels, CPM, 0.001, size.tolist())
    assert want[0] == (-1, -1, 0, 0, 0, 0, 0) and [w[2] for w in want[1:7]] == [1, LV_WAVE_ROW, LV_WAVE_ROW + 1, LV_BLOCK_ROW, LV_BLOCK_ROW + 1, 2200]
    assert want[7][3] >= 300 > LV_WAVE_SLOTS // 2 and want[8][:2] == (12, 650) and want[9][4] >= 40 * 0xFFFFFFFF


# ---- 4. chunks --------------------------------------------------------------------------------------------------------------
def test_query_chunks_and_edge_budget(ctx):
    model, queries = S.query_case()
    sk = _set(ctx, model + queries, 8)
    want_e, want_n = _query_ref(3)
    for chunk in (1, 7):
        got_e, got_n = ctx.graph_query(sk, len(model), S.THRESHOLD, S.K, 3, query_chunk=chunk)
        assert _edges(got_e) == want_e and _near(got_n) == want_n, chunk
        c = ctx.graph_query_counters()
        assert c["chunks"] == -(-40 // chunk)
        _counters_match(c, want_n, len(want_e))
    with ctx.env(RTC_EDGE_BUDGET="64"):  # raised to n_db + 1 024 = 1 325: the 40 queries' 370-odd candidates fit, twice as many would not
        got_e, got_n = ctx.graph_query(sk, len(model), S.THRESHOLD, S.K, 3)
        assert _edges(got_e) == want_e and _near(got_n) == want_n
    model, queries = S.long_case()  # 8 400 candidates of four queries under a budget of 5 324: halved until the long ones are alone
    sk = _set(ctx, model + queries, 4)
    ref_e, ref_n = ctx.graph_query(sk, len(model), 0.2, S.K, 300)
    assert ctx.graph_query_counters()["chunks"] == 1
    with ctx.env(RTC_EDGE_BUDGET="64"):
        got_e, got_n = ctx.graph_query(sk, len(model), 0.2, S.K, 300)
        c = ctx.graph_query_counters()
    assert c["chunks"] > 1 and c["candidates"] == 8400 + 1
    assert np.array_equal(got_e, ref_e) and np.array_equal(got_n, ref_n)


# ---- 5. end to end through the ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["leiden-cpm", "leiden-modularity", "louvain"])
def test_build_then_assign_through_the_abi(ctx, run):
    from rabbittclust_amd import api, host
    model, queries, fam = S.holdout_case()
    n, knn = len(model), 50
    objective, resolution = (CPM, 0.3) if run == "leiden-cpm" else (MODULARITY, 1.0)
    sk_model, sk_all = _set(ctx, model, 4), _set(ctx, model + queries, 4)
    sizes = [len(s) for s in model]
    edges = ctx.graph_build(sk_model, S.THRESHOLD, S.K, knn)
    w = [api.graph_weight(int(e["common"]), sizes[e["u"]], sizes[e["v"]], S.K) for e in edges]
    if run == "louvain":
        rec = api.graph_weights(edges, sizes, S.K)
        labels = ctx.louvain(n, rec, resolution)
        ncl = ctx.louvain_clusters
        scale, lo, span = False, 0.0, 1.0
    else:
        rec, _ = host.leiden_quantise(edges["u"], edges["v"], w, objective)
        labels = ctx.leiden(n, rec, resolution, objective)
        ncl = ctx.leiden_clusters
        scale, lo, span, _ = host.leiden_quantiser(w, objective)
    assert labels.tolist() == fam and ncl == 10 and scale == (objective == CPM)
    k, tot, m2, size = host.leiden_model_sums(rec, labels, ncl)
    assert (k.tolist(), tot.tolist(), m2, size.tolist()) == A.model_sums(n, [(int(r["u"]), int(r["v"]), int(r["q"])) for r in rec], labels, ncl)
    qe, near = ctx.graph_query(sk_all, n, S.THRESHOLD, S.K, knn)
    qrec = host.leiden_assign_weights(qe, sizes, [len(s) for s in queries], S.K, objective, scale, lo, span, threads=4)
    got = ctx.leiden_place(labels, ncl, len(queries), qrec, resolution, objective, tot=tot if objective else None, m2=m2 if objective else 0)
    want, want_near, want_rec = A.assign(model, labels, queries, S.THRESHOLD, S.K, knn, objective, resolution, (tot if objective else size).tolist(),
                                         m2 if objective else 0, scale, lo, span, api.graph_weight)
    assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in qrec] == want_rec and _near(near) == want_near
    assert _placements(got) == want
    assert got["label"].tolist() == list(range(10)) + [-1] and int(near["nearest"][10]) == A.NONE


# ---- 6. error returns -------------------------------------------------------------------------------------------------------
def test_error_returns(ctx):
    from rabbittclust_amd import api
    E = api._lib
    sets = [np.arange(10), np.arange(5, 15), np.arange(3, 13), np.arange(4, 14)]
    sk = _set(ctx, sets, 8)

    def q_fails(status, text, *a, **kw):
        with pytest.raises(api.RtcError) as ei:
            ctx.graph_query(*a, **kw)
        assert ei.value.status == status and text in str(ei.value), str(ei.value)
        e, near = ctx.graph_query(sk, 2, 0.2, S.K)  # the context is as usable as before
        assert _edges(e) == [(0, 0, 7), (0, 1, 8), (1, 0, 6), (1, 1, 9)] and _near(near)[0] == (1, 8, 12, 2, 2, 2)
    q_fails(E.RTC_ERR_ARG, "threshold", sk, 2, 0.0, S.K)
    q_fails(E.RTC_ERR_ARG, "threshold", sk, 2, float("nan"), S.K)
    q_fails(E.RTC_ERR_ARG, "k-mer size", sk, 2, 0.2, 0)
    q_fails(E.RTC_ERR_OVERFLOW, "4 edges, room for 3", sk, 2, 0.2, S.K, cap=3)
    assert ctx.graph_edges_needed == 4
    e, _ = ctx.graph_query(sk, 2, 0.2, S.K, cap=ctx.graph_edges_needed)  # the repeated call with the reported count
    assert len(e) == 4
    with pytest.raises(ValueError):
        ctx.graph_query(sk, 5, 0.2, S.K)
    e, near = ctx.graph_query(sk, 4, 0.2, S.K)  # no query
    assert len(e) == 0 and len(near) == 0
    e, near = ctx.graph_query(sk, 0, 0.2, S.K)  # no model
    assert len(e) == 0 and _near(near) == [(A.NONE, 0, 0, 0, 0, 0)] * 4

    labels, rec = [0, 1, 1], [(0, 0, 5 << 20), (1, 2, 7 << 20)]  # 5 and 7 units against 0.001 a member

    def p_fails(status, text, *a, **kw):
        with pytest.raises(api.RtcError) as ei:
            ctx.leiden_place(*a, **kw)
        assert ei.value.status == status and text in str(ei.value), str(ei.value)
        got = ctx.leiden_place(labels, 2, 2, np.array(rec, dtype=api.WEDGE_DT), 0.001, "cpm")
        assert _placements(got) == [(0, -1, 1, 1, 5 << 20, 5 << 20, 0), (1, -1, 1, 1, 7 << 20, 7 << 20, 0)]

    def wedges(r):
        return np.array(r, dtype=api.WEDGE_DT)
    p_fails(E.RTC_ERR_ARG, "record 1", labels, 2, 2, wedges([(0, 0, 5), (2, 1, 1)]), 0.5, "cpm")  # u >= n_queries
    p_fails(E.RTC_ERR_ARG, "record 0", labels, 2, 2, wedges([(0, 3, 5)]), 0.5, "cpm")  # v >= n_db
    p_fails(E.RTC_ERR_ARG, "record 0", labels, 2, 2, wedges([(0, 1, 0)]), 0.5, "cpm")  # q = 0
    p_fails(E.RTC_ERR_ARG, "label 2", [0, 2, 1], 2, 2, wedges(rec), 0.5, "cpm")
    p_fails(E.RTC_ERR_ARG, "label -1", [0, -1, 1], 2, 2, wedges(rec), 0.5, "cpm")
    p_fails(E.RTC_ERR_ARG, "objective 2", labels, 2, 2, wedges(rec), 0.5, 2)
    p_fails(E.RTC_ERR_ARG, "h_tot", labels, 2, 2, wedges(rec), 0.5, "modularity")
    for bad in (0.0, -1.0, float("nan"), 65536.0):
        p_fails(E.RTC_ERR_ARG, "resolution", labels, 2, 2, wedges(rec), bad, "cpm")
    p_fails(E.RTC_ERR_UNSUPPORTED, "2^46", labels, 2, 2, wedges(rec), 1.0, "modularity", tot=[1 << 45, 1 << 45], m2=1 << 46)
    p_fails(E.RTC_ERR_UNSUPPORTED, "query 1", labels, 2, 2, wedges([(1, 0, 0xFFFFFFFF)] * 4), 1.0, "modularity", tot=[1 << 44, 1 << 44],
            m2=(1 << 46) - (1 << 34))
    got = ctx.leiden_place(labels, 2, 3, wedges([]), 0.5, "cpm")  # no record: everything is novel
    assert _placements(got) == [(-1, -1, 0, 0, 0, 0, 0)] * 3
    assert len(ctx.leiden_place(labels, 2, 0, wedges([]), 0.5, "cpm")) == 0


# ---- 7. the command line ----------------------------------------------------------------------------------------------------
def _cli(args, cwd, env=None):
    r = subprocess.run([os.path.join(BIN, "clust-leiden")] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


_CLI = {}


def _cli_case(oracle, tmp):
    """20 model genomes of 1 Mbp in four families and the 40-query shape as FASTA files: 34 further family members at four
    substitution rates, a copy of a model genome, a poly-A record (an empty sketch), two unrelated genomes, a model genome inside
    3 Mbp (only the size ratio fails), one genome built from two families' halves"""
    from rabbittclust_amd import api
    L, k = 1_000_000, 17
    _, seqs, meta = _write_fastas(oracle, tmp, 4, 5, L, seed=9)
    desc = api.synth_family_descs(4, 5, global_seed=9)
    anc = [seqs[5 * f] for f in range(4)]
    qs = [oracle.synth_genome(int(desc[5 * (i % 4)]["fam_seed"]), 1000 + i, int((0.005, 0.02, 0.05, 0.1)[(i // 4) % 4] * 16384), L) for i in range(34)]
    other = api.synth_family_descs(3, 1, global_seed=77)
    fresh = [oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), 0, L) for d in other]
    qs += [seqs[7].copy(), np.full(20_000, ord("A"), np.uint8), fresh[0], fresh[1], np.concatenate([seqs[11], fresh[2], fresh[0][::-1].copy()]),
           np.concatenate([anc[0][:L // 2], anc[3][L // 2:]])]
    assert len(qs) == 40
    qdir = os.path.join(tmp, "q"); os.makedirs(qdir)
    paths = []
    for i, s in enumerate(qs):
        p = os.path.join(qdir, "q%02d.fna" % i)
        with open(p, "wb") as f:
            f.write((">q%d query %d\n" % (i, i)).encode() + s.tobytes() + b"\n")
        paths.append(p)
    q_list = os.path.join(tmp, "q.txt")
    open(q_list, "w").write("".join(p + "\n" for p in paths))
    fa = os.path.join(tmp, "queries.fna")
    with open(fa, "wb") as f:
        for i, s in enumerate(qs):
            f.write((">r%d query %d\n" % (i, i)).encode() + s.tobytes() + b"\n")
    db_list = os.path.join(tmp, "db.txt")
    open(db_list, "w").write("".join(m[0] + "\n" for m in meta))
    return dict(k=k, meta=meta, db_list=db_list, q_list=q_list, q_paths=paths, fa=fa, db_sk=[oracle.kssd_sketch(s, k, 3) for s in seqs],
                q_sk=[oracle.kssd_sketch(s, k, 3) for s in qs])


@pytest.mark.parametrize("algorithm", ["louvain", "leiden"])
def test_cli_build_stats_assign(oracle, tmp_path, algorithm):
    from rabbittclust_amd import api
    tmp = str(tmp_path)
    c = _cli_case(oracle, tmp)
    k, threshold, knn = c["k"], 0.08, 10
    flags = ["--louvain"] if algorithm == "louvain" else ["--leiden", "--objective", "cpm", "--resolution", "0.3"]
    objective, resolution = (MODULARITY, 1.0) if algorithm == "louvain" else (CPM, 0.3)
    common = ["--fast"] + flags + ["-l", "-i", c["db_list"], "-k", str(k), "-d", str(threshold), "--knn", str(knn), "-t", "4", "-e"]
    plain, built, db = os.path.join(tmp, "plain.out"), os.path.join(tmp, "built.out"), os.path.join(tmp, "model.ldb")
    _cli(common + ["-o", plain], tmp)
    err = _cli(common + ["--db", db, "--build", "-o", built], tmp)
    assert open(built, "rb").read() == open(plain, "rb").read() and "-----write the Leiden model (20 genomes" in err and not os.path.exists(db + ".tmp")
    blob = open(db, "rb").read()
    m = A.parse_model(blob)
    # the model holds what the restatement of the run gives
    weighted = refgraph.weighted(refgraph.edges(c["db_sk"], threshold, k, knn), c["db_sk"], k)
    records, _ = refleiden.normalise_and_quantise(weighted, objective)
    if algorithm == "louvain":
        labels, ncl = reflouvain.louvain(20, records, resolution)[:2]
    else:
        labels, ncl, _ = refleiden.leiden(20, records, resolution, objective)
    _, tot, m2, size = A.model_sums(20, records, labels, ncl)
    w = [x for _, _, x in weighted]
    lo, hi = min([1.0] + w), max([0.0] + w)
    scale = objective == CPM and hi - lo < 0.5 and hi - lo > 1e-6
    assert (m["version"], m["algorithm"], m["objective"], m["width"], m["by_file"], m["kmer_size"], m["half_k"], m["drlevel"], m["knn"]) == \
        (1, int(algorithm == "leiden"), objective, 4, 1, k, 9, 3, knn)
    assert (m["n"], m["n_clusters"], m["min_len"], m["threshold"], m["resolution"], m["scale"]) == (20, ncl, 10000, threshold, resolution, int(scale))
    assert m["labels"].tolist() == labels and m["tot"].tolist() == (tot if objective else size) and m["m2"] == (m2 if objective else 0)
    if objective == CPM:
        assert (m["lo"], m["range"]) == (lo, hi - lo)
    assert all(np.array_equal(a, b) for a, b in zip(m["sketches"], c["db_sk"]))
    assert [(g["file"], g["total_length"], g["name"], g["comment"]) for g in m["genomes"]] == c["meta"]
    # --stats: no GPU
    r = subprocess.run([os.path.join(BIN, "clust-leiden"), "--db", db, "--stats"], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and "Genomes:     20" in r.stdout and "Clusters:    %d" % ncl in r.stdout and "Knn:         10" in r.stdout
    assert ("Algorithm:   " + algorithm.capitalize()) in r.stdout and "no MI355X context" not in r.stderr
    # --assign: the lines the restatement predicts from the model file and the queries' oracle sketches
    want, near, _ = A.assign(m["sketches"], m["labels"], c["q_sk"], threshold, k, knn, objective, resolution, m["tot"].tolist(), m["m2"], bool(m["scale"]),
                             m["lo"], m["range"], api.graph_weight)
    assert len(c["q_sk"][35]) == 0 and near[35][0] == A.NONE and near[36][0] == A.NONE and near[38][3] > 0 and near[38][4] == 0
    assert sum(1 for x in want if x[0] >= 0) >= 10 and want[34][0] == labels[7]
    names = [g["file"] for g in m["genomes"]]
    msz = [len(s) for s in m["sketches"]]
    header = "query\tcluster\trunner_up\tedges\tcommunities\tweight\tshare\tnearest\tdistance\n"

    def tsv(qnames):
        return header + "".join(A.tsv_line(qn, want[i], near[i], names, len(c["q_sk"][i]), msz, k, api.graph_weight) + "\n" for i, qn in enumerate(qnames))
    out1, out2, mj = os.path.join(tmp, "assign.tsv"), os.path.join(tmp, "assign2.tsv"), os.path.join(tmp, "assign.json")
    _cli(["--db", db, "--assign", "-l", "-i", c["q_list"], "-k", "31", "-d", "0.9", "--resolution", "7", "--knn", "3", "--louvain", "-t", "4", "-o", out1],
         tmp, env={"RTC_METRICS_JSON": mj})
    assert open(out1).read() == tsv(c["q_paths"])
    metrics = json.load(open(mj))
    assert metrics["command"] == "clust-leiden"
    for key in ("leiden_assign_query_s", "leiden_assign_weights_s", "leiden_assign_place_s"):
        assert metrics[key] >= 0, key
    placed = sum(1 for x in want if x[0] >= 0)
    assert (metrics["leiden_assign_placed"], metrics["leiden_assign_novel"]) == (placed, 40 - placed)
    _cli(["--db", db, "--assign", "-i", c["fa"], "-t", "4", "-o", out2], tmp)
    assert open(out2).read() == tsv(["r%d" % i for i in range(40)])
    assert open(db, "rb").read() == blob  # --assign leaves the model as it was
