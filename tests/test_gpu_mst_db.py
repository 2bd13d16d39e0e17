"""GPU suite: rtc_rep_topk against a brute force with exact keys (tests/refmstdb.py), and clust-mst --db --build / --query /
--assign / --append end to end against the --save-rep state, tests/refmststate.py and tests/refmstdb.py."""
import os

import numpy as np
import pytest

import refmstdb as D
import refmststate as M
from test_gpu_mst_state import _folders, _genomes, _run, _sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


def _search_set(rng, width):
    """5 000 representatives and 40 queries of about 40 hashes: one hash shared by 4 900 representatives and query 0 (the
    long segment), duplicated representatives (equal keys), queries from a disjoint range (no candidate)"""
    hmax = (1 << 62) if width == 8 else (1 << 31) - 1
    pool = np.unique(rng.integers(1000, 1000 + 30_000, size=30_000, dtype=np.int64))
    hub = 7
    reps = []
    for r in range(5000):
        s = set(int(x) for x in rng.choice(pool, size=int(rng.integers(20, 60)), replace=False))
        if r < 4900:
            s.add(hub)
        reps.append(sorted(s))
    for r in range(0, 300, 3):  # duplicates of earlier representatives
        reps[4900 + r // 3] = list(reps[r])
    queries = []
    for q in range(40):
        if q % 10 == 9:  # shares nothing with any representative
            queries.append(sorted(int(x) for x in rng.integers(hmax // 2, hmax, size=30)))
            continue
        s = set(int(x) for x in rng.choice(pool, size=int(rng.integers(10, 70)), replace=False))
        if q % 5 == 0:
            s.add(hub)
        if q % 7 == 3:
            s |= set(reps[q * 50])  # a close relative of one representative
        queries.append(sorted(s))
    live = (rng.random(len(reps)) > 0.1).astype(np.uint8)
    dt = np.uint64 if width == 8 else np.uint32
    return [np.asarray(x, dtype=dt) for x in reps], [np.asarray(x, dtype=dt) for x in queries], live


@pytest.mark.gpu
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("mode", [0, 1, 2 | (32 << 2)])
def test_rep_topk_equals_brute_force(ctx, width, mode):
    from rabbittclust_amd import api
    rng = np.random.default_rng(width * 7 + mode)
    reps, queries, live = _search_set(rng, width)
    R = len(reps)
    s = api.SketchSet.from_host(reps + queries, ctx.device, k=21, width=width)
    full = D.topk(reps, queries, mode, 0, live)
    assert len(full[0]) > 4096, "query 0 must take the long-segment path"
    assert any(not h for h in full) and any(len(set((c, d) for _, c, d in h)) < len(h) for h in full), "no empty / no tied query"
    assert live[:4900].min() == 0, "no retired slot among the long segment's candidates"
    for k in (1, 5, 64, 256, 257, 0):
        want = [h if k == 0 else h[:k] for h in full]
        for chunk in (0, 7):
            got, per = ctx.rep_topk(s, R, mode, k, live=live, query_chunk=chunk)
            assert per.tolist() == [len(h) for h in want]
            flat = [(q, sl, c, d) for q, h in enumerate(want) for sl, c, d in h]
            assert [tuple(int(x) for x in g) for g in got] == flat, (k, chunk)
            cnt = ctx.rep_topk_counters()
            assert cnt["chunks"] == (1 if chunk == 0 else 6)
            path = ctx.rep_topk_last_path()
            assert path == (4 if k in (0, 257) else 3), path
            o = 0
            for q in range(len(queries)):  # distances never decrease within a query
                ds = [D.distance(int(g["common"]), int(g["denom"]), mode, 21) for g in got[o:o + per[q]]]
                assert ds == sorted(ds)
                o += per[q]
    if mode & 3 == 2:  # the union-truncated counts are rtc_pair_mash_dev's
        c, d = ctx.pair_mash(s, mode >> 2, row0=R, row1=R + len(queries), col0=0, col1=R)
        c, d = c.cpu().numpy(), d.cpu().numpy()
        got, _ = ctx.rep_topk(s, R, mode, 0, live=live)
        for g in got:
            assert (int(g["common"]), int(g["denom"])) == (int(c[g["query"], g["slot"]]), int(d[g["query"], g["slot"]]))


def _db_state(path):
    st, _ = M.parse(open(path, "rb").read())
    return st


def _fasta(tmp, seqs, name):
    p = os.path.join(tmp, name)
    with open(p, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">rec%d\n" % i + s.tobytes() + b"\n")
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [True, False])
def test_db_build_query_assign_append(oracle, tmp_path, fast):
    tmp = str(tmp_path)
    mst = os.path.join(BIN, "clust-mst")
    lst_a, paths_a, seqs_a = _genomes(oracle, tmp, "a", 3, 4, 300_000, seed=41)
    lst_b, paths_b, seqs_b = _genomes(oracle, tmp, "b", 4, 3, 300_000, seed=42)
    fl = ["--fast"] if fast else []
    par = ["-k", "21", "-d", "0.05", "-t", "4"] + ([] if fast else ["-s", "1000"])
    # a sketch folder of A, then the --save-rep state and the --db build from it: the same bytes, the same cluster file
    _run([mst] + fl + ["-l", "-i", lst_a, "-o", os.path.join(tmp, "a.out")] + par, tmp)
    (folder,) = _folders(tmp)
    _run([mst] + fl + ["--presketched", folder, "--save-rep", "-e", "-o", os.path.join(tmp, "p.out"), "-d", "0.05", "-t", "4"], tmp)
    db = os.path.join(tmp, "rep.mstdb")
    _run([mst] + fl + ["--db", db, "--build", "--presketched", folder, "-d", "0.05", "-o", os.path.join(tmp, "b.out"), "-t", "4"], tmp)
    state_path = os.path.join(folder, "mst_cluster_state.bin")
    assert open(db, "rb").read() == open(state_path, "rb").read()
    assert open(os.path.join(tmp, "b.out"), "rb").read() == open(os.path.join(tmp, "p.out"), "rb").read()
    # from the genome list: no sketch folder
    db2 = os.path.join(tmp, "rep2.mstdb")
    _run([mst] + fl + ["--db", db2, "--build", "-l", "-i", lst_a, "-o", os.path.join(tmp, "g.out")] + par, tmp)
    assert _folders(tmp) == [folder]
    assert os.path.exists(db2)
    st = _db_state(db)
    assert len(st.rep_hashes) < len(paths_a), "every cluster is a singleton: the test shows nothing"
    live = [1 if c else 0 for c in st.clusters]
    # --query / --assign, from a list and from one FASTA file whose records are the queries
    q_seqs = seqs_b + seqs_a[:2]
    q_paths = paths_b + paths_a[:2]
    lst_q = os.path.join(tmp, "q.txt")
    open(lst_q, "w").write("\n".join(q_paths) + "\n")
    qsk = _sketch(oracle, q_seqs, st)
    fa = _fasta(tmp, q_seqs, "q.fa")
    for k in (1, 3, 257):
        hits = D.topk(st.rep_hashes, qsk, D.wmode(st), k, live)
        out = os.path.join(tmp, "q%d.tsv" % k)
        _run([mst] + fl + ["--db", db, "--query", "-l", "-i", lst_q, "--top-k", str(k), "-o", out, "-t", "4"], tmp)
        assert open(out).read() == D.query_tsv(st, q_paths, hits)
    out = os.path.join(tmp, "qf.tsv")
    _run([mst] + fl + ["--db", db, "--query", "-i", fa, "--top-k", "5", "-o", out, "-t", "4"], tmp)
    assert open(out).read() == D.query_tsv(st, [""] * len(q_seqs), D.topk(st.rep_hashes, qsk, D.wmode(st), 5, live))
    hits1 = D.topk(st.rep_hashes, qsk, D.wmode(st), 1, live)
    for args, names in ((["-l", "-i", lst_q], q_paths), (["-i", fa], [""] * len(q_seqs))):
        out = os.path.join(tmp, "as.tsv")
        _run([mst] + fl + ["--db", db, "--assign"] + args + ["-o", out, "-t", "4"], tmp)
        text = open(out).read()
        assert text == D.assign_tsv(st, names, hits1)
    assert "\tassigned\n" in text
    # --db --append: the bytes --append --presketched --save-rep writes from the same state, and the same cluster file
    _run([mst] + fl + ["--db", db, "--append", lst_b, "-l", "-o", os.path.join(tmp, "da.out"), "-t", "4"], tmp)
    _run([mst] + fl + ["--append", lst_b, "--presketched", folder, "--save-rep", "-l", "-o", os.path.join(tmp, "pa.out"), "-t", "4"], tmp)
    assert open(db, "rb").read() == open(state_path, "rb").read()
    assert open(os.path.join(tmp, "da.out"), "rb").read() == open(os.path.join(tmp, "pa.out"), "rb").read()
    want = st  # and the restatement's replay of the same append
    M.append(want, paths_b, [len(s) for s in seqs_b], _sketch(oracle, seqs_b, st))
    assert open(db, "rb").read() == M.save(want)


@pytest.mark.gpu
def test_db_build_minhash_containment_stores_c(oracle, tmp_path):
    tmp = str(tmp_path)
    mst = os.path.join(BIN, "clust-mst")
    lst, paths, seqs = _genomes(oracle, tmp, "c", 2, 3, 300_000, seed=43)
    db = os.path.join(tmp, "c.mstdb")
    _run([mst, "--db", db, "--build", "-l", "-i", lst, "-c", "500", "-d", "0.05", "-o", os.path.join(tmp, "c.out"), "-t", "4"], tmp)
    st = _db_state(db)
    assert st.is_containment and st.contain_compress == 500
    assert _folders(tmp) == []
