"""clust-dbscan --db --update without a GPU: the two-stage rule (tests/refdbscan_update.py) held against the full-run
restatements of both kinds (tests/refdbscan.py, tests/refdbscan_mash.py) on the union, the crafted sets' events, the model file
rewritten by the update path, and the flag errors, which exit before any GPU is asked for."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refdbscan_assign as A
from tests import refdbscan_mash as M
from tests import refdbscan_update as U
from tests import sweep_sets
from tests.test_cpu_dbscan_assign import _model_bytes, _run

K = U.GRAPH_K


def full_kssd(sketches, eps, min_pts, use64):
    """the reference's walk and the core flags on a whole set"""
    nb = R.neighbour_lists(sketches, eps, K, use64)
    lab, _ = R.sequential_walk(nb, min_pts)
    return np.array([x if x >= 0 else -1 for x in lab], dtype=np.int32), np.array([len(x) + 1 >= min_pts for x in nb], dtype=bool)


def full_mash(sketches, sketch_size, eps, min_pts):
    return M.labels_of(M.distance_matrix(M.count_matrix(sketches, sketch_size), K), eps, min_pts)


def full(sketches, kind, eps, min_pts, use64=False, sketch_size=U.GRAPH_SKETCH_SIZE):
    return full_mash(sketches, sketch_size, eps, min_pts) if kind == "minhash" else full_kssd(sketches, eps, min_pts, use64)


def relation(sketches, kind, eps, use64=False, sketch_size=U.GRAPH_SKETCH_SIZE):
    return U.mash_relation(sketches, sketch_size, eps, K) if kind == "minhash" else U.kssd_relation(sketches, eps, K, use64)


def random_graph(rng, n, max_deg=5):
    """clumps of a few points with edges inside, a few edges between clumps, every degree at most max_deg"""
    deg, edges = [0] * n, set()
    clump = rng.integers(0, max(2, n // 4), size=n)
    for _ in range(int(n * rng.uniform(0.6, 1.6))):
        u, v = (int(x) for x in rng.integers(0, n, size=2))
        if u == v or (clump[u] != clump[v] and rng.random() < 0.85):
            continue
        e = (max(u, v), min(u, v))
        if e in edges or deg[u] >= max_deg or deg[v] >= max_deg:
            continue
        edges.add(e)
        deg[u] += 1
        deg[v] += 1
    return sorted(edges)


def check_update(sketches, n_old, kind, eps, min_pts, use64=False, sketch_size=U.GRAPH_SKETCH_SIZE):
    """the full run on the first n_old, the update with the rest, against the full run on all: the restatement's info"""
    lab_old, core_old = full(sketches[:n_old], kind, eps, min_pts, use64, sketch_size)
    want, want_core = full(sketches, kind, eps, min_pts, use64, sketch_size)
    got, got_core, info = U.update(n_old, len(sketches), relation(sketches, kind, eps, use64, sketch_size), lab_old, core_old,
                                   U.need_of(min_pts, kind == "minhash"))
    assert np.array_equal(got, want) and np.array_equal(got_core, want_core), (kind, n_old, min_pts, got.tolist(), want.tolist())
    old_noise_or_border = int((~core_old).sum())
    assert len(info["rows2"]) <= old_noise_or_border and all(not core_old[v] for v in info["rows2"])
    return info


def test_rule_equals_the_full_run_on_random_sets():
    seen, sets = set(), 0
    for seed in range(160):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(8, 61))
        sk = U.graph_sketches(n, random_graph(rng, n), rng, use64=bool(seed & 1))
        n_old = int(rng.integers(1, n))
        for kind in ("kssd", "minhash"):
            min_pts = 1 + (seed + (kind == "minhash")) % 5
            seen |= check_update(sk, n_old, kind, U.GRAPH_EPS, min_pts, use64=bool(seed & 1))["events"]
            sets += 1
    # sketch sets with real size spread: families, a chain, loners, empty sketches at both widths
    for seed in range(24):
        use64 = bool(seed & 1)
        sk = sweep_sets.family_sets(seed, use64, n_empty=(0, 2, 3)[seed % 3])
        rng = np.random.default_rng(seed)
        n_old = int(rng.integers(5, len(sk) - 2))
        for min_pts in (1 + seed % 5, 1 + (seed + 2) % 5):
            seen |= check_update(sk, n_old, "kssd", (0.02, 0.04, 0.06)[seed % 3], min_pts, use64=use64)["events"]
            mh = [np.asarray(s, dtype=np.uint64) for s in sk]
            seen |= check_update(mh, n_old, "minhash", (0.02, 0.04, 0.06)[seed % 3], min_pts - 1, sketch_size=256)["events"]
            sets += 2
    assert sets >= 400
    # (a relabelled border point needs a promoted point below every core point of a cluster: the crafted set has it)
    assert {"noise promoted", "border promoted", "clusters merged", "new cluster"} <= seen, seen


def test_three_successive_updates():
    for seed in range(12):
        rng = np.random.default_rng(77 + seed)
        n = 60
        sk = U.graph_sketches(n, random_graph(rng, n), rng)
        cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(5, n - 1), size=3, replace=False)) + [n]
        for kind in ("kssd", "minhash"):
            min_pts = 2 + seed % 3
            need = U.need_of(min_pts, kind == "minhash")
            lab, core = full(sk[:cuts[1]], kind, U.GRAPH_EPS, min_pts)
            for a, b in zip(cuts[1:-1], cuts[2:]):
                lab, core, _ = U.update(a, b, relation(sk[:b], kind, U.GRAPH_EPS), lab, core, need)
                want, want_core = full(sk[:b], kind, U.GRAPH_EPS, min_pts)
                assert np.array_equal(lab, want) and np.array_equal(core, want_core), (seed, kind, a, b)


@pytest.mark.parametrize("event", sorted(U.CRAFTED))
def test_crafted_sets_exercise_their_event(event):
    n_old, n, edges, min_pts = U.CRAFTED[event]
    for kind, use64 in (("kssd", False), ("kssd", True), ("minhash", True)):
        sk = U.graph_sketches(n, edges, np.random.default_rng(3), use64=use64)
        info = check_update(sk, n_old, kind, U.GRAPH_EPS, min_pts - (kind == "minhash"), use64=use64)
        assert event in info["events"], (event, kind, info)
    if event == "border relabelled":  # the bridging border point 7 moves from the first star's cluster to the second's
        sk = U.graph_sketches(n, edges, np.random.default_rng(3))
        old, _ = full_kssd(sk[:n_old], U.GRAPH_EPS, min_pts, False)
        new, _ = full_kssd(sk, U.GRAPH_EPS, min_pts, False)
        assert old[7] == old[4] != old[8] and new[7] == new[8] != new[4]


def test_rows_are_few_where_the_old_points_are_core():
    """the set of tests/test_gpu_dbscan_update.py's row bound: cliques of five (all core at min_pts 3), a few border points, pairs and loners"""
    sk, n_old = U.mostly_core_set(np.random.default_rng(8))
    info = check_update(sk, n_old, "kssd", U.GRAPH_EPS, 3)
    assert len(info["rows2"]) < n_old // 4 and info["rows2"], info["rows2"]


# ---- the model file -----------------------------------------------------------------------------------------------------
def test_update_path_with_no_new_genome_rewrites_the_same_bytes(tmp_path):
    from rabbittclust_amd import host
    lib = host.load()
    for kind, width in ((0, 4), (0, 8), (1, 8)):
        blob = _model_bytes(kind, width)
        path = os.path.join(str(tmp_path), "m%d%d.db" % (kind, width))
        open(path, "wb").write(blob)
        assert lib.rtch_dbscan_model_update(path.encode(), 0, None, None, None, None, None, None, 0) == 0
        assert open(path, "rb").read() == blob and not os.path.exists(path + ".tmp")
        # one genome appended: the records and sketches follow the old ones, the labels, flags and cluster count are replaced
        dt = np.uint64 if width == 8 else np.uint32
        h = np.arange(14, 24, dtype=dt)
        off = np.array([0, len(h)], dtype=np.uint64)
        names = (C.c_char_p * 1)(b"new.fna")
        lens = np.array([777], dtype=np.uint64)
        labels, core = np.array([0, 0, -1, 0], dtype=np.int32), np.array([1, 1, 0, 1], dtype=np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert lib.rtch_dbscan_model_update(path.encode(), 1, names, vp(lens), vp(h), vp(off), vp(labels), vp(core), 1) == 0
        m, m0 = A.parse_model(open(path, "rb").read()), A.parse_model(blob)
        assert m["n"] == 4 and m["labels"].tolist() == [0, 0, -1, 0] and m["core"].tolist() == [1, 1, 0, 1] and m["n_clusters"] == 1
        assert m["genomes"][:3] == m0["genomes"] and m["genomes"][3]["file"] == "new.fna" and m["genomes"][3]["total_length"] == 777
        assert all(np.array_equal(a, b) for a, b in zip(m["sketches"][:3], m0["sketches"])) and m["sketches"][3].tolist() == h.tolist()
        for f in ("version", "kind", "width", "by_file", "kmer_size", "min_pts", "max_posting", "eps", "min_len"):
            assert m[f] == m0[f], f


# ---- the command line ---------------------------------------------------------------------------------------------------
UPD = ["--update", "-l", "-i", "list.txt", "-o", "o.dbscan"]


@pytest.mark.parametrize("args,msg", [
    (["--fast", "--db", "m.db", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --db requires exactly one of --build, --assign, --stats, --update"),
    (["--fast", "--db", "m.db", "--build", "--update", "-l", "-i", "list.txt", "-o", "o.txt"],
     "ERROR: --db requires exactly one of --build, --assign, --stats, --update"),
    (["--fast", "--db", "m.db", "--assign", "--update", "-l", "-i", "list.txt", "-o", "o.txt"],
     "ERROR: --db requires exactly one of --build, --assign, --stats, --update"),
    (["--fast"] + UPD, "ERROR: --update requires --db"),
    (["--db", "missing.db"] + UPD, "ERROR: --db missing.db: cannot open"),
    (["--db", "kssd.db", "--update", "-l", "-o", "o.dbscan"], "ERROR: --update requires -i <input_file>"),
    (["--db", "kssd.db", "--knn", "5"] + UPD, "ERROR: --knn does not go with --db"),
    (["--db", "kssd.db", "--eps-sweep", "0.01,0.02"] + UPD, "ERROR: --update does not go with --eps-sweep"),
    (["--db", "kssd.db", "--kdist"] + UPD, "ERROR: --update does not go with --kdist"),
    (["--db", "kssd.db", "--hierarchy"] + UPD, "ERROR: --update does not go with --hierarchy"),
    (["--db", "kssd.db", "--max-posting", "5"] + UPD, "ERROR: --update does not go with --max-posting"),
    (["--db", "mp.db"] + UPD, "ERROR: --update: mp.db was built with --max-posting 7, which is out of scope"),
    (["--db", "kssd.db", "--update", "-i", "more.fna", "-o", "o.dbscan"], "ERROR: --update: kssd.db was built with -l"),
    (["--minhash", "--db", "kssd.db"] + UPD, "ERROR: --update: --minhash given, but kssd.db is a KSSD model"),
    (["--fast", "--db", "mh.db"] + UPD, "ERROR: --update: --fast given, but mh.db is a MinHash model"),
    (["--fast", "--db", "kssd.db", "--append", "list.txt", "-o", "o.txt"], "ERROR: --append not supported for DBSCAN clustering"),
    (["--fast", "--append", "list.txt", "-o", "o.txt"], "ERROR: --append not supported for DBSCAN clustering"),
])
def test_flag_errors_before_the_gpu(args, msg, tmp_path):
    tmp = str(tmp_path)
    for name, blob in (("kssd.db", _model_bytes(0, 4)), ("mh.db", _model_bytes(1, 8)), ("mp.db", _model_bytes(0, 4, max_posting=7))):
        open(os.path.join(tmp, name), "wb").write(blob)
    before = open(os.path.join(tmp, "kssd.db"), "rb").read()
    r = _run(args, cwd=tmp)
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr
    assert open(os.path.join(tmp, "kssd.db"), "rb").read() == before and not os.path.exists(os.path.join(tmp, "o.dbscan"))


def test_help_names_update():
    r = _run(["-h"])
    assert r.returncode == 0 and "--update" in r.stdout
    for other in ("clust-mst", "clust-greedy", "clust-leiden"):  # the flag belongs to clust-dbscan alone
        import subprocess
        from tests.test_cpu_dbscan_assign import BIN
        q = subprocess.run([os.path.join(os.path.dirname(BIN), other), "--update", "-l", "-i", "x", "-o", "y"], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
        assert q.returncode != 0 and "context" not in q.stderr, (other, q.stderr)
