"""CPU suite: clust-mst post-processing without a GPU -- --auto-threshold / --stability on --premsted folders and the host
--dedup-dist / --reps-per-cluster functions, against the Python restatement of the reference (tests/refpost.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import refpost as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, "rabbittclust_amd", "librtclust_host.so")
MST_BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-mst")
EDGE = np.dtype([("preNode", "<i4"), ("sufNode", "<i4"), ("dist", "<f8")])


def _bin():
    if not os.path.exists(MST_BIN):
        pytest.fail("clust-mst missing: run __graft_entry__.build()")
    return MST_BIN


def _folder(path, n, edges, kssd=False):
    """a --premsted folder: (kssd.)info.mst (file list mode) + edge.mst"""
    path.mkdir()
    with open(path / ("kssd.info.mst" if kssd else "info.mst"), "wb") as f:
        f.write(struct.pack("<?Q", True, n))
        for i in range(n):
            fn, name, cm = f"/data/g{i}.fna", f"seq{i}", "noName"
            f.write(struct.pack("<iiiiQ", len(fn), len(name), len(cm), 0, 1_000_000 + 13 * i))
            f.write(fn.encode() + name.encode() + cm.encode())
            if kssd:
                f.write(struct.pack("<?", False))
    with open(path / "edge.mst", "wb") as f:
        f.write(struct.pack("<Q", len(edges)))
        for a, b, d in edges:
            f.write(struct.pack("<iid", a, b, d))
    return str(path)


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _tree(rng, n, weights):
    return [(i, int(rng.integers(0, i)), float(w)) for i, w in zip(range(1, n), weights)]


def _distinct_gap_weights(rng, m, scale):
    """m sorted-distinct weights whose adjacent gaps are pairwise distinct (the gap sort's order is then unique)"""
    gaps = rng.permutation(np.arange(1, 4 * m + 1))[:m] * scale
    return rng.permutation(np.cumsum(gaps))


def _mst_cases():
    rng = np.random.default_rng(5)
    cases = {}
    cases["random"] = (60, _tree(rng, 60, _distinct_gap_weights(rng, 59, 1e-4)))
    cases["wide"] = (300, _tree(rng, 300, _distinct_gap_weights(rng, 299, 3e-5)))
    w = _distinct_gap_weights(rng, 30, 2e-3)
    w[:8] = 0.0  # zero edges: identical genomes, left out of the distribution
    cases["zeros"] = (31, _tree(rng, 31, w))
    cases["all_zero"] = (12, _tree(rng, 12, np.zeros(11)))
    cases["one_value"] = (9, _tree(rng, 9, np.full(8, 0.02)))
    cases["far"] = (40, _tree(rng, 40, 0.3 + _distinct_gap_weights(rng, 39, 1e-3)))  # nothing near -d 0.05
    cases["forest"] = (50, _tree(rng, 50, _distinct_gap_weights(rng, 49, 2e-4))[:30])  # 20 genomes on their own
    cases["tiny"] = (3, [(1, 0, 0.01), (2, 1, 0.04)])
    return cases


CASES = _mst_cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("stability", [False, True])
def test_auto_threshold_analysis_file_matches_restatement(tmp_path, name, stability):
    n, edges = CASES[name]
    src = _folder(tmp_path / "mst", n, edges)
    plain, out = str(tmp_path / "plain.out"), str(tmp_path / "auto.out")
    _run([_bin(), "--premsted", src, "-d", "0.05", "-o", plain])
    err = _run([_bin(), "--premsted", src, "-d", "0.05", "-o", out, "--auto-threshold"] + (["--stability"] if stability else []))
    want, opt = R.analysis_text(edges, 0.05, stability, n)
    assert open(out + ".threshold_analysis.txt").read() == want
    assert open(out, "rb").read() == open(plain, "rb").read()  # -d still cuts the forest
    assert "-----optimal threshold: " in err and "-----threshold analysis written to: " + out + ".threshold_analysis.txt" in err
    assert ("-----stability evaluation enabled" in err) == stability
    if stability:
        assert "-----near edges: %d, clusters: %d" % (opt["near"], opt["clusters"]) in err


@pytest.mark.parametrize("m", [0, 1])
def test_auto_threshold_needs_two_edges(tmp_path, m):
    src = _folder(tmp_path / "mst", 4, [(1, 0, 0.01)][:m])
    out = str(tmp_path / "o.out")
    err = _run([_bin(), "--premsted", src, "-d", "0.05", "-o", out, "--auto-threshold", "--stability"])
    assert not os.path.exists(out + ".threshold_analysis.txt")
    assert ("MST is empty" in err) if m == 0 else ("MST has only 1 edge(s)" in err)


def test_stability_alone_reports_on_stderr(tmp_path):
    n, edges = CASES["random"]
    src = _folder(tmp_path / "mst", n, edges)
    out = str(tmp_path / "o.out")
    err = _run([_bin(), "--premsted", src, "-d", "0.03", "-o", out, "--stability"])
    assert not os.path.exists(out + ".threshold_analysis.txt")
    overall, split, merge, near = R.stability(edges, 0.03, n)
    nc = len(R.clusters_bfs(R.forest(edges, 0.03), n))
    assert "-----evaluating stability for threshold: 0.03..." in err
    assert "-----near edges evaluated: %d, clusters: %d" % (near, nc) in err
    assert "-----threshold stability: %s" % ("%g" % overall) in err


def test_kssd_premsted_accepts_the_flags_without_effect(tmp_path):
    """clust_from_mst_fast (--fast --premsted, src/sub_command.cpp:1760-1822) has no edge-length analysis"""
    n, edges = CASES["random"]
    src = _folder(tmp_path / "mst", n, edges, kssd=True)
    plain, out = str(tmp_path / "plain.out"), str(tmp_path / "o.out")
    _run([_bin(), "--fast", "--premsted", src, "-d", "0.05", "-o", plain])
    _run([_bin(), "--fast", "--premsted", src, "-d", "0.05", "-o", out, "--auto-threshold", "--stability", "--dedup-dist", "0.01",
          "--reps-per-cluster", "2"])
    assert open(out, "rb").read() == open(plain, "rb").read()
    for ext in (".threshold_analysis.txt", ".dedup", ".reps"):
        assert not os.path.exists(out + ext)


# ---- host --dedup-dist / --reps-per-cluster (the host path of rtc_tree_medoids and the candidate / representative lists) ----
@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOSTLIB):
        pytest.fail("librtclust_host.so missing: run __graft_entry__.build()")
    lib = C.CDLL(HOSTLIB)
    lib.rtch_dedup_reps.argtypes = [C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 5
    return lib


def _host_dedup(lib, n, edges, lens, dedup, k, threads=4):
    a = np.array(edges, dtype=EDGE) if edges else np.zeros(1, dtype=EDGE)
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    rep, cd, rp = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    co, ro = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    nc = lib.rtch_dedup_reps(n, P(a), len(edges), P(lens), dedup, k, threads, P(rep), P(cd), P(co), P(rp), P(ro))
    assert nc >= 0
    return rep.tolist(), [cd[co[i]:co[i + 1]].tolist() for i in range(nc)], [rp[ro[i]:ro[i + 1]].tolist() for i in range(nc)]


def _random_forest(seed, n, p_zero, equal_lens):
    """a random forest (some trees, some singletons) with zero-weight edges and repeated weights"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n)
    edges = []
    for i in range(1, n):
        if rng.random() < 0.12:
            continue  # a new tree starts here
        w = 0.0 if rng.random() < p_zero else float(rng.choice([0.001, 0.002, 0.003, 0.01, 0.02, 0.03 + 0.01 * rng.random()]))
        edges.append((int(ids[i]), int(ids[int(rng.integers(0, i))]), w))
    rng.shuffle(edges)
    lens = np.full(n, 5000, dtype=np.uint64) if equal_lens else rng.choice([5000, 6000, 7000], size=n).astype(np.uint64)
    return edges, lens


@pytest.mark.parametrize("seed", range(6))
def test_host_dedup_and_reps_match_restatement(host, seed):
    n = [12, 40, 90, 150, 260, 33][seed]
    edges, lens = _random_forest(seed, n, p_zero=[0.0, 0.3, 0.6, 0.2, 0.4, 1.0][seed], equal_lens=seed % 2 == 1)
    thr = 0.05
    forest = R.forest(edges, thr)
    for dedup in (0.0015, 0.005, 0.5, -1.0):  # 0.5: above the threshold, every forest edge; -1: the no-op
        for k in (0, 1, 2, 3, 1000):
            got = _host_dedup(host, n, forest, lens, dedup, k, threads=1 + seed % 4)
            rep, cl, cd, rp = R.dedup_and_reps(n, forest, [int(x) for x in lens], dedup, k)
            assert got[0] == rep, (dedup, k)
            assert got[1] == cd, (dedup, k)
            assert got[2] == rp, (dedup, k)


def test_host_medoid_ties_and_refusal(host):
    # a star of identical genomes: every total ties exactly except the centre's; a chain of zeros: all tie -> longest, then smallest id
    star = [(0, i, 0.0) for i in range(1, 6)]
    assert _host_dedup(host, 6, star, [5, 5, 9, 9, 5, 5], 0.01, 0)[0] == R.tree_medoids(6, star, 0.01, [5, 5, 9, 9, 5, 5])
    chain = [(i, i + 1, 0.0) for i in range(7)]
    assert _host_dedup(host, 8, chain, [3, 4, 4, 1, 1, 4, 2, 2], 0.01, 0)[0] == [1] * 8
    lib_edges = np.array([(0, 1, 0.0), (1, 2, 0.0), (2, 0, 0.0)], dtype=EDGE)
    out = np.zeros(3, np.int32)
    zero = np.zeros(4, np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert host.rtch_dedup_reps(3, P(lib_edges), 3, P(np.ones(3, np.uint64)), 0.01, 0, 1, P(out), P(zero), P(zero), P(zero),
                                P(zero)) == -1  # a cycle: not a forest


def test_clust_greedy_still_rejects_the_mst_flags():
    greedy = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-greedy")
    r = subprocess.run([greedy, "--dedup-dist", "0.01", "-o", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--dedup-dist" in r.stderr
