"""clust-dbscan --knn without a GPU: the two closed forms rtc_dbscan_knn computes against the sequential steps
they replace -- the selection against the reference's min-heap on random arrival sequences, the walk against
refdbscan.sequential_walk on random directed lists -- the restated k-NN lists against the full neighbourhoods where they must
agree, the library's exports and the command line's flag errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refdbscan_knn as RK
from tests import sweep_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-dbscan")


def test_selection_closed_form_equals_the_heap():
    rng = np.random.default_rng(11)
    scores = [np.float32(x) for x in (0.125, 0.25, 0.3, 0.5, 0.75)]  # few distinct scores: ties dominate
    needed = truncated = short = 0
    for _ in range(12_000):
        n_cand = int(rng.integers(0, 14))
        k = int(rng.integers(1, 9))
        ids = rng.permutation(40)[:n_cand].tolist()  # arrival order is not id order
        n_scores = int(rng.integers(1, len(scores) + 1))
        arrivals = [(c, scores[int(rng.integers(0, n_scores))]) for c in ids]
        want = {c for c, _ in RK.heap_select(arrivals, k)}
        got, by_arrival = RK.closed_select(arrivals, k)
        assert got == want, (arrivals, k)
        short += n_cand < k
        truncated += n_cand > k
        needed += by_arrival
    assert short > 1000 and truncated > 1000 and needed > 1000  # every branch of the closed form was exercised


def test_walk_closed_form_equals_the_sequential_walk():
    rng = np.random.default_rng(12)
    borders = noise = 0
    for _ in range(2_500):
        n = int(rng.integers(1, 15))
        deg = int(rng.integers(0, 4))
        nbrs = []
        for v in range(n):
            others = [u for u in range(n) if u != v]
            m = min(len(others), int(rng.integers(0, deg + 1)))
            nbrs.append([others[i] for i in rng.permutation(len(others))[:m]])  # directed: u in N(v) says nothing about v in N(u)
        min_pts = int(rng.integers(1, 5))
        lab, n_core = R.sequential_walk(nbrs, min_pts)
        want = [x if x >= 0 else -1 for x in lab]
        got, core = RK.closed_walk(nbrs, min_pts)
        assert got == want, (nbrs, min_pts)
        assert sum(core) == n_core
        borders += any(g >= 0 and not c for g, c in zip(got, core))
        noise += -1 in got
    assert borders > 100 and noise > 100


@pytest.mark.parametrize("max_posting", [0, 5])
def test_knn_lists_with_a_large_k_are_the_full_neighbourhoods(max_posting):
    host = S.family_sets(2, False, n_empty=2)
    n = len(host)
    rows_checked = 0
    for eps in (0.02, 0.06):
        t = R.jaccard_min(eps, S.KMER)
        full = R.neighbour_lists(host, eps, S.KMER, False, max_posting)
        knn = RK.knn_lists(host, eps, S.KMER, n, max_posting)
        passers = RK.passers_in_arrival_order(host, eps, S.KMER, max_posting)
        for p in range(n):
            assert [c for c, _ in passers[p]] == full[p]  # the same scan, the same order
            if all(float(s) >= t for _, s in passers[p]):  # no passer fails the float test: the heap holds them all
                assert sorted(knn[p]) == sorted(full[p]), (eps, p)
                rows_checked += 1
            else:
                assert set(knn[p]) < set(full[p])
    assert rows_checked > n


def test_effective_k_and_labels_of_knn():
    host = S.family_sets(1, False)
    assert RK.effective_k(2, 5) == 4 and RK.effective_k(4, 5) == 4 and RK.effective_k(9, 5) == 9 and RK.effective_k(0, 5) == 0
    # k = n truncates nothing: where every row passes the float test the labels are the plain DBSCAN's
    eps = 0.04
    t = R.jaccard_min(eps, S.KMER)
    if all(float(s) >= t for row in RK.passers_in_arrival_order(host, eps, S.KMER) for _, s in row):
        assert np.array_equal(RK.labels_of_knn(host, eps, 5, S.KMER, len(host)), R.labels_of(host, eps, 5, S.KMER, False))
    assert not np.array_equal(RK.labels_of_knn(host, eps, 2, S.KMER, 1), R.labels_of(host, eps, 2, S.KMER, False))


def test_library_exports_the_knn_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "rabbittclust_amd", "librtclust_hip.so"))
    assert hasattr(lib, "rtc_dbscan_knn") and hasattr(lib, "rtc_dbscan_knn_counters")
    from rabbittclust_amd import api
    assert callable(api.Context.dbscan_knn) and callable(api.Context.dbscan_knn_counters)


def _run(args, cwd):
    if not os.path.exists(BIN):
        pytest.fail("clust-dbscan missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env, cwd=cwd)


@pytest.mark.parametrize("extra,flag", [
    (["--minhash"], "--minhash"),
    (["--fast", "--eps-sweep", "0.01,0.02"], "--eps-sweep"),
    (["--fast", "--kdist"], "--kdist"),
    (["--fast", "--hierarchy"], "--hierarchy"),
    (["--fast", "--min-cluster-size", "3"], "--min-cluster-size"),
    (["--fast", "--db", "model.db", "--build"], "--db"),
    (["--fast", "--db", "model.db", "--assign"], "--db"),
])
def test_knn_excludes_the_flows_of_the_symmetric_relation(tmp_path, extra, flag):
    lst = tmp_path / "list.txt"
    lst.write_text("")
    r = _run(extra + ["-l", "-i", str(lst), "--knn", "3", "-o", "o.txt"], str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert "ERROR: --knn does not go with " + flag + "\n" in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


def test_knn_run_on_a_missing_input_ends_before_the_gpu(tmp_path):
    r = _run(["--fast", "-l", "-i", "nowhere.txt", "--knn", "2", "--minpts", "5", "-o", "o.txt"], str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert "ERROR: --knn: cannot open the input nowhere.txt\n" in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr
    # --knn 0 is the run without the flag: its error path is the one it always was
    r0 = _run(["--fast", "-l", "-i", "nowhere.txt", "--knn", "0", "-o", "o.txt"], str(tmp_path))
    assert r0.returncode == 1 and "--knn" not in r0.stderr


def test_help_describes_the_flag():
    r = _run(["-h"], ROOT)
    assert r.returncode == 0 and "--knn K" in r.stdout and "not in this build" not in r.stdout
