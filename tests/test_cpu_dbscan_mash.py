"""clust-dbscan --minhash without a GPU: the restated walk of MinHashDBSCAN against the closed form the GPU computes
(tests/refdbscan_mash.py), the decision table of rtc_dbscan_mash against the distance it stands for, and the command line's
flag errors."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import refdbscan_mash as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-dbscan")


def _random_sets(seed, n=200, s=32):
    """families around a shared core of hashes (mixed sizes and mutation rates), singletons, short and empty lists"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        kind = rng.random()
        if kind < 0.7:
            size = rng.choice([2, 3, 5, 8, 13])
            base = sorted(rng.sample(range(1 << 30), s))
            for _ in range(min(size, n - len(out))):
                keep = rng.choice([s, s - 1, s - 3, s // 2])
                v = set(rng.sample(base, keep))
                while len(v) < rng.choice([s, s, s - 2]):
                    v.add(rng.randrange(1 << 30))
                out.append(np.array(sorted(v), dtype=np.uint64))
        elif kind < 0.95:
            out.append(np.array(sorted(rng.sample(range(1 << 30), rng.choice([s, s, 1, 7]))), dtype=np.uint64))
        else:
            out.append(np.zeros(0, dtype=np.uint64))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequential_walk_equals_closed_form(seed):
    s, k = 32, 21
    dist = M.distance_matrix(M.count_matrix(_random_sets(seed, s=s), s), k)
    shapes = set()
    for eps in (0.0, 0.005, 0.02, 0.05, 0.2):
        nbrs = M.neighbour_lists(dist, eps)
        assert all((p in nbrs[q]) for p in range(len(nbrs)) for q in nbrs[p])  # symmetric
        for min_pts in (1, 2, 5):
            walk = [x if x >= 0 else -1 for x in M.sequential_walk(nbrs, min_pts)]
            closed, core = M.closed_form(nbrs, min_pts)
            assert walk == closed, (eps, min_pts)
            shapes.add((max(closed) + 1, closed.count(-1), sum(1 for v, c in zip(closed, core) if v >= 0 and not c) > 0))
    assert len(shapes) >= 6 and any(b for _, _, b in shapes)  # the cases differ, and some have border points


def test_the_two_restated_merges_agree():
    sets = _random_sets(5, n=60, s=32)
    for s in (1, 7, 32, 40):
        common, denom = M.count_matrix(sets, s)
        for p in range(len(sets)):
            for q in range(len(sets)):
                assert M.mash_counts(sets[p].tolist(), sets[q].tolist(), s) == (common[p, q], denom[p, q])


def test_core_rule_does_not_count_the_point():
    # a path 0 - 1 - 2: with minPts 2 only the middle point has two neighbours; the KSSD rule (|N| + 1) would make all three core
    nbrs = [[1], [0, 2], [1]]
    lab, core = M.closed_form(nbrs, 2)
    assert core == [False, True, False] and lab == [0, 0, 0]
    assert M.sequential_walk(nbrs, 2) == [0, 0, 0]
    assert M.closed_form(nbrs, 3) == ([-1, -1, -1], [False, False, False])
    for mp in (0, -3):  # every point a core point, isolated ones too
        assert M.closed_form([[1], [0], []], mp) == ([0, 0, 1], [True, True, True])
        assert M.sequential_walk([[1], [0], []], mp) == [0, 0, 1]


@pytest.mark.parametrize("eps", [0.0, 1e-9, 0.01, 0.05, 0.0731, 0.3, 0.999])
def test_decision_table_is_the_distance_predicate(eps):
    from rabbittclust_amd import _lib
    lib = _lib.load()
    s, k = 64, 21
    out = np.zeros(s + 1, dtype=np.uint32)
    assert lib.rtc_dbscan_mash_table(s, k, eps, out.ctypes.data_as(C.c_void_p)) == 0
    assert out.tolist() == M.decision_table(s, k, eps)
    for d in range(s + 1):
        for c in range(d + 1):
            dist = lib.rtc_mash_distance(c, d, s, k)
            assert dist == M.distance(c, d, k)  # the library's distance is the restated one, bit for bit
            assert (c >= out[d]) == (dist <= eps), (c, d)
    # eps on a distance and just below it
    e = M.distance(40, 64, k)
    for eps2, want in ((e, 40), (np.nextafter(e, 0), 41)):
        assert lib.rtc_dbscan_mash_table(s, k, float(eps2), out.ctypes.data_as(C.c_void_p)) == 0 and out[64] == want
    for bad in (-0.1, 1.0, float("nan")):
        assert lib.rtc_dbscan_mash_table(s, k, bad, out.ctypes.data_as(C.c_void_p)) == _lib.RTC_ERR_ARG


def _run(args):
    if not os.path.exists(BIN):
        pytest.fail("clust-dbscan missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("args,msg", [
    (["--minhash", "--fast", "-l", "-i", "list.txt", "-o", "o.txt"], "--fast"),
    (["--minhash", "--kdist", "-l", "-i", "list.txt", "-o", "o.txt"], "--kdist"),
    (["--minhash", "--hierarchy", "-l", "-i", "list.txt", "-o", "o.txt"], "--hierarchy"),
    (["--minhash", "--min-cluster-size", "3", "-l", "-i", "list.txt", "-o", "o.txt"], "--min-cluster-size"),
    (["--minhash", "--max-posting", "5", "-l", "-i", "list.txt", "-o", "o.txt"], "--max-posting"),
    (["--minhash", "-c", "1000", "-l", "-i", "list.txt", "-o", "o.txt"], "-c/--containment"),
    (["--minhash", "--eps", "1.0", "-l", "-i", "list.txt", "-o", "o.txt"], "0 <= eps < 1"),
    (["--minhash", "--eps", "-0.1", "-l", "-i", "list.txt", "-o", "o.txt"], "0 <= eps < 1"),
])
def test_minhash_flag_errors_exit_before_the_gpu(args, msg):
    r = _run(args)
    assert r.returncode == 1, r.stderr
    assert "ERROR: --minhash" in r.stderr and msg in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


def test_help_names_minhash():
    r = _run(["-h"])
    assert r.returncode == 0 and "--minhash" in r.stdout
