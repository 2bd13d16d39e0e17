"""clust-dbscan without a GPU: the closed form the GPU computes equals the reference's sequential walk on symmetric
neighbour graphs (tests/refdbscan.py restates both), the restated predicate on hand-made sketches, and the command line's
flag errors, which exit before any GPU is asked for."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-dbscan")


def _random_graph(rng, n, p):
    nb = [set() for _ in range(n)]
    for i in range(n):
        for j in range(i):
            if rng.random() < p:
                nb[i].add(j)
                nb[j].add(i)
    # the reference lists neighbours in no particular order: shuffle them
    out = []
    for s in nb:
        lst = list(s)
        rng.shuffle(lst)
        out.append(lst)
    return out


@pytest.mark.parametrize("seed", range(40))
def test_sequential_walk_equals_closed_form(seed):
    rng = random.Random(seed)
    n = rng.randint(1, 60)
    p = rng.choice([0.0, 0.02, 0.05, 0.1, 0.3, 0.8])
    nbrs = _random_graph(rng, n, p)
    for min_pts in (0, 1, 2, 3, 5, rng.randint(1, 12)):
        walk, n_core = R.sequential_walk(nbrs, min_pts)
        walk = [x if x >= 0 else -1 for x in walk]
        closed, core = R.closed_form(nbrs, min_pts)
        assert walk == closed, (seed, min_pts)
        assert n_core == sum(core)


def test_hand_made_neighbour_rules():
    # cores {1, 2, 3, 9} and {5, 6, 7, 10} at minPts 4 (two cliques); 4 touches 3 and 5 but is no core and goes to the first
    # cluster; 0 (one neighbour, 9) is labelled noise first and absorbed by cluster 0 later; 8 stays noise
    edges = [(1, 2), (1, 3), (1, 9), (2, 3), (2, 9), (3, 9), (5, 6), (5, 7), (5, 10), (6, 7), (6, 10), (7, 10), (3, 4), (4, 5), (0, 9)]
    nbrs = [[] for _ in range(11)]
    for a, b in edges:
        nbrs[a].append(b)
        nbrs[b].append(a)
    walk, n_core = R.sequential_walk(nbrs, 4)
    want = [0, 0, 0, 0, 0, 1, 1, 1, -1, 0, 1]
    assert [x if x >= 0 else -1 for x in walk] == want == R.closed_form(nbrs, 4)[0]
    assert n_core == 8


def test_predicate_restatement_on_sketches():
    t = R.jaccard_min(0.05, 19)
    a = np.arange(1, 101, dtype=np.uint32)
    # common c with a = b = 100: accepted iff c (1 + t) + 1e-12 >= 200 t
    cut = next(c for c in range(101) if not (c * (1.0 + t) + 1e-12 < t * 100.0 + t * 100.0))
    sk = [a, np.concatenate([a[:cut], np.arange(1000, 1000 + 100 - cut, dtype=np.uint32)]),
          np.concatenate([a[:cut - 1], np.arange(2000, 2000 + 101 - cut, dtype=np.uint32)])]
    nb = R.neighbour_lists(sk, 0.05, 19, use64=False)
    assert nb[0] == [1] and nb[1] == [0] and nb[2] == []
    # the u64 brute force: empty sketches are neighbours of each other
    e = np.zeros(0, dtype=np.uint64)
    nb64 = R.neighbour_lists([e, a.astype(np.uint64), e], 0.05, 19, use64=True)
    assert nb64 == [[2], [], [0]]
    # --max-posting: a hash every sketch holds is dropped, the sizes stay
    sk2 = [np.array([1, 5], dtype=np.uint32), np.array([1, 6], dtype=np.uint32), np.array([1, 7], dtype=np.uint32)]
    assert R.neighbour_lists(sk2, 10.0 / 19, 19, use64=False, max_posting=0) != [[], [], []]
    assert R.neighbour_lists(sk2, 10.0 / 19, 19, use64=False, max_posting=2) == [[], [], []]


def test_print_restatement_layout():
    genomes = [("a.fna", 100, "ga", "c a"), ("b.fna", 200, "gb", ""), ("c.fna", 300, "gc", "x")]
    txt = R.print_result([0, -1, 0], genomes, True, 0.05, 2)
    assert txt.startswith("# DBSCAN clustering parameters: eps=0.050000, minPts=2\n# Total clusters: 1\n"
                          "# Total noise points (outliers): 1\n#\nthe cluster 0 is: \n")
    assert "the cluster 1 is: \n\t    0\t     1\t         200nt\t" in txt


def _run(args):
    if not os.path.exists(BIN):
        pytest.fail("clust-dbscan missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("args,msg", [
    (["-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: clust-dbscan requires --fast option"),
    (["--fast", "--presketched", "d", "--append", "list.txt", "-o", "o.txt"], "ERROR: --append not supported for DBSCAN clustering"),
    (["--fast", "-l", "-i", "list.txt", "--knn", "500", "-o", "o.txt"], "--knn"),
    (["--fast", "-l", "-i", "list.txt", "--drlevel", "9", "-o", "o.txt"], "ERROR: invalid drlevel 9, should be in [0, 8]"),
    (["--fast", "-l", "-i", "list.txt", "--drlevel", "-1", "-o", "o.txt"], "ERROR: invalid drlevel -1, should be in [0, 8]"),
    (["--fast", "-l", "-i", "list.txt", "--dense", "-o", "o.txt"], "unknown option --dense"),
])
def test_flag_errors_exit_before_the_gpu(tmp_path, args, msg):
    r = _run(args)
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


def test_help_names_the_dbscan_options():
    r = _run(["-h"])
    assert r.returncode == 0 and "--eps" in r.stdout and "--minpts" in r.stdout and "--max-posting" in r.stdout
