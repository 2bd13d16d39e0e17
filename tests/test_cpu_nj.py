"""clust-mst --nj-tree / --nj-all without a GPU: the restatement (tests/refnj.py) against the trees that generate its matrices, the
Newick writer, the refusals of the command line and the library's exports."""
import os
import subprocess

import numpy as np
import pytest

from tests import nj_sets as N
from tests import refnj as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


@pytest.mark.parametrize("m", [3, 4, 5, 8, 17, 40, 65, 130])
def test_restatement_returns_the_generating_tree(m):
    D, want = N.additive(m)
    rec = R.nj(D)
    assert len(rec) == m - 2
    assert R.splits(rec, m) == want
    assert all(c == R.NONE and lc == 0.0 for _, _, c, _, _, lc in rec[:-1]) and rec[-1][2] != R.NONE
    # the definition is symmetric in the matrix: its transpose (the same matrix) and a copy with another diagonal give the same bits
    other = D.copy()
    np.fill_diagonal(other, 7.0)
    assert R.bits(R.nj(other)) == R.bits(rec)


def test_restatement_small_cases_and_splits():
    assert R.nj(np.zeros((0, 0))) == [] and R.nj(np.zeros((1, 1))) == []
    assert R.nj(np.array([[0.0, 3.0], [3.0, 0.0]])) == [(0, 1, R.NONE, 1.5, 1.5, 0.0)]
    D, want = N.additive(2)
    assert R.splits(R.nj(D), 2) == want == [(2, D[0, 1])]
    # a quartet ((0:1,1:2):3,(2:4,3:5)): the first join is (0, 1), ties and all
    D = np.array([[0, 3, 8, 9], [3, 0, 9, 10], [8, 9, 0, 9], [9, 10, 9, 0]], dtype=np.float64)
    assert R.nj(D) == [(0, 1, R.NONE, 1.0, 2.0, 0.0), (0, 2, 3, 3.0, 4.0, 5.0)]
    # not additive: a negative length comes out as it is
    D = np.array([[0, 1, 5, 5], [1, 0, 1, 5], [5, 1, 0, 1], [5, 5, 1, 0]], dtype=np.float64)
    assert min(min(la, lb, lc) for _, _, _, la, lb, lc in R.nj(D)) < 0


def _records(rows):
    from rabbittclust_amd import api
    out = np.zeros(len(rows), dtype=api.NJOIN_DT)
    for e, (a, b, c, la, lb, lc) in enumerate(rows):
        out[e] = (a, b, c, 0, la, lb, lc)
    return out


def test_newick_writer():
    from rabbittclust_amd import host
    labels = [f"g{v}" for v in range(10)]
    assert host.nj_newick(labels, [4], _records([])) == "g4;"
    assert host.nj_newick(labels, [1, 6], _records([(1, 6, R.NONE, 0.5, 0.25, 0.0)])) == "(g1:0.500000,g6:0.250000);"
    assert host.nj_newick(labels, [0, 1, 2], _records([(0, 1, 2, 1.0, 2.0, 3.0)])) == "(g0:1.000000,g1:2.000000,g2:3.000000);"
    rec = _records([(3, 7, R.NONE, 1.5, -0.25, 0.0), (2, 9, R.NONE, 1.0, 2.0, 0.0), (2, 3, 5, 0.5, 0.75, 4.0)])
    assert host.nj_newick(labels, [9, 2, 3, 5, 7], rec) == \
        "((g2:1.000000,g9:2.000000):0.500000,(g3:1.500000,g7:-0.250000):0.750000,g5:4.000000);"


def test_newick_writer_does_not_recurse():
    from rabbittclust_amd import host
    n = 100_000
    labels = [f"L{v}" for v in range(n)]
    rows = [(0, k, R.NONE, 1.0, 2.0, 0.0) for k in range(1, n - 2)] + [(0, n - 2, n - 1, 1.0, 2.0, 3.0)]
    want = "(" * (n - 2) + "L0" + "".join(f":1.000000,L{k}:2.000000)" for k in range(1, n - 2)) + f":1.000000,L{n - 2}:2.000000,L{n - 1}:3.000000);"
    assert host.nj_newick(labels, range(n), _records(rows)) == want


def _mst(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, "clust-mst")] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("nj_flag", ["--nj-tree", "--nj-all"])
@pytest.mark.parametrize("flags,name", [
    (["-c", "1000"], "-c/--containment"),
    (["--inverted-index=false"], "--inverted-index=false"),
    (["--presketched", "nowhere", "--append", "list.txt"], "--append"),
    (["--premsted", "nowhere"], "--premsted"),
    (["--db", "x.db", "--build"], "--db"),
    (["--dense"], "--dense"),
    (["--auto-threshold"], "--auto-threshold"),
    (["--stability"], "--stability"),
])
def test_refusals_come_before_the_gpu(tmp_path, flags, name, nj_flag):
    out = os.path.join(str(tmp_path), "r.out")
    base = [] if "--append" in flags or "--premsted" in flags else ["-l", "-i", "list.txt"]
    r = _mst(base + ["--fast", "-o", out, nj_flag] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: {nj_flag} does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "--nj-tree" in h.stdout and "--nj-all" in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        for flag in ("--nj-tree", "--nj-all"):
            r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out, flag], cwd=str(tmp_path),
                               capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode == 1 and f"ERROR: unknown option {flag}\n" in r.stderr, tool
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_nj_calls():
    from rabbittclust_amd import _lib
    lib = _lib.load()
    for name in ("rtc_nj_dev", "rtc_nj_clusters", "rtc_nj_counters", "rtc_nj_last_path"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
