"""clust-leiden --minhash without a GPU: the strict decision table of rtc_graph_build_mash against a linear scan of the
restated distance (tests/refgraph_mash.py), the restated counts against the definition on sets, the host's weight, and the
command line's flag errors.  Everything is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import graph_mash_sets as S
from tests import refdbscan_mash as M
from tests import refgraph_mash as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-leiden")
K = 21


def _table(lib, s, threshold):
    out = np.zeros(s + 1, dtype=np.uint32)
    assert lib.rtc_graph_mash_table(s, K, float(threshold), out.ctypes.data_as(C.c_void_p)) == 0
    return out.tolist()


@pytest.mark.parametrize("s", [16, 257])
def test_strict_table_is_a_linear_scan_of_the_restatement(s):
    from rabbittclust_amd import _lib
    lib = _lib.load()
    on = M.distance(s // 3, s, K)  # a distance that occurs: threshold == it leaves that count out, the next double takes it in
    assert 0.0 < on < 1.0
    for threshold in (0.05, on, float(np.nextafter(on, 1.0)), 1.0):
        got = _table(lib, s, threshold)
        assert got == G.strict_table(s, K, threshold), threshold
        assert got[0] == 1 and all(1 <= got[d] <= d + 1 for d in range(s + 1))
    assert _table(lib, s, on)[s] == s // 3 + 1 and _table(lib, s, float(np.nextafter(on, 1.0)))[s] == s // 3
    assert _table(lib, s, on)[s] == M.decision_table(s, K, on)[s] + 1  # the DBSCAN table takes the distance itself in
    assert _table(lib, s, 1.0)[1:] == [1] * s  # every shared hash among the first s passes: the least distance below 1 is far from it
    for c in range(s + 1):  # the weight is one minus the restated distance, bit for bit
        assert lib.rtc_graph_weight_mash(c, s, s, K) == G.weight(c, s, K)
    assert lib.rtc_graph_weight_mash(0, 0, s, K) == 0.0
    out = np.zeros(s + 1, dtype=np.uint32)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        assert lib.rtc_graph_mash_table(s, K, bad, out.ctypes.data_as(C.c_void_p)) == _lib.RTC_ERR_ARG
    assert lib.rtc_graph_mash_table(0, K, 0.05, out.ctypes.data_as(C.c_void_p)) == _lib.RTC_ERR_ARG
    assert lib.rtc_graph_mash_table(s, 0, 0.05, out.ctypes.data_as(C.c_void_p)) == _lib.RTC_ERR_ARG


def test_restated_counts_equal_the_definition_on_sets():
    lists, _, counts, _ = S.case(256)
    assert len(counts) == 191 * 190 // 2
    for (u, v), got in list(counts.items())[::23]:
        assert got == M.mash_counts_sets(lists[u], lists[v], 256), (u, v)
    for s in (1, 7, 100):
        for u, v in ((0, 1), (5, 77), (100, 192), (3, 4)):
            if len(lists[u]) and len(lists[v]):
                assert M.mash_counts(lists[u].tolist(), lists[v].tolist(), s) == M.mash_counts_sets(lists[u], lists[v], s)


def test_rank_ties_go_to_the_lower_v_by_cross_multiplication():
    counts = {(0, 1): (1, 6), (0, 2): (2, 4), (0, 3): (1, 2), (0, 4): (3, 4), (1, 2): (5, 10)}
    assert G.edges(counts, 0.05, K) == [(0, 2, 2, 4), (0, 3, 1, 2), (0, 4, 3, 4), (1, 2, 5, 10)]  # 1/6 fails the threshold
    assert G.edges(counts, 0.05, K, 1) == [(0, 4, 3, 4), (1, 2, 5, 10)]
    assert G.edges(counts, 0.05, K, 2) == [(0, 2, 2, 4), (0, 4, 3, 4), (1, 2, 5, 10)]  # 2/4 == 1/2: the lower v stays


def _run(args):
    if not os.path.exists(BIN):
        pytest.fail("clust-leiden missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("args,msg", [
    (["--minhash", "--fast", "--louvain", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with --fast"),
    (["--minhash", "--louvain", "-c", "1000", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with -c/--containment"),
    (["--minhash", "--louvain", "--containment", "1000", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with -c/--containment"),
    (["--minhash", "--leiden", "--drlevel", "3", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with --drlevel"),
    (["--minhash", "--louvain", "--db", "m.db", "--build", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with --db"),
    (["--minhash", "--db", "m.db", "--assign", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash does not go with --db"),
    (["--minhash", "--louvain", "-d", "0", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash needs 0 < -d/--threshold <= 1"),
    (["--minhash", "--louvain", "-d", "-0.1", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash needs 0 < -d/--threshold <= 1"),
    (["--minhash", "--louvain", "-d", "1.01", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --minhash needs 0 < -d/--threshold <= 1"),
    (["--minhash", "--leiden", "-d", "nan", "--presketched", "d", "-o", "o.txt"], "ERROR: --minhash needs 0 < -d/--threshold <= 1"),
])
def test_minhash_refusals_exit_before_the_gpu(args, msg, tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run([out if a == "o.txt" else a for a in args])
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr
    assert "context" not in r.stderr and "Building similarity graph" not in r.stderr
    assert not os.path.exists(out)


def test_help_names_minhash():
    r = _run(["-h"])
    assert r.returncode == 0 and "--minhash" in r.stdout and "--fast" in r.stdout


def test_no_sketch_kind_keeps_its_error(tmp_path):
    r = _run(["--louvain", "-l", "-i", "list.txt", "-o", str(tmp_path / "o.txt")])
    assert r.returncode == 1 and "ERROR: clust-leiden requires --fast option\n" in r.stderr
    # -s and -c mean something beside --minhash alone
    for flag in (["-s", "500"], ["--sketch-size", "500"], ["-c", "1000"]):
        r = _run(["--fast", "--louvain", "-l", "-i", "list.txt", "-o", str(tmp_path / "o.txt")] + flag)
        assert r.returncode == 1 and "ERROR: unknown option " + flag[0] + "\n" in r.stderr
