"""clust-greedy --order degree without a GPU: the restatement's own invariants on the test sets (tests/refgreedy_degree.py on
tests/greedy_degree_sets.py), the two ways it forms the neighbour relation against each other, the command line's refusals, the
help text and the library's symbols."""
import os
import subprocess

import numpy as np
import pytest

from tests import greedy_degree_sets as S
from tests import refdbscan_mash as M
from tests import refgreedy_degree as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
K = S.KMER


def _check_invariants(nbrs, counts, result):
    rep, deg, common, denom, ncl = result
    n = len(nbrs)
    sets = [set(int(u) for u in x) for x in nbrs]
    reps = {v for v in range(n) if rep[v] == v}
    assert ncl == len(reps) and deg == [len(x) for x in nbrs]
    rank = {v: i for i, v in enumerate(sorted(range(n), key=lambda v: (-deg[v], v)))}
    for v in range(n):
        if v in reps:
            assert not (sets[v] & reps), v            # independent
            assert (common[v], denom[v]) == (0, 0)
            continue
        assert sets[v] & reps, v                      # maximal
        r = rep[v]
        assert r in reps and r in sets[v], v          # a member is next to its representative
        assert any(rank[q] < rank[v] for q in sets[v] & reps), v  # ... and an earlier one made it a member
        assert (common[v], denom[v]) == tuple(int(x) for x in counts(v, r))
        for q in sets[v] & reps:                      # no representative next to v beats the chosen one
            c, d = (int(x) for x in counts(v, q))
            assert c * denom[v] <= common[v] * d, (v, r, q)
            if c * denom[v] == common[v] * d:
                assert rank[r] <= rank[q], (v, r, q)
    return reps


@pytest.mark.parametrize("use64", [False, True])
@pytest.mark.parametrize("n_empty", [0, 3])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_invariants_on_the_family_sets(seed, use64, n_empty):
    sk = S.families(seed, use64, n_empty)
    nbrs = G.neighbours_kssd(sk, S.FAMILY_THRESHOLD, K, use64)
    # the array form of the relation, which the large sets use, is the posting walk's
    dense = G.neighbours_kssd_dense(G.common_matrix(sk), [len(s) for s in sk], S.FAMILY_THRESHOLD, K)
    assert [list(map(int, x)) for x in dense] == nbrs
    res = G.kssd(sk, S.FAMILY_THRESHOLD, K, use64, nbrs=nbrs)
    reps = _check_invariants(nbrs, G.kssd_counts(sk, use64), res)
    empty = [v for v, s in enumerate(sk) if len(s) == 0]
    assert len(empty) == n_empty and all(v in reps and not nbrs[v] for v in empty)  # isolated: clusters of their own
    assert 1 < res[4] < len(sk) and any(res[1][v] > 1 and v not in reps for v in range(len(sk)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_invariants_on_the_minhash_families(seed):
    s = 128
    sk = S.minhash_families(seed, s)
    common, denom = M.count_matrix(sk, s)
    res = G.minhash(sk, s, 0.05, K, counts=(common, denom))
    nbrs = M.neighbour_lists(M.distance_matrix((common, denom), K), 0.05)
    _check_invariants(nbrs, lambda v, r: (common[v, r], denom[v, r]), res)
    assert 1 < res[4] < len(sk) and (denom < s).any()


def test_path_takes_every_other_genome():
    n = 2000
    sk = S.path(n)
    nbrs = [[q for q in (p - 1, p + 1) if 0 <= q < n] for p in range(n)]
    assert G.neighbours_kssd(sk[:40], 0.05, K, False) == [[q for q in (p - 1, p + 1) if 0 <= q < 40] for p in range(40)]
    rep, deg, common, denom, ncl = G.walk(nbrs, G.kssd_counts(sk, False))
    assert ncl == n // 2 and [v for v in range(n) if rep[v] == v] == list(range(1, n, 2))
    assert rep[0] == 1 and rep[2] == 1 and rep[4] == 3 and (common[2], denom[2]) == (8, 24)  # of two equal j the earlier representative


def test_small_graphs_isolate_one_rule_each():
    for make in (S.star_and_clique, S.two_hubs, S.tie_in_j, S.both_sides):
        sk, edges = make()
        nbrs = G.neighbours_kssd(sk, S.GRAPH_THRESHOLD, K, False)
        assert nbrs == S.edges_to_lists(len(sk), edges), make.__name__
        _check_invariants(nbrs, G.kssd_counts(sk, False), G.kssd(sk, S.GRAPH_THRESHOLD, K, False, nbrs=nbrs))
    rep = G.kssd(S.star_and_clique()[0], S.GRAPH_THRESHOLD, K, False)[0]
    assert rep == [3, 3, 3, 3, 3, 3, 6, 6, 6, 6, 6]
    rep, deg, _, _, ncl = G.kssd(S.two_hubs()[0], S.GRAPH_THRESHOLD, K, False)
    assert deg[2] == deg[5] == 4 and rep == [2, 2, 2, 2, 4, 2, 6, 7] and ncl == 4
    rep, deg, common, denom, _ = G.kssd(S.tie_in_j()[0], S.GRAPH_THRESHOLD, K, False)
    assert (deg[0], deg[1]) == (3, 4) and rep[2] == 1 and (common[2], denom[2]) == (2, 12)
    counts = G.kssd_counts(S.tie_in_j()[0], False)
    assert counts(2, 0) == (4, 24)
    rep, deg, common, denom, _ = G.kssd(S.both_sides()[0], S.GRAPH_THRESHOLD, K, False)
    assert deg[0] == deg[1] == 3 and rep[2] == 1 and (common[2], denom[2]) == (6, 12)


def test_long_row_set_has_the_row():
    sk, edges = S.long_row(leaves=40)  # the construction at a size the posting walk takes in a moment
    nbrs = G.neighbours_kssd(sk, S.LONG_ROW_THRESHOLD, K, False)
    assert nbrs == S.edges_to_lists(len(sk), edges)
    rep, deg, common, denom, ncl = G.kssd(sk, S.LONG_ROW_THRESHOLD, K, False, nbrs=nbrs)
    assert deg[0] == deg[1] == 41 and rep[1] == 0 and ncl == 41
    assert sum(1 for q in nbrs[1] if rep[q] == q) == 41  # hub 1: hub 0 and its own 40 leaves are its candidates


def _tool(tool, args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, tool)] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("flags,name", [
    (["-c", "1000"], "-c/--containment"),
    (["--inverted-index=false"], "--inverted-index=false"),
    (["--presketched", "nowhere", "--append", "list.txt"], "--append"),
    (["--db", "x.db", "--build"], "--db"),
    (["--save-rep"], "--save-rep"),
])
@pytest.mark.parametrize("fast", [True, False])
def test_refusals_come_before_the_gpu(tmp_path, flags, name, fast):
    out = os.path.join(str(tmp_path), "r.out")
    base = [] if "--append" in flags else ["-l", "-i", "list.txt"]
    r = _tool("clust-greedy", base + (["--fast"] if fast else []) + ["-o", out, "--order", "degree"] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: --order does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_order_takes_degree_only_and_minhash_thresholds_below_one(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    for value in ("size", "length", "Degree"):
        r = _tool("clust-greedy", ["--fast", "-l", "-i", "list.txt", "-o", out, "--order", value], str(tmp_path))
        assert r.returncode == 1 and "ERROR: --order must be degree\n" in r.stderr, value
    r = _tool("clust-greedy", ["--fast", "-l", "-i", "list.txt", "-o", out, "--order"], str(tmp_path))
    assert r.returncode == 1 and "ERROR: option --order requires a value\n" in r.stderr
    for d in ("1", "1.5", "-0.01"):
        r = _tool("clust-greedy", ["-l", "-i", "list.txt", "-o", out, "--order", "degree", "-d", d], str(tmp_path))
        assert r.returncode == 1 and "ERROR: --order degree on MinHash sketches needs 0 <= -d/--threshold < 1" in r.stderr, d
        assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _tool("clust-greedy", ["-h"], str(tmp_path))
    assert h.returncode == 0 and "--order degree (clusters that do not depend on the order of the genomes" in h.stdout
    assert ".order.tsv" in h.stdout and "not with -c, --inverted-index=false, --append" in h.stdout
    for tool in ("clust-mst", "clust-dbscan", "clust-leiden"):
        r = _tool(tool, ["--fast", "-l", "-i", "list.txt", "-o", out, "--order", "degree"], str(tmp_path))
        assert r.returncode == 1 and "ERROR: unknown option --order\n" in r.stderr, tool
        assert "--order" not in _tool(tool, ["-h"], str(tmp_path)).stdout
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_greedy_degree_calls():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_greedy_degree", "rtc_greedy_degree_counters", "rtc_greedy_degree_last_path"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("greedy_degree", "greedy_degree_counters", "greedy_degree_last_path"):
        assert callable(getattr(api.Context, name))
    assert api.DEGREE_PLACE_DT.itemsize == 16 and api.DEGREE_PLACE_DT.names == ("rep", "degree", "common", "denom")
    assert (api.DEGREE_PATH_WAVE, api.DEGREE_PATH_WORKGROUP, api.DEGREE_PATH_TAIL) == (1, 2, 4)


def test_the_two_files_as_text():
    rep = [1, 1, 1, 3]
    res = (rep, [1, 2, 1, 0], [5, 0, 10, 0], [10, 0, 10, 0], 2)
    assert G.clusters(rep) == [[1, 0, 2], [3]]
    names = ["a", "b", "c", "d"]
    tsv = G.order_tsv(res, names, 21, False)
    assert tsv.split("\n")[:3] == ["name\tdegree\trole\trepresentative\tdistance", "b\t2\trep\tb\t0.000000", "a\t1\tmember\tb\t%.6f" % G.kssd_distance(5, 10, 21)]
    assert tsv.split("\n")[3] == "c\t1\tmember\tb\t0.000000" and G.order_tsv(res, names, 21, True).split("\n")[2].endswith("%.6f" % M.distance(5, 10, 21))
