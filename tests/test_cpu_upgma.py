"""clust-mst --upgma without a GPU: the two restatements of the definition agree on every matrix of the tests, tie-free matrices
give scipy's average linkage, heights never fall, the host's height and cut are the restatement's, the writers of the host
library are the restatement's, and the command line refuses what the flag does not go with before it asks for a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import refupgma as R
from tests import upgma_sets as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
Q1 = 1 << 20


@functools.lru_cache(maxsize=None)
def _sets():
    return {name: (S, w) for name, S, w in U.dev_sets()}


SET_NAMES = [name for name, _, _ in U.dev_sets()]


@pytest.mark.parametrize("name", SET_NAMES)
def test_naive_and_rowcache_agree_and_heights_never_fall(name):
    S, w = _sets()[name]
    m = len(S)
    want = R.naive(S, w)
    got, rescans = R.rowcache(S, w)
    assert got == want and len(want) == m - 1
    assert rescans >= m - 1  # row a at least, every step
    mean = R.means(want)
    assert all(x <= y for x, y in zip(mean, mean[1:]))
    h = [R.distance(s, na, nb) for _, _, na, nb, s in want]
    assert all(x <= y for x, y in zip(h, h[1:]))
    total = sum(w) if w else m
    assert want[-1][2] + want[-1][3] == total
    # the cut is a prefix: once the rule stops keeping, it never keeps again
    for threshold in (0.0, 0.004, 0.3, 1.0):
        flags = [R.keep(s, na, nb, threshold) for _, _, na, nb, s in want]
        assert flags == sorted(flags, reverse=True)


def test_the_named_hazards_are_what_they_say():
    S, _ = _sets()["tie_after_merge"]
    want = R.naive(S)
    assert want[0] == (2, 3, 1, 1, 10) and want[1] == (0, 2, 1, 2, 1000) and want[2] == (1, 5, 1, 1, 500)
    assert S[0][4] * 2 == S[0][2] + S[0][3]  # the mean that (0, 2) won with is (0, 4)'s own
    Sw, ww = _sets()["wide"]
    p = 3000 * 3000
    assert (Sw[0][1] * p) % (1 << 64) == (Sw[2][3] * p) % (1 << 64) and Sw[0][1] * p != Sw[2][3] * p
    first = R.naive(Sw, ww)[0]
    assert first[:2] == (2, 3) and first[4] == Sw[2][3]
    assert max(max(r) for r in Sw) * 15 < 1 << 62
    # all distances 1: the tie rule alone decides, (0, 1), (0, 2), ...; sums past 32 bits are weighted_ties'
    assert [(a, b, s) for a, b, _, _, s in R.naive(*_sets()["all_q1_300"])] == [(0, k, k * Q1) for k in range(1, 300)]
    Sb, wb = _sets()["weighted_ties_66"]
    assert sum(wb) < 1 << 22 and min(s for *_, s in R.naive(Sb, wb)) >= 1 << 32
    # the chain: the least pair is the two highest live indices, every step
    m = 70
    assert [(a, b) for a, b, *_ in R.naive(*_sets()["chain_70"])] == [(m - 2 - i, m - 1 - i) for i in range(m - 1)]


def _tie_free_seed(m):
    """the first seed whose matrix has no tied minimum at any step of the reference"""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    for seed in range(20):
        S = U.tie_free(m, seed)
        Z = linkage(squareform(np.array(S, dtype=np.float64) / Q1, checks=False), method="average")
        mean = R.means(R.naive(S))
        if len(set(mean)) == len(mean) and len(set(Z[:, 2].tolist())) == m - 1:
            return seed, S, Z
    raise AssertionError("no tie-free seed")


@pytest.mark.parametrize("m", [5, 17, 40])
def test_merge_order_heights_and_flat_clusters_equal_scipy(m):
    from scipy.cluster.hierarchy import fcluster
    seed, S, Z = _tie_free_seed(m)
    want = R.naive(S)
    mean = R.means(want)
    assert all(x < y for x, y in zip(mean, mean[1:]))  # no tied minimum at any step: strictly rising exact means
    # scipy names a new cluster m + step; here it keeps the name a
    ident = {g: g for g in range(m)}
    members = {g: [g] for g in range(m)}
    for step, (a, b, na, nb, s) in enumerate(want):
        assert {ident[a], ident[b]} == {int(Z[step, 0]), int(Z[step, 1])}, (m, seed, step)
        h = R.distance(s, na, nb)
        assert abs(h - Z[step, 2]) <= 1e-12 * Z[step, 2], (m, step, h, Z[step, 2])
        assert na + nb == int(Z[step, 3])
        ident[a] = m + step
        members[a] = members[a] + members.pop(b)
    hs = [R.distance(s, na, nb) for _, _, na, nb, s in want]
    for t in (0.5 * (hs[m // 4] + hs[m // 4 + 1]), 0.5 * (hs[m // 2] + hs[m // 2 + 1]), 0.5 * (hs[-2] + hs[-1])):
        flat = fcluster(Z, t=t, criterion="distance")
        ref = sorted(sorted(np.flatnonzero(flat == c).tolist()) for c in set(flat.tolist()))
        from tests import reflinkage as RL
        assert RL.clusters_of(range(m), R.cut(want, t)) == ref, (m, t)


def test_height_and_cut_are_the_librarys():
    from rabbittclust_amd import api, host
    cases = [(0, 1, 1), (1, 1, 1), (Q1, 1, 1), (Q1 - 1, 1, 1), (12345678901, 37, 1201), ((1 << 58) + 5, 3000, 3000), (3, 7, 11), ((1 << 62) - 1, 2047, 2048)]
    for s, na, nb in cases:
        assert np.float64(R.distance(s, na, nb)).view(np.uint64) == np.float64(api.upgma_distance(s, na, nb)).view(np.uint64), (s, na, nb)
    for threshold in (0.0, 0.03, 0.05, 0.9999995, 1.0, 0.0500004, 0.05000048, 2.5e-7, 4.76837158203125e-07):
        qcut = R.llround(threshold * 1048576.0)
        for na, nb in ((1, 1), (3, 5), (3000, 3000), (2047, 2048)):
            edge = qcut * na * nb
            for s in (edge - 1, edge, edge + 1):
                if s < 0:
                    continue
                want = s <= edge
                assert R.keep(s, na, nb, threshold) == want
                assert api.upgma_keep(s, na, nb, threshold) == want, (s, na, nb, threshold)
                assert host.upgma_keep(s, na, nb, threshold) == want, (s, na, nb, threshold)


def _leaf_depths(text):
    """the depth of every leaf below the root of a Newick text: the sum of the branch lengths on its path"""
    pos = 0

    def node():
        nonlocal pos
        if text[pos] != "(":
            while text[pos] not in ":;":
                pos += 1
            return [0.0]
        leaves = []
        while text[pos] in "(,":
            pos += 1
            sub = node()
            assert text[pos] == ":"
            end = pos + 1
            while text[end] in "0123456789.":
                end += 1
            ln = float(text[pos + 1:end])
            pos = end
            leaves += [d + ln for d in sub]
        assert text[pos] == ")"
        pos += 1
        return leaves
    out = node()
    assert text[pos] == ";"
    return out


def test_host_writers_are_the_restatements():
    """host.upgma_report / host.upgma_newick against refupgma.report over three run clusters of scattered genomes"""
    from rabbittclust_amd import api, host
    rng = np.random.default_rng(5)
    run = [[7, 2, 9, 4, 11], [0], [5, 1], [3, 10, 6, 8]]  # in the order <output> lists them: not by smallest member
    n = 12
    cluster_of = np.zeros(n, dtype=np.int32)
    for c, mem in enumerate(run):
        cluster_of[mem] = c
    merges, first = [], [0]
    for mem in sorted(sorted(c) for c in run):
        m = len(mem)
        if m >= 2:
            v = rng.integers(1, 9, size=(m, m)) * 9000
            S = [[int(v[min(i, j), max(i, j)]) if i != j else 0 for j in range(m)] for i in range(m)]
            merges += [(mem[a], mem[b], na, nb, s) for a, b, na, nb, s in R.naive(S)]
        first.append(len(merges))
    rec = R.as_records(merges, api.UMERGE_DT)
    label = lambda g: "genome_%d.fna" % g
    for threshold in (0.0, 0.02, 0.04, 1.0):
        want_cl, want_lk, want_nw = R.report(run, merges, first, threshold, n, label)
        text, refined, kept = host.upgma_report(cluster_of, rec, first, threshold)
        assert text == want_lk and refined == want_cl
        assert kept == n - len(want_cl)
    assert text.count("\n") == len(merges)
    rank = {c: q for q, c in enumerate(sorted(range(len(run)), key=lambda c: min(run[c])))}
    got_nw = "".join(host.upgma_newick([label(g) for g in range(n)], run[c], rec[first[rank[c]]:first[rank[c] + 1]]) + "\n" for c in range(len(run)))
    assert got_nw == want_nw
    lines = want_nw.split("\n")
    assert lines[1] == "genome_0.fna;" and lines[2].startswith("(genome_") and lines[2].count(":") == 2
    # ultrametric: every leaf of a tree is at the root's height, up to the six decimals of each printed branch
    for ln, c in zip(lines, run):
        d = _leaf_depths(ln)
        assert len(d) == len(c) and max(d) - min(d) <= 1e-6 * len(c)


def _tool(tool, args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, tool)] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


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
def test_refusals_come_before_the_gpu(tmp_path, flags, name):
    out = os.path.join(str(tmp_path), "r.out")
    base = [] if "--append" in flags or "--premsted" in flags else ["-l", "-i", "list.txt"]
    r = _tool("clust-mst", base + ["--fast", "-o", out, "--upgma"] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: --upgma does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []
    # beside an older flag whose refusal applies too, the older flag's message comes first
    r = _tool("clust-mst", base + ["--fast", "-o", out, "--linkage", "complete", "--upgma"] + flags, str(tmp_path))
    assert r.returncode == 1 and f"ERROR: --linkage does not go with {name}\n" in r.stderr and "--upgma" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _tool("clust-mst", ["-h"], str(tmp_path))
    assert h.returncode == 0 and "--upgma (average linkage" in h.stdout and ".upgma.newick" in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        r = _tool(tool, ["--fast", "-l", "-i", "list.txt", "-o", out, "--upgma"], str(tmp_path))
        assert r.returncode == 1 and "ERROR: unknown option --upgma\n" in r.stderr, tool
        assert "--upgma" not in _tool(tool, ["-h"], str(tmp_path)).stdout
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_upgma_calls():
    from rabbittclust_amd import _lib, api, host
    lib = _lib.load()
    for name in ("rtc_upgma_dev", "rtc_upgma_clusters", "rtc_upgma_counters", "rtc_upgma_last_path", "rtc_upgma_distance"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("upgma", "upgma_clusters", "upgma_counters", "upgma_last_path"):
        assert callable(getattr(api.Context, name))
    assert api.UMERGE_DT.itemsize == 24 and api.UPGMA_Q1 == Q1
    assert callable(api.upgma_distance) and callable(api.upgma_keep) and callable(host.upgma_report) and callable(host.upgma_newick)
