"""clust-mst --linkage complete without a GPU: the two restatements of the definition agree, the flat clusters equal scipy's complete
linkage where there are no ties, the cut gives cliques that cannot be joined, the conservative stop bound never stops early, and
the command line refuses what the flag does not go with before it asks for a GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import linkage_sets as S
from tests import reflinkage as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
D_GRID = (0.0, 0.003, 0.01, 0.05, 0.2, 0.5)
K_GRID = (17, 21, 31)


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_naive_and_rowbest_agree(case):
    for m in S.SIZES:
        keys = S.CASES[case](m)
        for kmin in ((0, 1), S.median_bound(keys)):
            want = R.naive(keys, kmin)
            got, rescans = R.rowbest(keys, kmin)
            assert got == want, (case, m, kmin)
            assert len(got) <= max(m - 1, 0)
            if case == "zeros":
                assert got == []
            if case == "star" and kmin == (0, 1) and m >= 2:
                assert [(a, b) for a, b, *_ in got] == [(0, j) for j in range(1, m)]
                assert rescans == (m - 1) * m // 2  # every live row, every step
            if case in ("all_equal", "equal_kappa") and kmin == (0, 1) and m >= 2:
                # ties everywhere: the smallest pair each step, and the smaller denominator is the one reported
                head = (0, 1, 2, 4) if case == "equal_kappa" else (0, 1, 1, 2)
                assert [(a, b, c, d) for a, b, c, d, _ in got] == [head] + [(0, j, 1, 2) for j in range(2, m)]
    # a bound inside the matrix ends the run mid-way
    keys = S.CASES["tie_free"](65)
    full, _ = R.rowbest(keys)
    part, _ = R.rowbest(keys, S.median_bound(keys))
    assert 0 < len(part) < len(full) == 64 and part == full[:len(part)]


def _partition(clusters):
    return sorted(tuple(sorted(c)) for c in clusters)


@pytest.mark.parametrize("m", [3, 64, 65, 257])
def test_flat_clusters_equal_scipy_on_tie_free_matrices(m):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    keys = S.tie_free(m)
    k = 21
    merges, _ = R.rowbest(keys)
    assert len(merges) == m - 1
    dist = [R.distance(c, d, k) for _, _, c, d, _ in merges]
    assert all(x < y for x, y in zip(dist, dist[1:]))  # no ties, monotone
    iu = np.triu_indices(m, 1)
    cond = np.array([R.distance(int(keys[i, j, 0]), int(keys[i, j, 1]), k) for i, j in zip(*iu)])
    Z = hier.linkage(cond, method="complete")
    for q in (0.1, 0.3, 0.5, 0.7, 0.9):
        at = int(q * (m - 1))
        t = dist[at] if at == m - 2 else 0.5 * (dist[at] + dist[at + 1])
        lab = hier.fcluster(Z, t, criterion="distance")
        want = {}
        for g, c in enumerate(lab):
            want.setdefault(int(c), []).append(g)
        got = R.clusters_of(range(m), R.cut(merges, t, k))
        assert _partition(got) == _partition(want.values()), (m, q)


def _check_cut(keys, members, threshold, k):
    merges, _ = R.rowbest(keys)
    local = R.clusters_of(range(len(members)), R.cut(merges, threshold, k))

    def d(i, j):
        return R.distance(int(keys[i, j, 0]), int(keys[i, j, 1]), k)
    for c in local:  # a clique of the dist <= d graph
        assert all(d(i, j) <= threshold for i, j in itertools.combinations(c, 2)), (threshold, k)
    for x, y in itertools.combinations(local, 2):  # and no two of them could be joined
        assert any(d(i, j) > threshold for i in x for j in y), (threshold, k, x, y)
    return local


def test_cut_clusters_are_cliques_that_cannot_be_joined():
    sketches, comp = S.component_set()
    groups = {}
    for g, lab in enumerate(comp):
        groups.setdefault(lab, []).append(g)
    counts = set()
    for members in groups.values():
        if len(members) < 2 or len(members) > 70:
            continue
        keys = R.keys_of([sketches[g] for g in members])
        for threshold in D_GRID:
            counts.add(len(_check_cut(keys, members, threshold, 21)))
    assert len(counts) > 3  # the grid cuts the components in different places
    for m in (5, 33):
        for threshold in D_GRID:
            _check_cut(S.random_ties(m), list(range(m)), threshold, 17)


def test_conservative_bound_never_stops_before_a_kept_merge():
    sketches, comp = S.component_set()
    members = [g for g, lab in enumerate(comp) if lab == comp[2]]  # the component of 65
    mats = [R.keys_of([sketches[g] for g in members]), S.random_ties(40), S.tie_free(40), S.near_2_31(20)]
    for keys in mats:
        full, _ = R.rowbest(keys)
        for threshold in D_GRID:
            for k in K_GRID:
                num, den = R.bound(threshold, k)
                assert 0 <= num <= den == 1 << 31
                kept = R.cut(full, threshold, k)
                bounded, _ = R.rowbest(keys, (num, den))
                assert R.cut(bounded, threshold, k) == kept, (threshold, k)
                # every key the cut keeps is at or above the bound
                for _, _, c, d, _ in kept:
                    assert c * den >= num * d
                # and the bound is not vacuous: it stops within 2^-19 of the true quotient
                for _, _, c, d, _ in bounded[len(kept):]:
                    j = 1.0 / (2.0 * np.exp(k * threshold) - 1.0)
                    assert c / d >= j * (1.0 - 2.0 ** -19)


def test_distance_is_the_librarys():
    from rabbittclust_amd import api
    for k in K_GRID:
        for c, d in [(0, 0), (0, 5), (5, 5), (1, 2), (2, 4), (999, 1000), (1, 1000), (123, 4567), (2 ** 30 - 1, 2 ** 31 - 1)]:
            assert np.float64(R.distance(c, d, k)).view(np.uint64) == np.float64(api.linkage_distance(c, d, k)).view(np.uint64), (c, d, k)
    for threshold in D_GRID:
        assert api.linkage_bound(threshold, 21) == R.bound(threshold, 21)


def _mst(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, "clust-mst")] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


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
    r = _mst(base + ["--fast", "-o", out, "--linkage", "complete"] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: --linkage does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_flag_spelling_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    r = _mst(["-l", "-i", "list.txt", "-o", out, "--linkage", "average"], str(tmp_path))
    assert r.returncode == 1 and "ERROR: --linkage must be complete\n" in r.stderr and "context" not in r.stderr
    r = _mst(["-l", "-i", "list.txt", "-o", out, "--linkage"], str(tmp_path))
    assert r.returncode == 1 and "requires a value" in r.stderr
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "--linkage complete" in h.stdout and "--linkage-matrix" not in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out, "--linkage", "complete"], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and "ERROR: unknown option --linkage\n" in r.stderr, tool
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_linkage_calls():
    from rabbittclust_amd import _lib
    lib = _lib.load()
    for name in ("rtc_linkage_dev", "rtc_linkage_complete", "rtc_linkage_counters", "rtc_linkage_distance"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
