"""clust-mst --quality without a GPU: the restatement of rtc_silhouette equals the textbook silhouette over the full distance matrix
in fractions, rtc_silhouette_value is the Python expression bit for bit, the sets of the GPU tests hold their cases, the report
writer's columns follow their rules, and the command line refuses what the flag does not go with before it asks for a GPU."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import quality_sets as S
from tests import refquality as R
from tests.community_sets import home_slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
ONE, NONE = R.ONE, R.NONE


def _check_against_dense(n, edges, labels):
    rec = R.silhouette(n, edges, labels)
    want = R.dense(n, edges, labels)
    seen = set()
    for x in range(n):
        r = rec[x]
        if want[x] is None:
            assert [int(r[f]) for f in R.FIELDS] == [0, 0, 0, 0, NONE, 0, 0, NONE], x
            seen.add("noise")
            continue
        a, b, b_cluster, far, near = want[x]
        if a is None:
            assert int(r["a_den"]) == 0 and int(r["a_num"]) == 0 and int(r["far_q"]) == 0, x
            seen.add("singleton")
        else:
            assert Fraction(int(r["a_num"]), int(r["a_den"])) == a and int(r["a_den"]) == int((labels == labels[x]).sum()) - 1, x
        if b is None:
            assert int(r["b_den"]) == 0 and int(r["b_num"]) == 0 and int(r["b_cluster"]) == NONE, x
            seen.add("alone")
        else:
            assert Fraction(int(r["b_num"]), int(r["b_den"])) == b, x
            if b < ONE:
                assert int(r["b_cluster"]) == b_cluster and int(r["b_den"]) == int((labels == b_cluster).sum()), x
                seen.add("b")
            else:
                assert (int(r["b_num"]), int(r["b_den"]), int(r["b_cluster"])) == (ONE, 1, NONE), x
                seen.add("b at one")
        assert int(r["far_q"]) == far and int(r["near_q"]) == near, x
        if near < ONE:
            assert int(r["near_cluster"]) in set(labels[labels >= 0].tolist()) - {int(labels[x])}
        # the value through fractions: (b - a) / max(a, b), 0 for a singleton, alone or at 0 / 0
        v = R.value(r)
        if a is None or b is None or max(a, b) == 0:
            assert v == 0.0
        else:
            assert abs(v - float((b - a) / max(a, b))) < 1e-12, x
    return seen


def test_restatement_equals_the_dense_silhouette():
    seen = set()
    for seed in range(12):
        n = (2, 3, 7, 12, 20, 33, 40, 40, 25, 31, 17, 38)[seed]
        seen |= _check_against_dense(*S.random_graph(seed, n, p_edge=(0.1, 0.3, 0.6, 1.0)[seed % 4], n_clusters=1 + seed % 5))
    seen |= _check_against_dense(*S.random_graph(100, 36, p_edge=0.5, n_clusters=4, lonely_cluster=True))
    seen |= _check_against_dense(*S.one_cluster())
    seen |= _check_against_dense(*S.singletons())
    seen |= _check_against_dense(*S.arithmetic())
    n, edges, labels = S.random_graph(101, 30, p_edge=0.4, n_clusters=3, p_noise=0.0)
    seen |= _check_against_dense(n, edges, labels)
    assert seen == {"noise", "singleton", "alone", "b", "b at one"}
    # a cluster none of whose members has a listed neighbour: every member sees a = 1 and b = 1
    n, edges, labels = S.random_graph(100, 36, p_edge=0.5, n_clusters=4, lonely_cluster=True)
    rec = R.silhouette(n, edges, labels)
    lonely = [x for x in range(n) if labels[x] >= 0 and not any(x in (u, v) for u, v, _ in edges)]
    assert len(lonely) >= 3 and len(set(labels[lonely].tolist())) == 1
    for x in lonely:
        assert (int(rec[x]["b_num"]), int(rec[x]["b_den"]), int(rec[x]["near_q"]), int(rec[x]["far_q"])) == (ONE, 1, ONE, ONE)


def test_argument_errors_of_the_restatement():
    lab = np.zeros(4, dtype=np.int64)
    for edges in ([(0, 0, 1)], [(0, 4, 1)], [(4, 0, 1)], [(0, 1, ONE + 1)], [(0, 1, 5), (1, 0, 6)], [(0, 1, 5), (2, 3, 1), (0, 1, 5)]):
        with pytest.raises(ValueError):
            R.silhouette(4, edges, lab)
    with pytest.raises(ValueError):
        R.silhouette(4, [], np.array([0, 1, 4, -1]))
    assert len(R.silhouette(0, [], np.zeros(0, dtype=np.int64))) == 0


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_value_is_the_librarys_bit_for_bit():
    from rabbittclust_amd import api
    assert api.SIL_DT == R.SIL_DT and api.SIL_DT.itemsize == 40 and api.SIL_ONE == ONE and api.SIL_NONE == NONE
    rng = np.random.default_rng(5)
    rec = np.zeros(400, dtype=R.SIL_DT)
    rec["a_den"] = rng.integers(1, 1 << 31, size=400)
    rec["b_den"] = rng.integers(1, 1 << 31, size=400)
    rec["a_num"] = (rng.random(400) * rec["a_den"] * ONE).astype(np.uint64)
    rec["b_num"] = (rng.random(400) * rec["b_den"] * ONE).astype(np.uint64)
    rec[0] = (5, 7, 0, 3, 1, 0, 0, 1)      # a_den == 0
    rec[1] = (5, 0, 2, 0, NONE, 0, 0, 1)   # b_den == 0
    rec[2] = (0, 0, 3, 4, 1, 0, 0, 1)      # a == b == 0
    rec[3] = (0, ONE, 3, 1, NONE, 0, 0, 1)  # a == 0: 1
    rec[4] = (3 * ONE, 0, 3, 4, 1, 0, 0, 1)  # b == 0: -1
    rec[5] = (ONE, ONE, 1, 1, 2, 0, 0, 1)   # equal: 0
    rec[6] = (((1 << 31) - 2) * ONE, ONE, (1 << 31) - 2, 1, NONE, ONE, ONE, NONE)  # the largest counts
    vec = api.silhouette_value(rec)
    for i in range(len(rec)):
        want = R.value(rec[i])
        assert _bits(api.silhouette_value_one(rec[i])) == _bits(want), i
        assert _bits(vec[i]) == _bits(want), i
    assert [R.value(rec[i]) for i in range(6)] == [0.0, 0.0, 0.0, 1.0, -1.0, 0.0]
    assert len({R.value(rec[i]) for i in range(7, 400)}) > 300


def test_path_boundaries_are_the_headers():
    from rabbittclust_amd import api
    text = open(os.path.join(ROOT, "rabbittclust_amd", "csrc", "rtc_quality.h")).read()
    got = {k: int(v) for k, v in re.findall(r"(SIL_[A-Z0-9_]+) = (\d+)", text)}
    for name, mine in (("SIL_WAVE_ROW", S.WAVE_ROW), ("SIL_WAVE_SLOTS", S.WAVE_SLOTS), ("SIL_BLOCK_ROW", S.BLOCK_ROW), ("SIL_BLOCK_SLOTS", S.BLOCK_SLOTS),
                       ("SIL_GLOBAL_LOG2_MIN", S.GLOBAL_LOG2_MIN)):
        assert got[name] == mine == getattr(api, name), name
    assert (api.SIL_PATH_WAVE, api.SIL_PATH_WORKGROUP, api.SIL_PATH_GLOBAL) == (S.WAVE, S.WORKGROUP, S.GLOBAL)
    assert (got["SIL_WAVE_WGS_PER_CU"], got["SIL_BLOCK_WGS_PER_CU"], got["SIL_GLOBAL_WGS_PER_CU"]) == (S.WGS_PER_CU[S.WAVE], S.WGS_PER_CU[S.WORKGROUP],
                                                                                                     S.WGS_PER_CU[S.GLOBAL])
    # no table is more than half full, and the LDS tables fit four workgroups a CU beside each other
    assert S.WAVE_SLOTS >= 2 * S.WAVE_ROW and S.BLOCK_SLOTS >= 2 * S.BLOCK_ROW and 4 * 16 * S.BLOCK_SLOTS <= 160 * 1024
    assert [S.table_log2(x) for x in (1, 128, 129, 1024, 1025, 2048, 2049)] == [8, 8, 11, 11, 12, 12, 13]
    assert [S.table_log2(x, True) for x in (1, 32, 33, 100, 1000, 2000)] == [6, 6, 7, 8, 11, 12]


def _row_lengths(n, edges):
    deg = np.zeros(n, dtype=np.int64)
    for u, v, _ in edges:
        deg[u] += 1
        deg[v] += 1
    return deg


def test_sets_hold_their_cases():
    for length in S.BOUNDARY_LENGTHS:
        n, edges, labels = S.boundary_star(length)
        deg = _row_lengths(n, edges)
        assert deg[n - 1] == length and deg[:n - 1].max() <= 3
        leaves = labels[[v for u, v, _ in edges if u == n - 1]]
        assert len(set(leaves[leaves >= 0].tolist())) == 5 and (leaves < 0).sum() >= 3
        rec = R.silhouette(n, edges, labels)
        assert int(rec[n - 1]["b_cluster"]) != NONE and int(rec[n - 1]["far_q"]) == ONE // 2  # it lists all of its own cluster
    for lg, length in S.COLLIDING_ROWS.items():
        n, edges, labels = S.colliding_star(lg)
        deg = _row_lengths(n, edges)
        assert deg[n - 1] == length and S.table_log2(length) == lg == S.table_log2(length, True)
        assert S.path_of(length) == {8: S.WAVE, 11: S.WORKGROUP, 12: S.GLOBAL}[lg]
        row = [int(labels[v if u == n - 1 else u]) for u, v, _ in edges]
        last = [d for d in set(row) | {int(labels[n - 1])} if home_slot(d, lg) == (1 << lg) - 1]
        assert len(last) >= 10  # they share the last slot as their home: all but one sit past the wrap, from slot 0 on
        assert len(set(row)) <= length // 2
        rec = R.silhouette(n, edges, labels)
        best = int(rec[n - 1]["b_cluster"])
        assert best in last and best == min(d for d in last if d != labels[n - 1] and row.count(d) == 1 and
                                            any(q == ONE // 8 for u, v, q in edges if labels[v if u == n - 1 else u] == d))
    n, edges, labels = S.arithmetic()
    rec = R.silhouette(n, edges, labels)
    assert (int(rec[0]["b_num"]), int(rec[0]["b_den"]), int(rec[0]["b_cluster"])) == (ONE, 2, 1)  # equal to cluster 2's 2 ONE / 4
    assert (int(rec[1]["b_num"]), int(rec[1]["b_den"]), int(rec[1]["b_cluster"]), int(rec[1]["near_q"]), int(rec[1]["near_cluster"])) == (ONE, 1, NONE, ONE, 1)
    assert int(rec[1]["far_q"]) == ONE // 4 and int(rec[2]["far_q"]) == 3 * ONE // 4 and int(rec[2]["near_cluster"]) == NONE
    assert [int(rec[10][f]) for f in R.FIELDS] == [0, 0, 0, 0, NONE, 0, 0, NONE]
    assert (int(rec[9]["a_den"]), int(rec[9]["far_q"]), int(rec[9]["near_q"]), int(rec[9]["near_cluster"])) == (0, 0, ONE // 8, 2)
    without = R.silhouette(n, [e for e in edges if 10 not in e[:2]], labels)
    assert without.tobytes() == rec.tobytes()  # the unclustered vertex's records change nothing


def _row_tables(n, edges, labels):
    """what the row kernel gathers of every clustered vertex with a row: (cluster -> [listed neighbours, sum of q], far, near)"""
    rows = {}
    for u, v, q in edges:
        for x, y in ((u, v), (v, u)):
            if labels[x] < 0:
                continue
            tab, far, near = rows.setdefault(x, ({}, 0, (ONE, NONE)))
            if labels[y] < 0:
                continue  # the entry stands in the row; its neighbour is a member of nothing
            d = int(labels[y])
            slot = tab.setdefault(d, [0, 0])
            slot[0] += 1
            slot[1] += q
            rows[x] = (tab, max(far, q) if d == labels[x] else far, near if d == labels[x] else min(near, (q, d)))
    return rows


def _record_of(tab, far, near, c, size, clustered):
    """sil_rule's sweep and finish over a gathered table, as (a_num, b_num, a_den, b_den, b_cluster, far_q, near_q, near_cluster)"""
    n_c = int(size[c])
    cnt_c, sum_c = tab.get(c, (0, 0))
    best = None
    for d, (cnt, total) in tab.items():
        if d == c:
            continue
        n_d = int(size[d])
        s_d = total + (n_d - cnt) * ONE
        if best is None or s_d * best[1] < best[0] * n_d or (s_d * best[1] == best[0] * n_d and d < best[2]):
            best = (s_d, n_d, d)
    if best is None or not best[0] < best[1] * ONE:
        best = (ONE, 1, NONE) if clustered > n_c else (0, 0, NONE)
    return (sum_c + (n_c - 1 - cnt_c) * ONE, best[0], n_c - 1, best[1], best[2], ONE if cnt_c < n_c - 1 else far, near[0], near[1])


@pytest.mark.parametrize("num_cu", [64, 256, 304])
def test_the_row_grids_take_a_second_turn(num_cu):
    """many_short_rows and many_long_rows (tests/test_gpu_quality.py runs them): more rows on a path than row_kernel's grid there
    has workgroups, and a row gathered on top of the table of the row its workgroup scored a turn earlier gives another record"""
    for build, all_global, path in ((S.many_short_rows, False, S.WAVE), (S.many_short_rows, True, S.GLOBAL), (S.many_long_rows, False, S.WORKGROUP)):
        n, edges, labels = build(num_cu)
        deg = _row_lengths(n, edges)
        assert set(deg.tolist()) == ({6} if build is S.many_short_rows else {S.WAVE_ROW + 2})
        assert len(set(q for _, _, q in edges)) == 8 and len(set(labels[labels >= 0].tolist())) == 9 and (labels < 0).sum() == n // 41
        listed = [x for x in range(n) if labels[x] >= 0]  # the path's list: every clustered vertex has a row, all of one length
        assert {S.path_of(int(deg[x]), all_global) for x in listed} == {path}
        grid = min(len(listed), S.WGS_PER_CU[path] * num_cu)
        assert grid == S.WGS_PER_CU[path] * num_cu < len(listed)
        rows = _row_tables(n, edges, labels)
        want = R.silhouette(n, edges, labels)
        size = np.bincount(labels[labels >= 0], minlength=n)
        clustered = int((labels >= 0).sum())
        differ = 0
        for i, x in enumerate(listed):
            tab, far, near = rows[x]
            clean = _record_of(tab, far, near, int(labels[x]), size, clustered)
            assert clean == tuple(int(want[x][f]) for f in R.FIELDS), x  # the model with a cleared table is the restatement
            if i < grid:
                continue
            stale = {d: list(v) for d, v in rows[listed[i - grid]][0].items()}
            for d, (cnt, total) in tab.items():
                slot = stale.setdefault(d, [0, 0])
                slot[0] += cnt
                slot[1] += total
            differ += _record_of(stale, far, near, int(labels[x]), size, clustered) != clean
        assert 10 * differ >= 9 * (len(listed) - grid), (differ, len(listed) - grid)
    n, edges, labels = S.many_long_rows(num_cu)
    assert (labels >= 0).sum() < S.WGS_PER_CU[S.GLOBAL] * num_cu  # under RTC_SIL_GLOBAL=1 the long rows stay within one turn


def test_the_large_set_needs_128_bits():
    n, edges, labels = S.past_64_bits()
    n1, n2 = (1 << 22) + 256, (1 << 22) + 2
    assert n == 2 + n1 + n2 and int((labels == 2).sum()) == n1 and int((labels == 3).sum()) == n2
    p1, p2 = S.big_products(n, edges, labels, 0)  # cluster 2's S times cluster 3's N, and the other way round
    assert (p1, p2) == ((1 << 64) + 2, (1 << 64) - 256)
    right = 2 if p1 < p2 else 3
    assert right == 3  # the larger id is the nearer cluster
    # a product kept to 64 bits: the high words differ and the low words stand in the reverse order -- the wrong cluster
    mask = (1 << 64) - 1
    assert p1 >> 64 != p2 >> 64
    assert (2 if (p1 & mask) <= (p2 & mask) else 3) == 2 != right
    # the products as doubles tie, and so do the means as doubles: the tie goes to the smaller id -- the wrong cluster
    assert float(p1) == float(p2)
    s1, s2 = p1 // n2, p2 // n1
    assert float(s1) / float(n1) == float(s2) / float(n2)
    assert (2 if float(p1) <= float(p2) else 3) == 2 != right
    # and the means as integers tie as well
    assert s1 // n1 == s2 // n2
    rec = R.silhouette(n, edges, labels)
    assert (int(rec[0]["b_cluster"]), int(rec[0]["b_den"]), int(rec[0]["b_num"])) == (3, n2, s2)
    assert int(rec[0]["near_q"]) == 0 and int(rec[0]["near_cluster"]) == 2
    assert int(rec[1]["b_cluster"]) == 3  # (N - 1/2) / N is the smaller for the smaller cluster
    assert int(rec[n - 1]["a_num"]) == (n2 - 1) * ONE and int(rec[n - 1]["b_den"]) == 1
    deg0 = sum(1 for u, v, _ in edges if 0 in (u, v))
    assert S.WAVE_ROW < deg0 <= S.BLOCK_ROW  # vertex 0's row takes the workgroup path


def test_report_columns_from_hand_made_records():
    from rabbittclust_amd import api, host
    rec = np.zeros(6, dtype=R.SIL_DT)
    #           a_num        b_num    a_den b_den b_cluster far_q        near_q    near_cluster
    rec[0] = (ONE // 2,     ONE,      2,    1,    NONE,     ONE // 2,    ONE,      NONE)
    rec[1] = (3 * ONE // 2, ONE // 2, 2,    3,    1,        ONE,         ONE // 8, 1)
    rec[2] = (0,            ONE // 4, 0,    2,    0,        0,           ONE // 8, 0)
    rec[3] = (ONE,          3 * ONE,  2,    3,    2,        ONE // 16,   ONE // 8, 2)
    rec[4] = (ONE // 3,     ONE,      1,    1,    NONE,     ONE // 3,    ONE // 4, 0)
    rec[5] = (ONE // 3,     ONE // 5, 1,    3,    0,        ONE // 3,    ONE // 4, 2)
    clusters = [[3, 0, 1], [2], [5, 4]]  # as the result file lists them; members in any order
    names = ["g%d.fna" % g for g in range(6)]
    cluster_of = [0, 0, 1, 0, 2, 2]
    sil = api.silhouette_value(rec)
    q, s = host.quality_report(names, cluster_of, rec, sil)
    want_q, want_s = R.reports(names, clusters, rec)
    assert q == want_q and s == want_s
    with pytest.raises(ValueError):  # the reports are of a run's clusters: no genome is outside them
        host.quality_report(names, [0, 0, -1, 0, 2, 2], rec, sil)
    rows = [ln.split("\t") for ln in q.split("\n")]
    assert rows[0] == ["cluster", "size", "mean_silhouette", "min_silhouette", "mean_intra_distance", "diameter", "separation", "nearest_cluster"]
    v = [R.value(rec[g]) for g in range(6)]
    assert rows[1] == ["0", "3", "%.6f" % (((v[0] + v[1]) + v[3]) / 3.0), "%.6f" % min(v[0], v[1], v[3]), "%.6f" % (3.0 / 6.0), "1.000000", "0.125000", "1"]
    assert rows[2] == ["1", "1", "0.000000", "0.000000", "0.000000", "0.000000", "0.125000", "0"]
    assert rows[3] == ["2", "2", "%.6f" % ((v[4] + v[5]) / 2.0), "%.6f" % min(v[4], v[5]), "%.6f" % ((2 * (ONE // 3)) / (2.0 * ONE)), "0.333333", "0.250000", "0"]
    assert rows[4] == ["all", "6", "%.6f" % (sum(v[g] for g in range(6)) / 6.0), "-", "-", "-", "-", "-"] and rows[5] == [""]
    lines = s.split("\n")
    assert lines[0] == "name\tcluster\tsilhouette\ta\tb\tb_cluster" and lines[-1] == "" and len(lines) == 8
    assert lines[1] == "g0.fna\t0\t%.6f\t0.250000\t1.000000\t-" % v[0]
    assert lines[3] == "g2.fna\t1\t0.000000\t0.000000\t0.125000\t0"
    assert lines[6] == "g5.fna\t2\t%.6f\t0.333333\t0.066667\t0" % v[5]


# ---- the command line ----------------------------------------------------------------------------------------------------------
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
    r = _mst(base + ["--fast", "-o", out, "--quality"] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: --quality does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_refusals_keep_the_order_of_precedence(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    order = [(["-c", "1000"], "-c/--containment"), (["--inverted-index=false"], "--inverted-index=false"), (["--premsted", "nowhere"], "--premsted"),
             (["--db", "x.db", "--build"], "--db"), (["--dense"], "--dense"), (["--auto-threshold"], "--auto-threshold"), (["--stability"], "--stability")]
    for i in range(len(order) - 1):
        flags = [f for fl, _ in order[i:] for f in fl]
        r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out, "--quality"] + flags, str(tmp_path))
        assert r.returncode == 1 and f"ERROR: --quality does not go with {order[i][1]}\n" in r.stderr, (i, r.stderr)
    # --linkage and --nj-tree speak first where they stand beside it
    r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out, "--quality", "--linkage", "complete", "--dense"], str(tmp_path))
    assert r.returncode == 1 and "ERROR: --linkage does not go with --dense\n" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "  --quality (" in h.stdout and ".quality.tsv" in h.stdout and ".silhouette.tsv" in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out, "--quality"], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and "ERROR: unknown option --quality\n" in r.stderr, tool
        hh = subprocess.run([os.path.join(BIN, tool), "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60,
                            env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert "--quality" not in hh.stdout, tool
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_quality_calls():
    from rabbittclust_amd import _lib
    lib = _lib.load()
    for name in ("rtc_silhouette", "rtc_silhouette_counters", "rtc_silhouette_last_path", "rtc_silhouette_value", "rtc_cluster_quality",
                 "rtc_cluster_quality_counters"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
