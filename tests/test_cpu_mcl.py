"""rtc_mcl without a GPU: the restatement (tests/refmcl.py) on the cases worked out on paper and on the family sets, the inputs
of tests/mcl_sets.py shown to hold their cases, and the command line's refusals, which all come before a context exists."""
import os
import subprocess

import pytest

from tests import mcl_sets as S
from tests import refmcl as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-leiden")
ONE = R.ONE


# ---- the cases on paper ----
def test_path_of_nine():
    n, rec, sel = S.path9()
    labels, iterations, converged, M = R.mcl(n, rec, 4, sel, 100)
    assert converged == 1
    assert [a for a in range(n) if M[a].get(a, 0) > 0] == [1, 7]
    assert M[4] == {1: 1 << 29, 7: 1 << 29}
    assert labels == [0, 0, 0, 0, 0, 5, 5, 5, 5]  # vertex 4 goes to the lower of its two equal attractors


def test_one_edge_and_no_edge():
    n, rec, sel = S.one_edge()
    labels, iterations, converged, M = R.mcl(n, rec, 4, sel, 100)
    assert labels == [0, 0] and converged == 1
    n, rec, sel = S.empty()
    labels, iterations, converged, M = R.mcl(n, rec, 4, sel, 100)
    assert labels == [0, 1, 2, 3, 4] and iterations == 1 and converged == 1
    assert M == [{j: ONE} for j in range(n)]
    assert R.mcl(n, rec, 4, sel, 0)[1:3] == (0, 0)  # T == 0: the start matrix, not converged


def test_ring_of_forty():
    n, rec, sel = S.ring40()
    labels, iterations, converged, _ = R.mcl(n, rec, 4, sel, 100)
    assert (iterations, converged) == (60, 1)


def test_two_cliques_and_duplicates():
    n, rec, sel = S.two_cliques()
    assert R.mcl(n, rec, 4, sel, 100)[0] == [0] * 6 + [6] * 6
    n, rec, sel = S.duplicates()
    adj = R.adjacency(n, rec)
    assert adj[0][1] == adj[1][0] == 17 * S.UNIT // 16 and adj[4][5] == adj[5][4] == 18 * S.UNIT // 16  # layers and orientations summed
    assert all(x not in adj[x] for x in range(n)) and adj[8] == {}  # the self records are gone
    assert R.mcl(n, rec, 4, sel, 100)[0] == [0, 0, 0, 0, 4, 4, 4, 4, 8]


def test_isqrt_half_step():
    """inflation 1.5 and 2.5 on a value whose root is irrational: floor of the exact root, then the products' floors"""
    e = 3 * ONE // 4
    root = R.isqrt(e << 30)
    assert root * root <= e << 30 < (root + 1) * (root + 1)
    assert R.inflate(e, 3) == (e * root) >> 30
    assert R.inflate(e, 5) == ((((e * e) >> 30) * root) >> 30)
    assert R.inflate(e, 4) == (e * e) >> 30 and R.inflate(ONE, 16) == ONE


def test_refusals_of_the_definition():
    n, rec, sel = S.summed((1 << 32) - 1)
    assert R.start(n, rec, sel)[0][1] > 0
    with pytest.raises(R.Refused) as e:
        R.start(*S.summed(1 << 32))
    assert e.value.status == "RTC_ERR_UNSUPPORTED"
    for bad in ([(0, 3, 1)], [(0, 1, 0)]):
        with pytest.raises(R.Refused) as e:
            R.start(3, bad, 8)
        assert e.value.status == "RTC_ERR_ARG"
    for h, sel in ((2, 8), (17, 8), (4, 0), (4, 4097)):
        with pytest.raises(R.Refused):
            R.mcl(2, [(0, 1, 1)], h, sel, 1)


# ---- the sets hold their cases ----
def test_constants_agree_with_the_header():
    from rabbittclust_amd import api
    assert (api.MCL_WAVE_WORK, api.MCL_BLOCK_WORK) == S.boundaries()
    assert api.MCL_WAVE_WORK < api.MCL_BLOCK_WORK
    # what the turn sets are built from: the tables' sizes, the hash's multiplier and the launches' workgroups a CU.  A change
    # of one of these asks for the sets to be sized again.
    c = S.constants()
    assert (c["MCL_WAVE_SLOTS"], c["MCL_BLOCK_SLOTS"], c["MCL_GLOBAL_LOG2_MIN"], c["MCL_GOLDEN"]) == (512, 4096, 10, 2654435761)
    assert S.grids(S.CUS, S.TURNS_N) == (8 * S.CUS, 32 * S.CUS, 3 * S.CUS, 4 * S.CUS)
    assert S.grids(2, 5) == (5, 5, 5, 5)
    assert not set(S.turn_sets()) & set(S.every_set())


def test_boundary_sets_hold_the_three_works():
    wave, block = S.boundaries()
    seen = set()
    for B in (wave, block):
        (n, rec, sel), probes = S.boundary(B)
        assert n <= 3000
        W = S.work(R.start(n, rec, sel))
        assert [W[p] for p in probes] == [B - 1, B, B + 1]
        seen |= {0 if w <= wave else 1 if w <= block else 2 for w in W}
    assert seen == {0, 1, 2}  # the first iteration alone takes all three paths


def test_selection_sets_cut():
    n, rec, sel = S.hub_star()
    M = R.start(n, rec, sel)
    assert len(R.adjacency(n, rec)[0]) == 20 > sel and len(M[0]) == sel  # the start matrix is cut
    for sel in (8, 64):
        n, rec, _ = S.tied_clique(sel)
        M = R.start(n, rec, sel)
        assert all(sorted(col) == list(range(min(sel, 30))) for col in M)  # equal values: the lowest rows stay
    n, rec, sel = S.families("families_12x15_s8")
    assert any(len(col) == sel for col in R.start(n, rec, sel))


def test_record_order_does_not_matter():
    n, rec, sel = S.families("families_12x15_s8")
    assert R.start(n, S.shuffled(rec), sel) == R.start(n, rec, sel)


@pytest.mark.parametrize("name", sorted(S.FAMILY_SETS))
def test_family_sets(name):
    """exactly the families at inflation 1.5, 2 and 2.5, at an exact fixed point after the iterations of the table"""
    for h, want in zip((3, 4, 5), S.FAMILY_ITERATIONS[name]):
        labels, iterations, converged, _ = S.expected(name, h, 100)
        assert labels == S.family_of(name), h
        assert (iterations, converged) == (want, 1), h


def test_high_inflation_splits_families():
    n, rec, sel = S.families("families_12x15")
    for h in (12, 16):
        labels, iterations, converged, _ = R.mcl(n, rec, h, sel, 100)
        assert converged == 1 and iterations <= 10 and len(set(labels)) > 12


def test_fallback_rule_without_convergence():
    """stopped early, a column without an attractor takes its largest row of any kind"""
    n, rec, sel = S.chain_s1()
    for T, rows in ((0, [0, 0, 1, 2, 3, 4]), (1, [0, 0, 0, 1, 2, 3]), (2, [0, 0, 0, 0, 0, 1])):
        labels, iterations, converged, M = R.mcl(n, rec, 4, sel, T)
        assert [list(col) for col in M] == [[r] for r in rows] and (iterations, converged) == (T, 0)
        assert not M[5].get(5) and not M[rows[5]].get(rows[5])  # column 5 names a row that is no attractor
        assert labels == [0] * 6
    assert R.mcl(n, rec, 4, sel, 100)[1:3] == (4, 1)
    n, rec, sel = S.path9()
    labels, iterations, converged, M = R.mcl(n, rec, 4, sel, 2)
    assert (iterations, converged) == (2, 0) and labels == R.clusters(M)


# ---- the turn sets hold their cases (tests/test_gpu_mcl_turns.py runs them) ----
def test_turn_sets_give_every_launch_more_columns_than_workgroups():
    """on the 256 CUs of an MI355X: more vertices than mcl_start_kernel has workgroups, in every early iteration more wave
    columns than the wave launch has workgroups and more workgroup columns than the workgroup launch has, and at S = 8
    every column on the wave path, a good part of them cut"""
    T = S.turn_sets()
    wave_work, block_work = S.boundaries()
    start, wave, block, glob = S.grids(S.CUS, S.TURNS_N)
    n, rec, sel = T["turns_10k"]
    assert n == S.TURNS_N > start and sel == 1024
    mats, _ = S.trajectory("turns_10k", 4, T, upto=3)
    counts = [S.path_counts(M) for M in mats[:3]]  # of the iterations 1, 2 and 3
    assert all(sum(c) == n for c in counts)
    assert counts[0][0] > wave and counts[0][1] > block and counts[0][2] == 0
    for c in counts[1:]:
        assert c[0] > wave and c[1] > block and 0 < c[2] < glob  # the global launch takes a second turn under the switch only,
    assert n > glob                                             # where it gets all n columns
    assert S.cuts("turns_10k", 4, 3, T) == 0
    # from the second iteration the global columns take tables of more than one size, the largest there is among them; under
    # the switch the others take the smallest
    for M in mats[1:3]:
        W = S.work(M)
        sizes = {S.table_log2(w, n, sel) for w in W if w > block_work}
        assert len(sizes) > 1 and max(sizes) == 15 and min(sizes) > 10
        assert all(2 * min(w, n) > 1024 for w in W if w > block_work)
        assert {S.table_log2(w, n, sel) for w in W} >= sizes | {10}
    assert T["turns_10k_s8"][:2] == (n, rec) and T["turns_10k_s8"][2] == 8
    mats8, _ = S.trajectory("turns_10k_s8", 4, T, upto=3)
    assert all(S.path_counts(M) == (n, 0, 0) for M in mats8[:3]) and n > wave
    cut = [S.cuts("turns_10k_s8", 4, t, T) for t in range(4)]
    assert cut[0] > 1000 and all(b - a > 1000 for a, b in zip(cut, cut[1:]))
    assert all(len(col) <= 8 for M in mats8 for col in M) and not any(len(col) == 0 for M in mats + mats8 for col in M)


def test_wrap_cliques_run_off_the_last_slot():
    """the row set of every column of the two wrap cliques, put into its table by linear probing: slot 0 ends up holding a
    row whose home is among the table's last slots -- in the LDS table of its path and in the smallest global table"""
    T = S.turn_sets()
    wave_work, block_work = S.boundaries()
    wave_ids, block_ids = S.wrap_ids()
    assert len(wave_ids) == 12 and len(block_ids) == 18 and not set(wave_ids) & set(block_ids)
    assert max(wave_ids + block_ids) < S.TURNS_N
    # (log2 of the table's slots, the slots at its end that hold the homes); at S = 8 every column takes the wave table
    for name, cases in (("turns_10k", ((wave_ids, ((9, 4), (10, 8))), (block_ids, ((12, 8), (10, 8))))),
                        ("turns_10k_s8", ((wave_ids, ((9, 4),)), (block_ids, ((9, 4),))))):
        M = S.trajectory(name, 4, T, upto=0)[0][0]
        for ids, tables in cases:
            for j in ids:
                rows = set().union(*(M[k] for k in M[j]))  # the rows that column j's expansion reaches in the first iteration
                W = sum(len(M[k]) for k in M[j])
                if name == "turns_10k":
                    assert rows == set(ids) and W == len(ids) ** 2
                    assert W <= wave_work if ids is wave_ids else wave_work < W <= block_work
                else:
                    assert rows <= set(ids) and len(rows) >= 8 and W <= wave_work
                for log2, tail in tables:
                    slots = S.probe_fill(sorted(rows), log2)
                    assert sorted(slots.values()) == sorted(rows)
                    assert (1 << log2) - 1 in slots and 0 in slots and S.home(slots[0], log2) >= (1 << log2) - tail, (name, j, log2)


def test_hub_300_is_cut_among_equals_past_one_turn_of_the_lanes():
    T = S.turn_sets()
    n, rec, _ = T["hub_300_s64"]
    assert T["hub_300_s1024"][:2] == (n, rec)
    adj = R.adjacency(n, rec)
    hub = S.HUB_300
    assert len(adj[hub]) == 300 > 256  # the lanes of mcl_start_kernel
    keys = sorted(list(adj[hub].items()) + [(hub, max(adj[hub].values()))], key=lambda e: (-e[1], e[0]))
    assert keys[63][1] == keys[64][1] and keys[63][0] < keys[64][0]  # the 64th and the 65th differ by the row alone
    assert sorted(R.start(n, rec, 64)[hub]) == sorted(i for i, _ in keys[:64]) and hub in R.start(n, rec, 64)[hub]
    assert len(R.start(n, rec, 1024)[hub]) == 301
    assert (S.cuts("hub_300_s64", 4, 0, T), S.cuts("hub_300_s1024", 4, 0, T)) == (1, 0)
    assert S.cuts("hub_300_s64", 4, 1, T) > 1 and S.cuts("hub_300_s1024", 4, 1, T) == 0


@pytest.mark.parametrize("h", range(6, 17))
def test_high_inflation_leaves_no_column_empty(h):
    """inflation 3 to 8: the product loop of mcl_inflate takes two to seven turns.  The largest entry of a column inflates to
    ONE, so no column empties and every set reaches its fixed point.  One turn of the loop fewer gives another matrix after the
    first iteration already (but for the clique of equal weights, whose entries all are the largest), so a kernel that took
    a wrong number of turns would not meet the restatement."""
    for name in S.HIGH_INFLATION_SETS:
        mats, converged = S.trajectory(name, h)
        assert converged and len(mats) >= 2, name
        assert all(col for M in mats for col in M), name
        assert mats[1] != S.trajectory(name, h - 2)[0][1] or name == "tied_clique_s8", name


# ---- the command line ----
def _run(args):
    if not os.path.exists(BIN):
        pytest.fail("clust-leiden missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env)


_IN = ["--fast", "-l", "-i", "list.txt", "-o", "o.txt"]


@pytest.mark.parametrize("args,msg", [
    (["--mcl", "--louvain"] + _IN, "ERROR: --mcl does not go with --louvain\n"),
    (["--mcl", "--leiden"] + _IN, "ERROR: --mcl does not go with --leiden\n"),
    (["--mcl", "--resolution", "0.5"] + _IN, "ERROR: --mcl does not go with --resolution\n"),
    (["--mcl", "--objective", "modularity"] + _IN, "ERROR: --mcl does not go with --objective\n"),
    (["--mcl", "--db", "m.db", "--build"] + _IN, "ERROR: --mcl does not go with --db --build\n"),
    (["--mcl", "--inflation", "1.7"] + _IN, "ERROR: --inflation must be a multiple of 0.5 between 1.5 and 8, got 1.7\n"),
    (["--mcl", "--inflation", "1"] + _IN, "ERROR: --inflation must be a multiple of 0.5 between 1.5 and 8, got 1\n"),
    (["--mcl", "--inflation", "8.5"] + _IN, "ERROR: --inflation must be a multiple of 0.5 between 1.5 and 8, got 8.5\n"),
    (["--mcl", "--inflation", "nan"] + _IN, "ERROR: --inflation must be a multiple of 0.5 between 1.5 and 8, got nan\n"),
    (["--mcl", "--mcl-select", "0"] + _IN, "ERROR: --mcl-select must be between 1 and 4096, got 0\n"),
    (["--mcl", "--mcl-select", "4097"] + _IN, "ERROR: --mcl-select must be between 1 and 4096, got 4097\n"),
    (["--louvain", "--inflation", "2"] + _IN, "ERROR: --inflation needs --mcl\n"),
    (["--leiden", "--mcl-select", "64"] + _IN, "ERROR: --mcl-select needs --mcl\n"),
    (["--louvain", "--mcl-iterations", "10"] + _IN, "ERROR: --mcl-iterations needs --mcl\n"),
])
def test_mcl_refusals_exit_before_the_gpu(args, msg, tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run([out if a == "o.txt" else a for a in args])
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr
    assert "context" not in r.stderr and "Building similarity graph" not in r.stderr and "-----Algorithm" not in r.stderr
    assert not os.path.exists(out)


def test_existing_messages_stay(tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run(["--fast", "-l", "-i", "list.txt", "-o", out])
    last = r.stderr.splitlines()[-2:]
    assert r.returncode == 1 and last[0] == "ERROR: Leiden refinement is not in this build; run with --louvain"
    assert last[1].startswith("NOTE: ") and "--leiden" in last[1] and "--louvain" in last[1] and "--mcl" in last[1]
    assert r.stderr.count("ERROR") == 1
    r = _run(["--fast", "--leiden", "--louvain", "-l", "-i", "list.txt", "-o", out])
    assert r.returncode == 1 and "ERROR: --leiden and --louvain exclude each other\n" in r.stderr


def test_mcl_takes_the_knn_default_of_leiden(tmp_path):
    """the flags pass and the algorithm is named with its parameters; the run ends at the drlevel check, after the defaulting"""
    r = _run(["--mcl", "--inflation", "2.5", "--mcl-select", "64", "--mcl-iterations", "7", "--fast", "--drlevel", "9", "-l", "-i", "none", "-o",
              str(tmp_path / "o.txt")])
    assert r.returncode == 1 and "ERROR: invalid drlevel 9" in r.stderr
    assert "-----Auto-selecting k-NN: k=500 (use --knn 0 to disable)\n" in r.stderr and "Auto-enabled" not in r.stderr
    assert "-----Algorithm: MCL (inflation 2.5, select 64)\n" in r.stderr and "(k=500)" in r.stderr
    r = _run(["--mcl", "--fast", "--drlevel", "9", "-l", "-i", "none", "-o", str(tmp_path / "o.txt")])
    assert "-----Algorithm: MCL (inflation 2, select 1024)\n" in r.stderr


def test_help_names_the_flags():
    r = _run(["-h"])
    assert r.returncode == 0
    for flag in ("--mcl", "--inflation", "--mcl-select", "--mcl-iterations"):
        assert flag in r.stdout
