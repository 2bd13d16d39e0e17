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
