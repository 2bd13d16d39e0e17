"""rtc_graph_snn without a GPU: the restatement (tests/refsnn.py) on the cases worked out on paper, rtc_snn_weight bit for bit
against Python's division, the inputs of tests/snn_sets.py shown to hold their cases, and the command line's refusals, which all
come before a context exists."""
import os
import subprocess

import pytest

from tests import refsnn as R
from tests import snn_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


def _weights(name):
    from rabbittclust_amd import api
    n, rec = S.every_set()[name]
    out = []
    for (u, v), (s, du, dv, fl) in zip(rec, S.expected(name)):
        assert fl == 0
        w = api.snn_weight(s, du, dv)
        assert w == (s + 2) / (du + dv - s) == R.weight(s, du, dv)  # the one double division, bit for bit
        N = R.neighbourhoods(n, rec)
        both, either = R.weight_of_sets(N, u, v)
        assert (both, either) == (s + 2, du + dv - s) and either >= 2 and 0 < w <= 1  # the closed neighbourhoods' Jaccard index
        out.append(w)
    return out


# ---- the cases on paper ----
def test_single_edge():
    assert S.expected("single_edge") == [(0, 1, 1, 0)] and _weights("single_edge") == [1.0]


def test_path_of_three():
    assert S.expected("path3") == [(0, 1, 2, 0), (0, 2, 1, 0)] and _weights("path3") == [2 / 3, 2 / 3]


def test_triangle_and_k5():
    assert S.expected("triangle") == [(1, 2, 2, 0)] * 3 and _weights("triangle") == [1.0] * 3
    assert S.expected("k5") == [(3, 4, 4, 0)] * 10 and _weights("k5") == [1.0] * 10
    assert S.expected_counters("k5") == (10, 10, 40, 10)


def test_star_of_seventy():
    assert S.expected("star70") == [(0, 70, 1, 0)] * 70 and _weights("star70") == [2 / 71] * 70
    assert S.expected_counters("star70") == (70, 0, 70, 70)


def test_two_k40_and_their_bridge():
    n, rec = S.every_set()["two_k40"]
    w = _weights("two_k40")
    assert rec[-1] == (39, 40) and S.expected("two_k40")[-1] == (0, 40, 40, 0) and w[-1] == 2 / 80
    inside = [x for (u, v), x in zip(rec[:-1], w) if 39 not in (u, v) and 40 not in (u, v)]
    at_bridge = [x for (u, v), x in zip(rec[:-1], w) if 39 in (u, v) or 40 in (u, v)]
    assert set(inside) == {1.0} and set(at_bridge) == {40 / 41} and len(at_bridge) == 78
    assert S.expected_counters("two_k40")[:2] == (2 * 780 + 1, 2 * 9880)


def test_records_as_a_file_may_hold_them():
    n, rec = S.every_set()["messy"]
    want = S.expected("messy")
    assert want[0] == want[2] and want[1] == (want[0][0], want[0][2], want[0][1], 0)  # a duplicate, and the reverse
    assert want[5] == (0, 3, 3, 1) and want[9] == (0, 0, 0, 1)  # u == v: the degrees still those of G
    assert R.neighbourhoods(n, rec)[7] == set() and R.edges(n, rec) == [(0, 1), (0, 2), (0, 3), (1, 2), (2, 3), (3, 4), (6, 8)]
    assert S.expected_counters("messy") == (7, 2, R.probes(n, rec), 11)
    out, pruned = R.reweighted(n, rec, [0.25] * len(rec), 0.6)
    assert (2, 2, 0.25) not in out and pruned == len(rec) - len(out)  # a self record keeps its weight, and is pruned by it
    assert (2, 2, 0.25) in R.reweighted(n, rec, [0.25] * len(rec), 0.2)[0]
    for bad in ([(0, 9)], [(9, 0)]):
        with pytest.raises(R.Refused):
            R.snn(9, bad)
    with pytest.raises(R.Refused):
        R.snn((1 << 31) - 1, [])


# ---- the sets hold their cases ----
def test_constants_agree_with_the_header():
    from rabbittclust_amd import api
    c = S.constants()
    assert (api.SNN_WAVE_ROW, api.SNN_BLOCK_ROW) == S.boundaries() and 64 < api.SNN_WAVE_ROW < api.SNN_BLOCK_ROW
    # the derivation of rtc_snn.h: the slice's words and the row in the LDS share of a workgroup, at the residency named there
    assert c["SNN_WAVE_ROW"] * 4 + 64 * c["SNN_SLICE_BYTES"] + 8 <= 160 * 1024 // c["SNN_WAVE_WGS_PER_CU"]
    assert c["SNN_BLOCK_ROW"] * 4 + 256 * c["SNN_SLICE_BYTES"] + 32 <= 160 * 1024 // c["SNN_BLOCK_WGS_PER_CU"]


def test_sets_hold_their_cases():
    wave, block = S.boundaries()
    assert all(s == 128 and du == dv == 129 for s, du, dv, _ in S.expected("k130")) and 129 > 2 * 64
    assert all((s, du, dv) == (0, 65, 65) for s, du, dv, _ in S.expected("k65_65"))
    for seed in (1, 2, 3):
        n, rec = S.every_set()["random_%d" % seed]
        assert n == 300 and len(rec) > 300 and len(set(s for s, _, _, _ in S.expected("random_%d" % seed))) > 5
        assert len(R.edges(n, rec)) < len(rec)  # two vertices named each other somewhere: duplicates in both orientations
    paths = 0
    for row in S.hub_rows():
        n, rec = S.every_set()["hub_%d" % row]
        assert len(R.neighbourhoods(n, rec)[0]) == row
        w, b, g = S.expected_paths("hub_%d" % row)
        assert w == 10 * (row // 5) + (row if row <= wave else 0) and b == (row if wave < row <= block else 0) and g == (row if row > block else 0)
        assert S.hub_path(row) == (1 if w else 0) | (2 if b else 0) | (4 if g else 0)
        paths |= S.hub_path(row)
    assert paths == 7 and max(S.hub_rows()) > 256  # a hub owns more records than one slice holds


# ---- the library and its Python face ----
def test_symbols():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_graph_snn", "rtc_snn_weight", "rtc_graph_snn_counters", "rtc_graph_snn_last_path"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "rtclust.h")).read()
    assert "typedef struct { uint32_t shared, deg_u, deg_v, flags; } rtc_snn;" in header
    assert api.SNN_DT.itemsize == 16 and api.SNN_DT.names == ("shared", "deg_u", "deg_v", "flags")
    for name in ("graph_snn", "graph_snn_counters", "graph_snn_last_path"):
        assert callable(getattr(api.Context, name))
    assert api.snn_weight(0xffffffff, 0xffffffff, 0xffffffff) == (2 ** 32 + 1) / (2 ** 32 - 1)  # no 32-bit wrap in the sums


# ---- the command line ----
def _run(tool, args):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        pytest.fail("%s missing: run __graft_entry__.build()" % tool)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)


_IN = ["--fast", "--louvain", "-l", "-i", "list.txt", "-o", "o.txt"]


@pytest.mark.parametrize("args,msg", [
    (["--snn", "--db", "m.db", "--build"] + _IN, "ERROR: --snn does not go with --db\n"),
    (["--snn", "--db", "m.db", "--assign"] + _IN, "ERROR: --snn does not go with --db\n"),
    (["--snn", "--db", "m.db", "--stats"] + _IN, "ERROR: --snn does not go with --db\n"),
    (["--snn-prune", "0.5"] + _IN, "ERROR: --snn-prune needs --snn\n"),
    (["--snn", "--snn-prune", "1"] + _IN, "ERROR: --snn-prune must be in [0, 1)\n"),
    (["--snn", "--snn-prune", "-0.25"] + _IN, "ERROR: --snn-prune must be in [0, 1)\n"),
    (["--snn", "--snn-prune", "nan"] + _IN, "ERROR: --snn-prune must be in [0, 1)\n"),
    (["--snn", "--snn-prune", "half"] + _IN, "ERROR: --snn-prune must be in [0, 1)\n"),
])
def test_snn_refusals_exit_before_the_gpu(args, msg, tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run("clust-leiden", [out if a == "o.txt" else a for a in args])
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr
    assert "context" not in r.stderr and "Building similarity graph" not in r.stderr and "-----Algorithm" not in r.stderr
    assert not os.path.exists(out)


def test_existing_refusals_keep_their_wording(tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run("clust-leiden", ["--minhash", "--snn", "--db", "m.db", "--build", "--louvain", "-l", "-i", "list.txt", "-o", out])
    assert r.returncode == 1 and "ERROR: --minhash does not go with --db (models of MinHash sketches are out of scope)\n" in r.stderr
    r = _run("clust-leiden", ["--mcl", "--snn", "--db", "m.db", "--build", "--fast", "-l", "-i", "list.txt", "-o", out])
    assert r.returncode == 1 and "ERROR: --mcl does not go with --db --build\n" in r.stderr


def test_snn_passes_the_flag_checks(tmp_path):
    """the flags pass with every algorithm; the run ends at the drlevel check, after them"""
    for alg in (["--louvain"], ["--leiden"], ["--mcl"]):
        r = _run("clust-leiden", alg + ["--snn", "--snn-prune", "0.25", "--fast", "--drlevel", "9", "-l", "-i", "none", "-o", str(tmp_path / "o.txt")])
        assert r.returncode == 1 and "ERROR: invalid drlevel 9" in r.stderr and r.stderr.count("ERROR") == 1


@pytest.mark.parametrize("tool", ["clust-mst", "clust-greedy", "clust-dbscan"])
def test_the_other_tools_do_not_know_the_flags(tool, tmp_path):
    for flag in (["--snn"], ["--snn-prune", "0.5"]):
        r = _run(tool, flag + ["-l", "-i", "list.txt", "-o", str(tmp_path / "o.txt")])
        assert r.returncode == 1 and "unknown option %s" % flag[0] in r.stderr and "context" not in r.stderr


def test_help_names_the_flags():
    r = _run("clust-leiden", ["-h"])
    assert r.returncode == 0
    for flag in ("--snn", "--snn-prune"):
        assert flag in r.stdout
