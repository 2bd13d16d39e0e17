"""rtc_rep_screen without a GPU: the restatement (tests/refscreen.py) on a case worked out by hand, the generated set of
tests/screen_sets.py shown to reach the ground the GPU tests stand on, rtc_screen_identity against math.pow, the two report
writers through host.py, and the command line's refusals, which all come before a context exists."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import refscreen as R
import screen_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
A, B, C, D = 0, 1, 2, 3


# ---- the case on paper: X = {1..10}, A = {1..6}, B = {5,6,7,8}, C = {1,2,3}, D = {9,20,21,22} ----
def test_hand_case_min_unique_2():
    reps, x = S.hand()
    hits, sums, info = R.screen(reps, x, 1, 0, 2, 0)
    # picks A (6), B (2); then C by containment 3/3 before D 1/4, with what was left of them
    assert hits == [[(A, 6, 6, 6, 1), (B, 4, 4, 2, 2), (C, 3, 3, 0, 0), (D, 1, 4, 1, 0)]]
    assert sums == [(10, 9, 8, 4, 2)]
    assert info[0]["rounds"] == 2


def test_hand_case_min_unique_1():
    reps, x = S.hand()
    hits, sums, _ = R.screen(reps, x, 1, 0, 1, 0)
    assert hits == [[(A, 6, 6, 6, 1), (B, 4, 4, 2, 2), (D, 1, 4, 1, 3), (C, 3, 3, 0, 0)]]
    assert sums == [(10, 9, 9, 4, 3)]


def test_hand_case_max_picks_1():
    reps, x = S.hand()
    hits, sums, _ = R.screen(reps, x, 1, 0, 1, 1)
    # only A; the rest by containment: B 4/4 and C 3/3 tie at one, the lower slot first
    assert hits == [[(A, 6, 6, 6, 1), (B, 4, 4, 2, 0), (C, 3, 3, 0, 0), (D, 1, 4, 1, 0)]]
    assert sums == [(10, 9, 6, 4, 1)]


def test_hand_case_containment_half():
    reps, x = S.hand()
    hits, sums, _ = R.screen(reps, x, 1, S.Q20 // 2, 2, 0)
    assert [h[0] for h in hits[0]] == [A, B, C], "D (1 / 4) is not a hit at all"
    assert sums == [(10, 8, 8, 3, 2)]


def test_hand_case_live_mask_and_min_common():
    reps, x = S.hand()
    hits, sums, _ = R.screen(reps, x, 1, 0, 1, 0, live=[0, 1, 1, 1])
    assert hits == [[(B, 4, 4, 4, 1), (C, 3, 3, 3, 2), (D, 1, 4, 1, 3)]] and sums == [(10, 8, 8, 3, 3)]
    hits, sums, _ = R.screen(reps, x, 4, 0, 1, 0)
    assert hits == [[(A, 6, 6, 6, 1), (B, 4, 4, 2, 2)]] and sums == [(10, 8, 8, 2, 2)]


# ---- the generated set reaches every path and edge the GPU tests rely on ----
def test_generated_set_holds_its_cases():
    from rabbittclust_amd import api
    wave, block = api.SCREEN_WAVE_CANDS, api.SCREEN_BLOCK_CANDS
    assert 64 <= wave < block
    reps, samples, live = S.generated()
    assert len(reps) == 5000 and all(20 <= len(r) <= 60 for r in reps) and 0.05 < 1.0 - live.mean() < 0.15
    assert sum(1 for r in reps[:4900] if S.HUB in r) == 4900 and all(reps[4900 + i] == reps[3 * i] for i in range(100))
    hits, sums, info = S.reference(S.CONFIGS[0])
    n_elig = [s[3] for s in sums]
    print("eligible", n_elig, "picks", [s[4] for s in sums], "expansion", [i["expansion"] for i in info])
    assert any(n > block for n in n_elig), "no sample on the global path"
    assert any(wave < n <= block for n in n_elig), "no sample on the workgroup path"
    assert any(0 < s[3] <= wave and s[4] >= 2 for s in sums), "no sample of two picks on the wave path"
    assert wave < n_elig[S.MIX2] <= block and n_elig[S.MIX6] > block and n_elig[S.DRAWN] > block and 0 < n_elig[S.SMALL] <= wave
    assert sums[S.SMALL][4] >= 2
    assert info[S.DRAWN]["rounds"] > 256, "no sample of more rounds than a workgroup has lanes"
    assert any(i["ties"] for i in info), "no round decided by the lower slot"
    assert max(i["expansion"] for i in info) > 256, "no hash that expands past 256 match records"
    assert sums[S.EMPTY] == (0, 0, 0, 0, 0) and not hits[S.EMPTY]
    assert sums[S.DISJOINT][1:] == (0, 0, 0, 0) and sums[S.DISJOINT][0] > 0 and not hits[S.DISJOINT]
    # the order of the picks is not the order by containment: the duplicate of a picked representative ranks third by
    # containment (behind two that were taken whole) and is never picked
    by_cont = [r[0] for r in R.containment_order(hits[S.MIX6])]
    assert by_cont[:3] == [S.WHOLE_A, S.WHOLE_B, S.DUP_OF_A]
    picked = [r[0] for r in hits[S.MIX6] if r[4]]
    assert S.WHOLE_A in picked and S.WHOLE_B in picked and S.DUP_OF_A not in picked and picked != by_cont[:len(picked)]
    dup = [r for r in hits[S.MIX6] if r[0] == S.DUP_OF_A][0]
    assert dup[1] == dup[2] and dup[3] == 0 and dup[4] == 0
    # every pick removes a hash, the sum of unique over the picks is what is explained
    for q in range(len(samples)):
        assert sum(r[3] for r in hits[q] if r[4]) == sums[q][2] <= sums[q][1] <= sums[q][0]
        assert [r[4] for r in hits[q] if r[4]] == list(range(1, sums[q][4] + 1))
    # the second configuration thins the candidates to other paths, the third stops after three picks
    _, sums2, _ = S.reference(S.CONFIGS[1])
    print("eligible (2, 0.25)", [s[3] for s in sums2])
    assert [s[3] for s in sums2] != n_elig and all(a[3] <= b[3] for a, b in zip(sums2, sums))
    _, sums3, _ = S.reference(S.CONFIGS[2])
    assert [s[4] for s in sums3] == [min(s[4], 3) for s in sums]


def test_width_8_keeps_the_structure():
    reps, samples, _ = S.generated()
    r8, s8 = S.as_width(reps[:50], 8), S.as_width(samples, 8)
    mul = 0x9E3779B97F4A7C15
    for a, b in zip(reps[:50] + samples, r8 + s8):
        assert b.dtype == np.uint64 and sorted((x * mul) & (2 ** 64 - 1) for x in a) == [int(x) for x in b] and len(set(b.tolist())) == len(a)
    assert max(int(x.max()) for x in r8) > 2 ** 63, "no hash with the top bit set"


# ---- the library's constants, signatures and host function ----
def test_constants_follow_the_header():
    from rabbittclust_amd import api
    text = open(os.path.join(ROOT, "rabbittclust_amd", "csrc", "rtc_screen.h")).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint(?:32|64)_t (SCREEN_\w+) = (\d+);", text)}
    assert (api.SCREEN_WAVE_CANDS, api.SCREEN_BLOCK_CANDS) == (c["SCREEN_WAVE_CANDS"], c["SCREEN_BLOCK_CANDS"])
    assert (api.SCREEN_POS_BYTES, api.SCREEN_MATCH_BYTES) == (c["SCREEN_POS_BYTES"], c["SCREEN_MATCH_BYTES"])
    # the derivation of rtc_screen.h: the counts in the LDS share of a workgroup at the residency named there
    assert c["SCREEN_WAVE_CANDS"] * 4 + 16 <= 160 * 1024 // 32 and c["SCREEN_BLOCK_CANDS"] * 4 + 48 <= 160 * 1024 // 8
    assert (api.SCREEN_PATH_WAVE, api.SCREEN_PATH_BLOCK, api.SCREEN_PATH_GLOBAL) == (1, 2, 4) and api.SCREEN_Q20 == 1 << 20


def test_symbols():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_rep_screen", "rtc_rep_screen_counters", "rtc_rep_screen_last_path", "rtc_screen_identity"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "rtclust.h")).read()
    assert "typedef struct { uint32_t query, slot, common, size, unique, rank; } rtc_screen_hit;" in header
    assert "typedef struct { uint32_t n_hashes, n_matched, n_explained, n_hits, n_picks, pad; } rtc_screen_sum;" in header
    assert api.SCREEN_HIT_DT.itemsize == 24 and api.SCREEN_HIT_DT.names == ("query", "slot", "common", "size", "unique", "rank")
    assert api.SCREEN_SUM_DT.itemsize == 24 and api.SCREEN_SUM_DT.names == ("n_hashes", "n_matched", "n_explained", "n_hits", "n_picks", "pad")
    for name in ("rep_screen", "rep_screen_counters", "rep_screen_last_path"):
        assert callable(getattr(api.Context, name))


def test_identity_against_pow():
    from rabbittclust_amd import api
    assert api.screen_identity(0, 40, 21) == 0.0 and api.screen_identity(40, 40, 21) == 1.0
    for c, s, k in ((13, 40, 21), (1, 4000000, 19), (39, 40, 31)):
        assert api.screen_identity(c, s, k) == math.pow(float(c) / float(s), 1.0 / k) == R.identity(c, s, k)


# ---- the writers ----
def test_writers_on_a_hand_made_hit_list():
    from rabbittclust_amd import api, host
    names = ["mix.fna", "", "none.fna", "bare.fna"]
    rep_names = ["r0.fna", "r1.fna", "r2.fna"]
    cid, csz = [0, -1, 1], [4, 0, 2]
    hits = [[(2, 30, 40, 30, 1), (0, 12, 12, 5, 2), (1, 7, 50, 0, 0)], [(0, 12, 12, 12, 1)], [], []]
    sums = [(300, 41, 35, 3, 2), (12, 12, 12, 1, 1), (77, 0, 0, 0, 0), (0, 0, 0, 0, 0)]
    h = np.array(R.flat(hits), dtype=api.SCREEN_HIT_DT)
    s = np.array([x + (0,) for x in sums], dtype=api.SCREEN_SUM_DT)
    tsv, summary = host.screen_report(names, rep_names, cid, csz, h, s, 21)
    assert tsv == R.screen_tsv(names, rep_names, cid, csz, hits, sums, 21)
    assert summary == R.summary_tsv(names, sums)
    lines = tsv.split("\n")
    assert lines[0] == "#sample\trank\tcluster_id\trep_name\tcluster_size\tshared\trep_hashes\tcontainment\tidentity\tunique\tunique_share"
    assert lines[1] == "mix.fna\t1\t1\tr2.fna\t2\t30\t40\t0.750000\t%.6f\t30\t0.100000" % math.pow(0.75, 1 / 21)
    assert lines[2] == "mix.fna\t2\t0\tr0.fna\t4\t12\t12\t1.000000\t1.000000\t5\t0.016667"
    assert lines[3].startswith("mix.fna\t-\t-1\tr1.fna\t0\t7\t50\t0.140000\t")
    assert lines[4].startswith("query_1\t1\t0\tr0.fna\t")
    assert lines[5] == "none.fna\t0\t-1\tno_match\t0\t0\t0\t0.000000\t0.000000\t0\t0.000000" and lines[6].startswith("bare.fna\t0\t-1\tno_match")
    assert summary.split("\n")[:5] == ["#sample\thashes\tmatched\texplained\thits\tpicks\tunexplained_share",
                                       "mix.fna\t300\t41\t35\t3\t2\t0.883333", "query_1\t12\t12\t12\t1\t1\t0.000000",
                                       "none.fna\t77\t0\t0\t0\t0\t1.000000", "bare.fna\t0\t0\t0\t0\t0\t-"]
    with pytest.raises(ValueError):
        host.screen_report(names, rep_names, cid, csz, h[::-1], s, 21)


# ---- the command line ----
def _run(tool, args):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        pytest.fail("%s missing: run __graft_entry__.build()" % tool)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)


_DB = ["--fast", "--db", "rep.mstdb"]
_IN = ["-l", "-i", "list.txt", "-o", "o.txt"]


@pytest.mark.parametrize("args,msg", [
    (["--fast", "--screen"] + _IN, "ERROR: --screen requires --db\n"),
    (["--db", "rep.mstdb", "--screen"] + _IN, "ERROR: --screen needs --fast (a KSSD database)\n"),
    (_DB + ["--screen", "--build"] + _IN, "ERROR: --screen does not go with --build\n"),
    (_DB + ["--screen", "--query"] + _IN, "ERROR: --screen does not go with --query\n"),
    (_DB + ["--screen", "--assign"] + _IN, "ERROR: --screen does not go with --assign\n"),
    (_DB + ["--screen", "--stats"] + _IN, "ERROR: --screen does not go with --stats\n"),
    (_DB + ["--screen", "--append", "more.txt", "-o", "o.txt"], "ERROR: --screen does not go with --append\n"),
    (_DB + ["--screen", "-o", "o.txt"], "ERROR: --screen requires -i <input_file>\n"),
    (_DB + ["--screen", "--min-containment", "1.5"] + _IN, "ERROR: --min-containment must be in [0, 1]\n"),
    (_DB + ["--screen", "--min-containment", "-0.1"] + _IN, "ERROR: --min-containment must be in [0, 1]\n"),
    (_DB + ["--screen", "--min-containment", "nan"] + _IN, "ERROR: --min-containment must be in [0, 1]\n"),
    (_DB + ["--screen", "--min-containment", "half"] + _IN, "ERROR: --min-containment must be in [0, 1]\n"),
    (_DB + ["--screen", "--min-shared", "0"] + _IN, "ERROR: --min-shared must be at least 1\n"),
    (_DB + ["--screen", "--min-unique", "0"] + _IN, "ERROR: --min-unique must be at least 1\n"),
    (_DB + ["--screen", "--min-unique", "-3"] + _IN, "ERROR: --min-unique must be at least 1\n"),
    (_DB + ["--query", "--min-containment", "0.5"] + _IN, "ERROR: --min-containment needs --screen\n"),
    (_DB + ["--query", "--min-shared", "2"] + _IN, "ERROR: --min-shared needs --screen\n"),
    (_DB + ["--assign", "--min-unique", "2"] + _IN, "ERROR: --min-unique needs --screen\n"),
    (["--fast", "--screen-picks", "4"] + _IN, "ERROR: --screen-picks needs --screen\n"),
])
def test_screen_refusals_exit_before_the_gpu(args, msg, tmp_path):
    out = str(tmp_path / "o.txt")
    r = _run("clust-mst", [out if a == "o.txt" else a for a in args])
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr and r.stderr.count("ERROR") == 1
    assert "context" not in r.stderr and "MST RepDB" not in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".summary.tsv")


def test_existing_refusals_keep_their_wording(tmp_path):
    out = str(tmp_path / "o.txt")
    io = ["-l", "-i", "list.txt", "-o", out]
    for args, msg in (
            (_DB + ["--screen", "--build", "--query"] + io, "ERROR: --build, --query, --assign and --stats exclude each other\n"),
            (_DB + io, "ERROR: --db requires one of: --build, --query, --assign, --append, --stats\n"),
            (_DB + ["--screen", "--top-k", "3"] + io, "ERROR: --top-k requires --query\n"),
            (["--fast", "--query", "--screen"] + io, "ERROR: --build / --query / --assign / --stats require --db\n")):
        r = _run("clust-mst", args)
        assert r.returncode == 1 and msg in r.stderr and r.stderr.count("ERROR") == 1, r.stderr


def test_screen_passes_the_flag_checks(tmp_path):
    """a complete --screen line gets through every check of the flags: it ends behind them, where the run asks for a GPU"""
    r = _run("clust-mst", _DB[:2] + [str(tmp_path / "none.mstdb"), "--screen", "--min-containment", "0.1", "--min-shared", "3", "--min-unique", "2",
                                    "--screen-picks", "5", "-i", "contigs.fna", "-o", str(tmp_path / "o.txt")])
    assert r.returncode == 1 and "needs --screen" not in r.stderr and "must be" not in r.stderr and "does not go with" not in r.stderr
    assert not os.path.exists(str(tmp_path / "o.txt"))


@pytest.mark.parametrize("tool", ["clust-greedy", "clust-dbscan", "clust-leiden"])
def test_the_other_tools_do_not_know_the_flags(tool, tmp_path):
    for flag in (["--screen"], ["--min-containment", "0.5"], ["--min-shared", "2"], ["--min-unique", "2"], ["--screen-picks", "1"]):
        r = _run(tool, ["--fast"] + flag + ["-l", "-i", "list.txt", "-o", str(tmp_path / "o.txt")])
        assert r.returncode == 1 and "unknown option %s" % flag[0] in r.stderr and "context" not in r.stderr
