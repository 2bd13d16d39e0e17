"""clust-mst --pangenome without a GPU: the command line refuses what the flag does not go with before it asks for a GPU, the
restatement (tests/refpangenome.py) satisfies the identities the header states, rtc_pan_growth is the restatement's doubles bit for
bit and the mean over all orders, the constants of rtc_pan.h and of the Python layer agree, and the report writer's columns follow
their rules."""
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import pangenome_sets as PS
from tests import refpangenome as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


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
    r = _mst(base + ["--fast", "-o", out, "--pangenome"] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: --pangenome does not go with {name}\n" in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_refusals_keep_the_order_of_precedence(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    order = [(["-c", "1000"], "-c/--containment"), (["--inverted-index=false"], "--inverted-index=false"), (["--premsted", "nowhere"], "--premsted"),
             (["--db", "x.db", "--build"], "--db"), (["--dense"], "--dense"), (["--auto-threshold"], "--auto-threshold"), (["--stability"], "--stability")]
    for i in range(len(order) - 1):
        flags = [f for fl, _ in order[i:] for f in fl]
        r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out, "--pangenome"] + flags, str(tmp_path))
        assert r.returncode == 1 and f"ERROR: --pangenome does not go with {order[i][1]}\n" in r.stderr, (i, r.stderr)
    # --quality speaks first where it stands beside it
    r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out, "--pangenome", "--quality", "--dense"], str(tmp_path))
    assert r.returncode == 1 and "ERROR: --quality does not go with --dense\n" in r.stderr
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("flags,message", [
    (["--pangenome"], "ERROR: --pangenome needs --fast (KSSD sketches)\n"),
    (["--fast", "--pan-soft", "90"], "ERROR: --pan-soft needs --pangenome\n"),
    (["--fast", "--pan-cloud", "10"], "ERROR: --pan-cloud needs --pangenome\n"),
    (["--fast", "--pan-cloud", "10", "--pan-soft", "90"], "ERROR: --pan-soft needs --pangenome\n"),
    (["--fast", "--pangenome", "--pan-soft", "101"], "ERROR: --pan-soft and --pan-cloud must satisfy 1 <= cloud <= soft <= 100, not soft 101 and cloud 15\n"),
    (["--fast", "--pangenome", "--pan-cloud", "0"], "ERROR: --pan-soft and --pan-cloud must satisfy 1 <= cloud <= soft <= 100, not soft 95 and cloud 0\n"),
    (["--fast", "--pangenome", "--pan-soft", "10", "--pan-cloud", "11"],
     "ERROR: --pan-soft and --pan-cloud must satisfy 1 <= cloud <= soft <= 100, not soft 10 and cloud 11\n"),
    (["--fast", "--pangenome", "--pan-soft", "10"], "ERROR: --pan-soft and --pan-cloud must satisfy 1 <= cloud <= soft <= 100, not soft 10 and cloud 15\n"),
])
def test_what_the_flags_need(tmp_path, flags, message):
    out = os.path.join(str(tmp_path), "r.out")
    r = _mst(["-l", "-i", "list.txt", "-o", out] + flags, str(tmp_path))
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "  --fast --pangenome [--pan-soft P] [--pan-cloud P] (" in h.stdout
    for ext in (".pangenome.tsv", ".pangenome.genomes.tsv", ".pangenome.hist.tsv", ".pangenome.curve.tsv"):
        assert "<output>" + ext in h.stdout, ext
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        for flag in (["--pangenome"], ["--pan-soft", "90"], ["--pan-cloud", "10"]):
            r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out] + flag, cwd=str(tmp_path),
                               capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode == 1 and f"ERROR: unknown option {flag[0]}\n" in r.stderr, (tool, flag)
        hh = subprocess.run([os.path.join(BIN, tool), "-h"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60,
                            env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert "--pangenome" not in hh.stdout and "--pan-" not in hh.stdout, tool
    assert os.listdir(str(tmp_path)) == []


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_the_restatement_satisfies_its_identities(width):
    seen_singleton = seen_empty = seen_out = False
    for name, (sketches, labels) in PS.small_identity_sets().items():
        for soft, cloud in ((95, 15), (100, 1), (50, 50)):
            clusters, hist, genomes = R.pangenome(PS.materialise(sketches, width), labels, soft, cloud)
            assert R.identities(clusters, hist, genomes, labels) == [], name
            assert int(clusters["size"].sum()) == sum(1 for x in labels if x >= 0)
            assert not hist[int(clusters["size"].sum()):].any()
            for g, lab in enumerate(labels):
                if lab < 0:
                    assert not genomes[g:g + 1].view(np.uint8).any()
                    seen_out = True
                else:
                    r = genomes[g]
                    assert int(r["core"]) + int(r["soft"]) + int(r["shell"]) + int(r["cloud"]) == len(sketches[g])
                    seen_empty |= len(sketches[g]) == 0
            seen_singleton |= bool((clusters["size"] == 1).any())
    assert seen_singleton and seen_empty and seen_out


def test_the_restatement_on_a_set_counted_by_hand():
    #            g0          g1   g2            g3         g4 (unclustered)
    sketches = [[1, 2, 3], [], [2, 3, 4, 9], [3, 4, 5], [1, 2, 3]]
    clusters, hist, genomes = R.pangenome([np.asarray(s, dtype=np.uint64) for s in sketches], [4, 4, 4, 4, -1], 70, 30)
    # m = 4; occ: 1 -> 1, 2 -> 2, 3 -> 3, 4 -> 2, 5 -> 1, 9 -> 1.  100 occ >= 280: soft is occ 3; 100 occ < 120: cloud is occ 1
    assert clusters.tolist() == [(10, 6, 0, 1, 2, 3, 3, 4, 0)]
    assert hist.tolist() == [3, 2, 1, 0, 0]
    #                           occ_sum unique core soft shell cloud
    assert genomes.tolist() == [(6, 1, 0, 1, 1, 1, 0), (0, 0, 0, 0, 0, 0, 0), (8, 1, 0, 1, 2, 1, 0), (6, 1, 0, 1, 1, 1, 0), (0, 0, 0, 0, 0, 0, 0)]


# ---- rtc_pan_growth ------------------------------------------------------------------------------------------------------------
def _bits(x):
    return struct.pack("<d", float(x))


def _hist_of(sketches):
    c, h, _ = R.pangenome([np.asarray(s, dtype=np.uint64) for s in sketches], [0] * len(sketches))
    return h[:len(sketches)], c[0]


def _growth_hists():
    rng = np.random.default_rng(3)
    out = [h for h in (_hist_of(PS.thresholds(m)[0])[0] for m in (1, 2, 7, 20))]
    out.append(_hist_of(PS.wide()[0])[0])
    out.append(_hist_of(PS.family(rng, 40, 120, 200, 15, 1 << 21))[0])
    for m in (256, 257, 1000):
        h = np.zeros(m, dtype=np.uint64)
        at = np.unique(np.concatenate([rng.integers(0, m, size=12), [0, m - 1, m // 2]]))
        h[at] = rng.integers(1, 5000, size=len(at))
        out.append(h)
    return out


def test_growth_is_the_restatement_bit_for_bit():
    from rabbittclust_amd import api
    for h in _growth_hists():
        m = len(h)
        j, pan, core = api.pan_growth(h)
        rj, rpan, rcore = R.growth(h)
        assert j.tolist() == rj.tolist() and len(j) == min(m, 256)
        assert [_bits(x) for x in pan] == [_bits(x) for x in rpan], m
        assert [_bits(x) for x in core] == [_bits(x) for x in rcore], m
        for threads in (3, 64):
            tj, tpan, tcore = api.pan_growth(h, threads=threads)
            assert tj.tolist() == j.tolist() and tpan.tobytes() == pan.tobytes() and tcore.tobytes() == core.tobytes()
        total = sum((f + 1) * int(k) for f, k in enumerate(h))
        assert j[0] == 1 and j[-1] == m
        assert pan[-1] == float(int(h.sum())) and core[-1] == float(int(h[m - 1]))  # exactly
        assert abs(pan[0] - total / m) <= 1e-9 * (total / m) and abs(core[0] - total / m) <= 1e-9 * (total / m)
        assert (np.diff(pan) >= 0).all() and (np.diff(core) <= 0).all()
    assert [len(x) for x in api.pan_growth([])] == [0, 0, 0]


def test_growth_points():
    from rabbittclust_amd import api
    for m in (256, 257, 1000):
        j = api.pan_growth(np.ones(m, dtype=np.uint64))[0].tolist()
        want = list(range(1, 257)) if m <= 256 else [1 + (i * (m - 1)) // 255 for i in range(256)]
        assert j == want and len(j) == 256 and j[0] == 1 and j[-1] == m and all(b > a for a, b in zip(j, j[1:]))
    assert api.pan_growth(np.ones(255, dtype=np.uint64))[0].tolist() == list(range(1, 256))
    assert api.PAN_GROWTH_POINTS == 256


def test_growth_is_the_mean_over_all_orders():
    from rabbittclust_amd import api
    rng = np.random.default_rng(11)
    for m in (1, 2, 3, 4, 5, 6):
        sets = [set(rng.choice(14, size=int(rng.integers(0, 10)), replace=False).tolist()) for _ in range(m)]
        if m >= 3:
            sets[1] |= {100, 101}
            sets = [s | {200} for s in sets]  # a core hash
        hist, _ = _hist_of([sorted(s) for s in sets])
        pan_sum, core_sum, orders = [0] * m, [0] * m, 0
        for order in itertools.permutations(range(m)):
            union, inter = set(), None
            for j, g in enumerate(order):
                union |= sets[g]
                inter = set(sets[g]) if inter is None else inter & sets[g]
                pan_sum[j] += len(union)
                core_sum[j] += len(inter)
            orders += 1
        j, pan, core = api.pan_growth(hist)
        assert j.tolist() == list(range(1, m + 1))
        for k in range(m):
            assert abs(pan[k] - pan_sum[k] / orders) <= 1e-9 * max(1.0, pan_sum[k] / orders), (m, k)
            assert abs(core[k] - core_sum[k] / orders) <= 1e-9 * max(1.0, core_sum[k] / orders), (m, k)


# ---- constants and report ------------------------------------------------------------------------------------------------------
def test_path_boundaries_are_the_headers():
    from rabbittclust_amd import api
    text = open(os.path.join(ROOT, "rabbittclust_amd", "csrc", "rtc_pan.h")).read()
    got = {k: int(v, 0) for k, v in re.findall(r"(PAN_[A-Z0-9_]+) = (0x[0-9A-Fa-f]+|\d+)", text)}
    for name in ("PAN_WAVE_RECORDS", "PAN_WAVE_SLOTS", "PAN_WAVE_HIST", "PAN_BLOCK_RECORDS", "PAN_BLOCK_SLOTS", "PAN_BLOCK_HIST", "PAN_GLOBAL_LOG2_MIN",
                 "PAN_GLOBAL_WGS_PER_CU", "PAN_WAVE_WGS_PER_CU", "PAN_BLOCK_WGS_PER_CU", "PAN_SWEEP_BINS", "PAN_SLOT_BYTES", "PAN_MEMBER_BYTES", "PAN_CLUSTER_BYTES", "PAN_MULT", "PAN_GROWTH_POINTS"):
        assert got[name] == getattr(api, name), name
    assert "PAN_EMPTY = ~0ull" in text and api.PAN_EMPTY == (1 << 64) - 1
    assert (api.PAN_PATH_WAVE, api.PAN_PATH_BLOCK, api.PAN_PATH_GLOBAL) == (1, 2, 4)
    # no table is more than half full; the LDS of a CU (160 KiB) holds the workgroups the header counts
    assert api.PAN_WAVE_SLOTS >= 2 * api.PAN_WAVE_RECORDS and api.PAN_BLOCK_SLOTS >= 2 * api.PAN_BLOCK_RECORDS
    wave = api.PAN_SLOT_BYTES * api.PAN_WAVE_SLOTS + 4 * api.PAN_WAVE_HIST + 64
    block = api.PAN_SLOT_BYTES * api.PAN_BLOCK_SLOTS + 4 * api.PAN_BLOCK_HIST + 64
    assert got["PAN_WAVE_WGS_PER_CU"] * wave <= 160 * 1024 < (got["PAN_WAVE_WGS_PER_CU"] + 1) * wave
    assert got["PAN_BLOCK_WGS_PER_CU"] * block <= 160 * 1024 < (got["PAN_BLOCK_WGS_PER_CU"] + 1) * block
    assert [api.pan_table_log2(x) for x in (0, 512, 2048, 2049, 4096, 4097, 10 ** 6)] == [None, None, None, 13, 13, 14, 21]
    assert [api.pan_table_log2(x, True) for x in (0, 1, 128, 129, 2048)] == [8, 8, 8, 9, 12]
    assert api.pan_cluster_bytes(2049, 3) == 12 * 8192 + 56 * 3 + 48 and api.pan_cluster_bytes(100, 7) == 56 * 7 + 48
    assert api.pan_slot(0, 13) == 0 and api.pan_slot(1, 8) == api.PAN_MULT >> 56 and api.pan_slot(api.PAN_EMPTY - 1, 10) < 1024
    assert PS.widen([0, 5, PS.ONES32]).tolist() == [0, (5 << 32) | ((5 * 2654435761) & 0xFFFFFFFF), api.PAN_EMPTY]


def test_report_columns_from_hand_made_records():
    from rabbittclust_amd import api, host
    # g0 and g2 hold the same three hashes and g1, of their cluster, holds nothing; g3 is alone
    sketches = [np.asarray(s, dtype=np.uint64) for s in ([1, 2, 3], [], [1, 2, 3], [7, 8])]
    cluster_of = [1, 1, 1, 0]  # as the result file numbers them: the singleton first
    clusters, hist, genomes = R.pangenome(sketches, cluster_of)
    assert clusters.dtype == api.PAN_DT and genomes.dtype == api.PAN_GENOME_DT
    assert clusters["size"].tolist() == [3, 1]  # the library's order: by smallest member
    names = ["g%d.fna" % g for g in range(4)]
    pan, gen, hs, curve = host.pangenome_report(names, cluster_of, clusters, hist, genomes)
    assert pan.split("\n") == [
        "cluster\tsize\thashes\tpan\tcore\tsoft_core\tshell\tcloud\tsingletons\tcore_share\tnew_per_genome\tcentre",
        "0\t1\t2\t2\t2\t0\t0\t0\t2\t1.000000\t2.000000\tg3.fna",
        "1\t3\t6\t3\t0\t0\t3\t0\t0\t0.000000\t0.000000\tg0.fna",  # g0 and g2 tie at occ_sum 6: the smaller index
        ""]
    assert gen.split("\n") == [
        "name\tcluster\thashes\tunique\tcore\tsoft_core\tshell\tcloud\ttypicality",
        "g0.fna\t1\t3\t0\t0\t0\t3\t0\t0.666667",
        "g1.fna\t1\t0\t0\t0\t0\t0\t0\t-",
        "g2.fna\t1\t3\t0\t0\t0\t3\t0\t0.666667",
        "g3.fna\t0\t2\t2\t2\t0\t0\t0\t1.000000",
        ""]
    assert hs.split("\n") == ["cluster\tf\tcount", "0\t1\t2", "1\t2\t3", ""]
    assert curve.split("\n") == ["cluster\tj\tpan\tcore", "1\t1\t2.000000\t2.000000", "1\t2\t3.000000\t1.000000", "1\t3\t3.000000\t0.000000", ""]
    # new_per_genome is the closed form's last step
    big, big_rec = _hist_of(PS.family(np.random.default_rng(2), 40, 60, 90, 7, 1 << 21))
    j, p, c = api.pan_growth(big)
    assert int(big[0]) >= 280 and abs((p[-1] - p[-2]) - int(big[0]) / len(big)) < 1e-9
    with pytest.raises(ValueError):  # the reports are of a run's clusters: no genome is outside them
        host.pangenome_report(names, [1, 1, -1, 0], clusters, hist, genomes)
    with pytest.raises(ValueError):  # records of other clusters
        host.pangenome_report(names, [0, 0, 0, 1], clusters[::-1].copy(), hist, genomes)


def test_library_exports_the_pangenome_calls():
    from rabbittclust_amd import _lib
    lib = _lib.load()
    for name in ("rtc_pangenome", "rtc_pangenome_counters", "rtc_pangenome_phases", "rtc_pangenome_last_path", "rtc_pan_growth"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
