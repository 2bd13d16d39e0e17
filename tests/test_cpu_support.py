"""clust-mst --cluster-support without a GPU: the keep table against direct evaluation, the restatement's own invariants
(tests/refsupport.py), the report writer, the refusals of the command line and the library's exports."""
import os
import subprocess

import numpy as np
import pytest

from tests import reflinkage as RL
from tests import refsupport as R
from tests import support_sets as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
MAX_DENOM = 3000


@pytest.mark.parametrize("k,d", [(21, 0.05), (21, 0.001), (16, 0.2), (31, 0.9), (21, 0.0)])
def test_keep_table_against_direct_evaluation(k, d):
    from rabbittclust_amd import api
    table = api.support_keep_table(k, d, MAX_DENOM)
    assert table.dtype == np.uint32 and table.shape == (MAX_DENOM + 1,) and table[0] == 1
    inv = 1.0 / k
    for den in range(1, MAX_DENOM + 1):
        t = int(table[den])
        assert 1 <= t <= den + 1
        # the entry is the boundary, by the function the restatement calls
        assert t == den + 1 or RL.distance(t, den, k) <= d, den
        assert t == 1 or RL.distance(t - 1, den, k) > d, den
        # and the rule is monotone in c, so the boundary is the least: every count of the row at once, in the same expression order
        c = np.arange(1, den + 1, dtype=np.float64)
        j = c / float(den)
        with np.errstate(divide="ignore"):
            dist = np.where(j == 1.0, 0.0, -inv * np.log((2.0 * j) / (1.0 + j)))
        ok = dist <= d
        assert not (ok[:-1] & ~ok[1:]).any(), den
        assert (int(np.argmax(ok)) + 1 if ok.any() else den + 1) == t, den
    # a short row by the definition itself
    for den in (1, 2, 7, 64, 200, 400):
        assert int(table[den]) == R.need(den, k, d)


def test_keep_table_refusals():
    from rabbittclust_amd import _lib, api
    assert api.CSUPPORT_TABLE_MAX == 1 << 25 and api.CSUPPORT_MAX == 256
    for args, status in (((0, 0.05, 10), _lib.RTC_ERR_ARG), ((21, -0.1, 10), _lib.RTC_ERR_ARG), ((21, float("nan"), 10), _lib.RTC_ERR_ARG)):
        with pytest.raises(_lib.RtcError) as e:
            api.support_keep_table(*args)
        assert e.value.status == status
    out = np.zeros(1, dtype=np.uint32)
    st = _lib.load().rtc_support_keep_table(21, 0.05, api.CSUPPORT_TABLE_MAX, out.ctypes.data)  # one entry too many: refused before it writes
    assert st == _lib.RTC_ERR_UNSUPPORTED


def test_the_restatement_sums_and_recovers():
    sk, groups = SS.constructed()
    lab = R.mst_partition(sk, SS.KMER, SS.THRESHOLD)
    _, members = R.cluster_order(lab)
    assert sorted(map(tuple, members)) == sorted(map(tuple, groups))  # the MST's partition is the clusters as built
    assert sorted(len(m) for m in members) == [1, 1, 3, 4, 4, 5, 6, 7]
    B = 100
    rec, together = R.support(sk, lab, SS.KMER, SS.THRESHOLD, B, 1)
    assert all(sum(r[1:5]) == B for r in rec) and [r[0] for r in rec] == [len(m) for m in members]
    # what the set is there for
    assert any(r[2] > 0 and r[3] > 0 and r[4] > 0 for r in rec) and any(0 < r[1] < B for r in rec)
    seven = [m for m in members if len(m) == 7][0]
    assert len({together[g] for g in seven}) > 1
    lone = [c for c, m in enumerate(members) if len(m) == 1]
    assert all(rec[c] == (1, B, 0, 0, 0, 1) and together[members[c][0]] == 0 for c in lone)  # the empty sketch and the one that shares nothing
    # with every hash kept, every cluster of the MST's own partition is recovered in every replicate
    rec, together = R.support(sk, lab, SS.KMER, SS.THRESHOLD, 3, 1, keep_all=True)
    assert all(r == (len(m), 3, 0, 0, 0, 1) for r, m in zip(rec, members))
    assert all(together[g] == 3 * (len(m) - 1) for m in members for g in m)
    # any labelling: all in one cluster is never split by a crossing edge, every genome its own is never split at all
    rec, _ = R.support(sk, [0] * len(sk), SS.KMER, SS.THRESHOLD, 5, 1)
    assert len(rec) == 1 and rec[0][3] == rec[0][4] == 0 and rec[0][2] == 5 and rec[0][5] >= 8
    rec, together = R.support(sk, list(range(len(sk))), SS.KMER, SS.THRESHOLD, 5, 1)
    assert all(r[2] == r[4] == 0 and r[5] == 1 for r in rec) and not any(together)


def test_the_chain_breaks_where_it_should():
    lab = [0] * 130
    assert R.mst_partition(SS.chain(110), SS.KMER, SS.THRESHOLD) == lab
    (r110,), _ = R.support(SS.chain(110), lab, SS.KMER, SS.THRESHOLD, 64, 1)
    (r116,), _ = R.support(SS.chain(116), lab, SS.KMER, SS.THRESHOLD, 64, 1)
    assert 0 < r110[1] < 64 and r110[3] == r110[4] == 0
    assert r116[5] >= 3 and r116[1] + r116[2] == 64


def test_support_report_text():
    from rabbittclust_amd import api, host
    names = ["a", "b", "c", "d", "e", "f"]
    # the run lists the cluster of c and e first, then the singleton d, then a, b, f; the library orders them by smallest member
    cluster_of = [2, 2, 0, 1, 0, 2]
    rec = np.zeros(3, dtype=api.CSUPPORT_DT)
    rec[0] = (3, 1, 4, 2, 1, 3)    # {a, b, f}: 1 of 8 is 12.5 %, printed 13
    rec[1] = (2, 8, 0, 0, 0, 1)    # {c, e}
    rec[2] = (1, 5, 0, 3, 0, 1)    # {d}: 5 of 8 is 62.5 %, printed 63
    together = [9, 16, 8, 0, 8, 1]
    s, g = host.support_report(names, cluster_of, rec, together, 8)
    assert s == ("cluster\tsize\treplicates\trecovered\tsplit\tmerged\tmixed\tmax_pieces\tsupport\n"
                 "0\t2\t8\t8\t0\t0\t0\t1\t100\n"
                 "1\t1\t8\t5\t0\t3\t0\t1\t63\n"
                 "2\t3\t8\t1\t4\t2\t1\t3\t13\n")
    assert g == ("name\tcluster\ttogether\tfraction\n"
                 "a\t2\t9\t0.562500\n"
                 "b\t2\t16\t1.000000\n"
                 "c\t0\t8\t1.000000\n"
                 "d\t1\t0\t-\n"
                 "e\t0\t8\t1.000000\n"
                 "f\t2\t1\t0.062500\n")
    for count, B, want in ((1, 3, 33), (2, 3, 67), (1, 8, 13), (0, 7, 0), (256, 256, 100), (1, 256, 0), (1, 200, 1)):
        assert R.label(count, B) == want
        one = np.zeros(1, dtype=api.CSUPPORT_DT)
        one[0] = (1, count, 0, B - count, 0, 1)
        assert host.support_report(["x"], [0], one, [0], B)[0].split("\n")[1] == "0\t1\t%d\t%d\t0\t%d\t0\t1\t%d" % (B, count, B - count, want)
    with pytest.raises(ValueError):
        host.support_report(names, [0, 0, 0, 2, 2, 2], rec, together, 8)  # cluster 1 has no member
    with pytest.raises(ValueError):
        host.support_report(names, cluster_of, rec, together, 0)


def _mst(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, "clust-mst")] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("flags,text", [
    (["--cluster-support", "10", "-c", "1000"], "ERROR: --cluster-support does not go with -c/--containment\n"),
    (["--cluster-support", "10", "--inverted-index=false"], "ERROR: --cluster-support does not go with --inverted-index=false\n"),
    (["--cluster-support", "10", "--presketched", "nowhere", "--append", "list.txt"], "ERROR: --cluster-support does not go with --append\n"),
    (["--cluster-support", "10", "--premsted", "nowhere"], "ERROR: --cluster-support does not go with --premsted\n"),
    (["--cluster-support", "10", "--db", "x.db", "--build"], "ERROR: --cluster-support does not go with --db\n"),
    (["--cluster-support", "10", "--dense"], "ERROR: --cluster-support does not go with --dense\n"),
    (["--cluster-support", "10", "--auto-threshold"], "ERROR: --cluster-support does not go with --auto-threshold\n"),
    (["--cluster-support", "10", "--stability"], "ERROR: --cluster-support does not go with --stability\n"),
    (["--cluster-support", "0"], "ERROR: --cluster-support must lie in 1 .. 256, not 0\n"),
    (["--cluster-support", "257"], "ERROR: --cluster-support must lie in 1 .. 256, not 257\n"),
    (["--cluster-support", "-3"], "ERROR: --cluster-support must lie in 1 .. 256, not -3\n"),
    (["--support-seed", "4"], "ERROR: --support-seed needs --cluster-support\n"),
    (["--quality", "--support-seed", "4"], "ERROR: --support-seed needs --cluster-support\n"),
])
def test_refusals_come_before_the_gpu(tmp_path, flags, text):
    out = os.path.join(str(tmp_path), "r.out")
    base = [] if "--append" in flags or "--premsted" in flags else ["-l", "-i", "list.txt"]
    r = _mst(base + ["--fast", "-o", out] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert text in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "--cluster-support" in h.stdout and "--support-seed" in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out, "--cluster-support", "10"], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and "ERROR: unknown option --cluster-support\n" in r.stderr, tool
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_support_calls():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_cluster_support", "rtc_cluster_support_counters", "rtc_support_keep_table", "rtc_components64_dev"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert api.CSUPPORT_DT.itemsize == 24
    for method in ("cluster_support", "cluster_support_counters", "components64"):
        assert hasattr(api.Context, method)
