"""clust-dbscan --db without a GPU: the placement rule (tests/refdbscan_assign.py) held against the reference's compiled
KssdDBSCAN by leaving one point out, the model file parsed from its documented layout, --stats, and the flag errors, which
exit before any GPU is asked for."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refdbscan_assign as A
from tests import reflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-dbscan")
K, EPS, MIN_PTS = 21, 0.04, 5


@pytest.mark.parametrize("use64", [False, True])
def test_leave_one_out_against_the_reference(use64):
    """S = T without p, p placed last: where adding p moves no core flag of S and p is no core point, the reference labels S
    alone and inside S + [p] alike, and gives p the restated placement's label."""
    L = reflib.ref_dbscan()
    if L is None:  # a restatement in its place would anchor nothing
        pytest.fail("oracle/_ref/libref_dbscan.so is not built: this test needs the reference's compiled KssdDBSCAN")

    def reference(points):
        return reflib.kssd_dbscan(L, points, use64, EPS, MIN_PTS, K)[0]

    def core_flags(points):
        return [len(x) + 1 >= MIN_PTS for x in R.neighbour_lists(points, EPS, K, use64)]
    T = A.satellite_set(1, use64)
    checked = {"cluster": 0, "novel": 0}
    for p in range(len(T)):
        S = [x for i, x in enumerate(T) if i != p]
        both = S + [T[p]]
        core_s, core_both = core_flags(S), core_flags(both)
        if core_both[:-1] != core_s or core_both[-1]:
            continue
        lab_s, lab_both = reference(S), reference(both)
        assert np.array_equal(lab_both[:-1], lab_s), p
        rec = A.place_kssd(S, lab_s, core_s, T[p], EPS, MIN_PTS, K, use64)
        assert rec[0] == int(lab_both[-1]), (p, rec, int(lab_both[-1]))
        assert rec[2] == len(R.neighbour_lists(both, EPS, K, use64)[-1]) and rec[7] == 0
        checked["cluster" if rec[0] >= 0 else "novel"] += 1
    assert checked["cluster"] >= 5 and checked["novel"] >= 5 and sum(checked.values()) >= 20, checked


def test_restated_rule_on_hand_made_points():
    a, b = np.arange(0, 100), np.arange(1000, 1100)
    model = [a, a + 1, a + 2, b, b + 1, b + 2, np.arange(5000, 5100)]
    labels, core = [0, 0, 0, 1, 1, 1, -1], [1, 1, 1, 1, 1, 1, 0]
    bridge = np.concatenate([a[:60], b[:60]])  # Jaccard 60 / 160 with both clusters' points
    rec = A.place_kssd(model, labels, core, bridge, 0.05, 3, K, False)
    assert rec[:4] == (0, 1, 6, 6) and rec[4] == 0 and rec[5:7] == (60, 160) and rec[7] == 1
    assert A.place_kssd(model, labels, core, np.arange(5000, 5100), 0.05, 3, K, False) == (-1, -1, 1, 0, 6, 100, 100, 0)
    assert A.place_kssd(model, labels, core, np.arange(9000, 9100), 0.05, 3, K, False) == (-1, -1, 0, 0, A.NONE, 0, 0, 0)
    assert A.place_kssd(model, labels, core, np.zeros(0, dtype=np.int64), 0.05, 1, K, True) == (-1, -1, 0, 0, A.NONE, 0, 0, 1)
    # MinHash: the core rule counts the neighbours alone, and the counts are the union-truncated ones
    rec = A.place_mash(model, labels, core, a, 0.05, 3, K, 100)
    assert rec[:5] == (0, 0, 3, 3, 0) and rec[5:7] == (100, 100) and rec[7] == 1
    assert A.place_mash(model, labels, core, a, 0.05, 4, K, 100)[7] == 0


# ---- the command line ---------------------------------------------------------------------------------------------------
def _run(args, cwd=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)


def _model_bytes(kind=0, width=4, max_posting=0):
    """a model file written from the layout INTEGRATION.md documents"""
    sk = [np.arange(10, 20), np.arange(12, 22), np.zeros(0, dtype=np.int64)]
    dt = "<u8" if width == 8 else "<u4"
    out = [A.MAGIC, struct.pack("<12i", 1, kind, width, 1, 21, 11 if kind == 0 else 0, 6 if kind == 0 else 0, 3 if kind == 0 else 0,
                               0 if kind == 0 else 1000, 2, max_posting, 1),
           struct.pack("<QQd", 10000, 3, 0.05), struct.pack("<3i", 0, 0, -1), bytes([1, 1, 0])]
    for i in range(3):
        for text in ("g%d.fna" % i, "seq%d" % i, "a comment"):
            out.append(struct.pack("<I", len(text)) + text.encode())
        out.append(struct.pack("<QQ", 500 + i, 900 + i))
    out.append(struct.pack("<3I", *[len(s) for s in sk]))
    out += [np.asarray(s, dtype=dt).tobytes() for s in sk]
    return b"".join(out)


def test_model_layout_round_trip_and_stats(tmp_path):
    from rabbittclust_amd import host
    for kind, width in ((0, 4), (0, 8), (1, 8)):
        blob = _model_bytes(kind, width)
        m = A.parse_model(blob)
        assert m["n"] == 3 and m["labels"].tolist() == [0, 0, -1] and m["sketches"][1].tolist() == list(range(12, 22))
        assert m["genomes"][2] == {"file": "g2.fna", "name": "seq2", "comment": "a comment", "length": 502, "total_length": 902}
        path = os.path.join(str(tmp_path), "m%d%d.db" % (kind, width))
        open(path, "wb").write(blob)
        # the host library reads the file and writes the same bytes back, through a temporary name
        again = path + ".again"
        assert host.load().rtch_dbscan_model_resave(path.encode(), again.encode()) == 0
        assert open(again, "rb").read() == blob and not os.path.exists(again + ".tmp")
        r = _run(["--db", path, "--stats"])
        assert r.returncode == 0, r.stderr
        for line in ("Kind:        %s" % ("KSSD" if kind == 0 else "MinHash"), "Hash width:  %d" % width, "Kmer size:   21", "Eps:         0.05",
                     "MinPts:      2", "Genomes:     3", "Clusters:    1", "Noise:       1", "Core points: 2"):
            assert line in r.stdout, (line, r.stdout)
        assert ("Sketch size: 1000" in r.stdout) == (kind == 1) and ("Drlevel:     3" in r.stdout) == (kind == 0)
        assert "context" not in r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--fast", "--db", "m.db", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --db requires exactly one of --build, --assign, --stats"),
    (["--fast", "--db", "m.db", "--build", "--assign", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --db requires exactly one of --build, --assign, --stats"),
    (["--fast", "--build", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --build / --assign / --stats require --db"),
    (["--fast", "--db", "m.db", "--build", "--max-posting", "5", "-l", "-i", "list.txt", "-o", "o.txt"],
     "ERROR: --build does not go with --max-posting"),
    (["--db", "m.db", "--build", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: clust-dbscan requires --fast option"),
    (["--db", "missing.db", "--stats"], "ERROR: --db missing.db: cannot open"),
    (["--db", "missing.db", "--assign", "-l", "-i", "list.txt", "-o", "o.txt"], "ERROR: --db missing.db: cannot open"),
    (["--fast", "--db", "m.db", "--query", "-l", "-i", "list.txt", "-o", "o.txt"], "unknown option --query"),
    (["--fast", "--db", "m.db", "--assign", "--top-k", "3", "-l", "-i", "list.txt", "-o", "o.txt"], "unknown option --top-k"),
    (["--fast", "--db", "m.db", "--append", "list.txt", "-o", "o.txt"], "ERROR: --append not supported for DBSCAN clustering"),
])
def test_flag_errors_before_the_gpu(args, msg, tmp_path):
    r = _run(args, cwd=str(tmp_path))
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


def test_foreign_truncated_and_mismatched_models(tmp_path):
    tmp = str(tmp_path)

    def write(name, blob):
        open(os.path.join(tmp, name), "wb").write(blob)
        return name
    good = _model_bytes(0, 4)
    assign = ["--assign", "-l", "-i", "list.txt", "-o", "o.tsv"]
    cases = [
        (["--db", write("foreign.db", b"KSMSTST01" + good[9:]), "--stats"], "is not a clust-dbscan model"),
        (["--db", write("short.db", good[:-5]), "--stats"], "is truncated"),
        (["--db", write("head.db", good[:30]), "--stats"], "is truncated"),
        (["--db", write("long.db", good + b"x"), "--stats"], "bytes after its end"),
        (["--db", "short.db"] + assign, "is truncated"),
        (["--db", write("v2.db", good[:8] + struct.pack("<i", 2) + good[12:]), "--stats"], "version 2"),
        (["--minhash", "--db", write("kssd.db", good)] + assign, "ERROR: --assign: --minhash given, but kssd.db is a KSSD model"),
        (["--fast", "--db", write("mh.db", _model_bytes(1, 8))] + assign, "ERROR: --assign: --fast given, but mh.db is a MinHash model"),
        (["--db", write("mp.db", _model_bytes(0, 4, max_posting=7))] + assign, "was built with --max-posting 7"),
        (["--db", "kssd.db", "--assign", "-o", "o.tsv"], "ERROR: --assign requires -i <input_file>"),
    ]
    for args, msg in cases:
        r = _run(args, cwd=tmp)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert "context" not in r.stderr
    with pytest.raises(ValueError):
        A.parse_model(good[:-5])
    with pytest.raises(ValueError):
        A.parse_model(b"KSMSTST01" + good[9:])


def test_help_names_the_model_flags():
    r = _run(["-h"])
    assert r.returncode == 0
    for flag in ("--db", "--build", "--assign", "--stats", "--eps", "--minpts", "--max-posting", "--minhash", "--eps-sweep", "--kdist"):
        assert flag in r.stdout, flag
