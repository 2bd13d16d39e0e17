"""clust-mst --nj-support without a GPU: the mask's known answers, the restatement's splits (tests/refnjsupport.py), one constructed
cluster, the labelled Newick writer, the refusals of the command line and the library's exports."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import nj_support_sets as NS
from tests import refnj as R
from tests import refnjsupport as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
NONE = R.NONE

KNOWN_MIX = {0: 0xE220A8397B1DCDAF, 1: 0x910A2DEC89025CC1, 0xFFFFFFFF: 0x73B13BA2AFF181C0}
KNOWN_WORD = {(0, 0, 0): 0xA706DD2F4D197E6F, (12345, 7, 1): 0x3717D7091474E1B6}


def test_known_answers_of_the_mask():
    from rabbittclust_amd import api
    for x, want in KNOWN_MIX.items():
        assert RS.mix(x) == want
    for (h, seed, w), want in KNOWN_WORD.items():
        assert RS.word(h, seed, w) == want
        assert api.jackknife_word(h, seed, w) == want
    # the library and the restatement agree beyond them: the seed and the word add modulo 2^64, the hash is taken whole
    rng = np.random.default_rng(3)
    for _ in range(200):
        h, seed, w = int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 4))
        assert api.jackknife_word(h, seed, w) == RS.word(h, seed, w)
    assert api.jackknife_word(5, (1 << 64) - 1, 1) == RS.word(5, 0, 0)
    # replicate r reads bit r % 64 of word r / 64
    assert RS.kept(12345, 7, 64 + 1) == bool(KNOWN_WORD[(12345, 7, 1)] >> 1 & 1)


def _rec(rows):
    return [(a, b, c, 0.0, 0.0, 0.0) for a, b, c in rows]


def test_split_extraction_on_hand_written_records():
    # m <= 3: no inner branch
    assert RS.record_splits([], 1) == []
    assert RS.record_splits(_rec([(0, 1, NONE)]), 2) == [None]
    assert RS.record_splits(_rec([(0, 1, 2)]), 3) == [None]
    # m = 4: one split, whichever side the record joins
    assert RS.record_splits(_rec([(2, 3, NONE), (0, 1, 2)]), 4) == [frozenset({2, 3}), None]
    assert RS.record_splits(_rec([(0, 1, NONE), (0, 2, 3)]), 4) == [frozenset({2, 3}), None]
    assert RS.record_splits(_rec([(0, 2, NONE), (0, 1, 3)]), 4) == [frozenset({1, 3}), None]
    # m = 5, a caterpillar grown from leaf 0: the sides away from it
    assert RS.record_splits(_rec([(0, 1, NONE), (0, 2, NONE), (0, 3, 4)]), 5) == [frozenset({2, 3, 4}), frozenset({3, 4}), None]
    # m = 5, balanced: two cherries and a leaf at the closing node
    assert RS.record_splits(_rec([(1, 2, NONE), (3, 4, NONE), (0, 1, 3)]), 5) == [frozenset({1, 2}), frozenset({3, 4}), None]
    # a node named by its first child: the second record joins the node {1, 2} (named 1) with 3
    assert RS.record_splits(_rec([(1, 2, NONE), (1, 3, NONE), (0, 1, 4)]), 5) == [frozenset({1, 2}), frozenset({1, 2, 3}), None]


def test_constructed_cluster_by_the_restatement():
    """two subfamilies of four: the branch between them is in all 64 replicates, one inside a subfamily is not"""
    B = 64
    sk = NS.constructed()
    assert len(sk) == 8 and all(150 <= len(s) <= 202 for s in sk)
    main, support = RS.support_of(sk, 21, B, 0)
    splits = RS.record_splits(main, 8)
    assert len(main) == 6 and splits[-1] is None and support[-1] == 0
    between = frozenset({4, 5, 6, 7})
    assert between in splits and support[splits.index(between)] == B
    inside = [support[e] for e, s in enumerate(splits) if s is not None and s != between]
    assert len(inside) == 4 and all(s <= frozenset({1, 2, 3}) or s <= between for s in splits[:-1])
    assert min(inside) < B
    # a replicate's sizes are about half: a delete-half jackknife
    kept = sum(len(s) for s in RS.replicate_sets(sk, 0, 0))
    total = sum(len(s) for s in sk)
    assert 0.4 * total < kept < 0.6 * total
    # another seed is another jackknife
    assert RS.replicate_sets(sk, 1, 0) != RS.replicate_sets(sk, 0, 0)


def _records(rows):
    from rabbittclust_amd import api
    out = np.zeros(len(rows), dtype=api.NJOIN_DT)
    for e, (a, b, c, la, lb, lc) in enumerate(rows):
        out[e] = (a, b, c, 0, la, lb, lc)
    return out


def _strip(text):
    return re.sub(r"\)\d+", ")", text)


def test_support_newick_writer():
    from rabbittclust_amd import host
    labels = [f"g{v}" for v in range(10)]
    rec = _records([(3, 7, NONE, 1.5, -0.25, 0.0), (2, 9, NONE, 1.0, 2.0, 0.0), (2, 3, 5, 0.5, 0.75, 4.0)])
    got = host.nj_support_newick(labels, [9, 2, 3, 5, 7], rec, [3, 10, 0], 10)
    assert got == "((g2:1.000000,g9:2.000000)100:0.500000,(g3:1.500000,g7:-0.250000)30:0.750000,g5:4.000000);"
    assert _strip(got) == host.nj_newick(labels, [9, 2, 3, 5, 7], rec)
    # percent, half up, in integers: 1 of 3 is 33, 2 of 3 is 67, 1 of 8 is 13 (12.5), 0 is 0
    for count, B, want in ((1, 3, 33), (2, 3, 67), (1, 8, 13), (0, 7, 0), (256, 256, 100), (1, 256, 0), (1, 200, 1)):
        assert RS.label(count, B) == want
        text = host.nj_support_newick(labels, [0, 1, 2, 3], _records([(2, 3, NONE, 1.0, 1.0, 0.0), (0, 1, 2, 1.0, 1.0, 1.0)]), [count, 0], B)
        assert text == "(g0:1.000000,g1:1.000000,(g2:1.000000,g3:1.000000)%d:1.000000);" % want
    # trees of three members or fewer carry nothing
    assert host.nj_support_newick(labels, [4], _records([]), [], 5) == "g4;"
    assert host.nj_support_newick(labels, [1, 6], _records([(1, 6, NONE, 0.5, 0.25, 0.0)]), [0], 5) == "(g1:0.500000,g6:0.250000);"
    assert host.nj_support_newick(labels, [0, 1, 2], _records([(0, 1, 2, 1.0, 2.0, 3.0)]), [0], 5) == "(g0:1.000000,g1:2.000000,g2:3.000000);"


def _mst(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([os.path.join(BIN, "clust-mst")] + args, cwd=cwd, capture_output=True, text=True, timeout=60, env=env)


@pytest.mark.parametrize("flags,flag", [
    (["--nj-support", "10"], "--nj-support"),
    (["--nj-tree", "--nj-support", "0"], "--nj-support"),
    (["--nj-all", "--nj-support", "257"], "--nj-support"),
    (["--nj-tree", "--nj-support", "-3"], "--nj-support"),
    (["--nj-tree", "--nj-seed", "4"], "--nj-seed"),
    (["--nj-seed", "4"], "--nj-seed"),
])
def test_refusals_come_before_the_gpu(tmp_path, flags, flag):
    out = os.path.join(str(tmp_path), "r.out")
    r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out] + flags, str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert f"ERROR: {flag} " in r.stderr
    assert "context" not in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_the_conflicts_of_nj_tree_hold_with_support(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    r = _mst(["-l", "-i", "list.txt", "--fast", "-o", out, "--nj-tree", "--nj-support", "10", "--dense"], str(tmp_path))
    assert r.returncode == 1 and "ERROR: --nj-tree does not go with --dense\n" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_help_and_the_other_commands(tmp_path):
    out = os.path.join(str(tmp_path), "r.out")
    h = _mst(["-h"], str(tmp_path))
    assert h.returncode == 0 and "--nj-support" in h.stdout and "--nj-seed" in h.stdout
    for tool in ("clust-greedy", "clust-dbscan", "clust-leiden"):
        r = subprocess.run([os.path.join(BIN, tool), "--fast", "-l", "-i", "list.txt", "-o", out, "--nj-support", "10"], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1 and "ERROR: unknown option --nj-support\n" in r.stderr, tool
    assert os.listdir(str(tmp_path)) == []


def test_library_exports_the_support_calls():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_nj_support", "rtc_nj_support_counters", "rtc_jackknife_word", "rtc_jackknife_pairs_dev"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert api.JK_LDS_ELEMS == 1024 and api.NJ_SUPPORT_MAX == 256
