"""clust-dbscan --eps-sweep / --kdist without a GPU: the exported symbols, the help text, the malformed lists (which exit before
any GPU is asked for), the k-distance restatement (tests/refkdist.py) tied to the reference's own predicate
(tests/refdbscan.py), and the preconditions the GPU sweep tests rely on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refkdist as KD
from tests import sweep_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
LIB = os.path.join(ROOT, "rabbittclust_amd", "librtclust_hip.so")


def test_library_exports_the_sweep():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "rtc_dbscan_sweep" in names and "rtc_dbscan_sweep_counters" in names
    from rabbittclust_amd import _lib
    assert "rtc_dbscan_sweep" in _lib.SIGNATURES and "rtc_dbscan_sweep_counters" in _lib.SIGNATURES
    from rabbittclust_amd import api
    assert api.KDIST_DT.itemsize == 16 == ctypes.sizeof(ctypes.c_uint32) * 4


def _run(tool, args):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        pytest.fail(tool + " missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)


def test_help_names_the_sweep_options():
    r = _run("clust-dbscan", ["-h"])
    assert r.returncode == 0 and "--eps-sweep" in r.stdout and "--kdist" in r.stdout
    for tool in ("clust-mst", "clust-greedy"):
        h = _run(tool, ["-h"])
        assert h.returncode == 0 and "--eps-sweep" not in h.stdout and "--kdist" not in h.stdout


@pytest.mark.parametrize("value,msg", [
    ("0.01,,0.02", "empty element"),
    (",0.01", "empty element"),
    ("0.01,", "empty element"),
    ("", "empty element"),
    ("0.01,0", "must be > 0"),
    ("0.01,-0.5", "must be > 0"),
    ("0.01,abc", "must be > 0"),
    (",".join(["0.01"] * 33), "at most 32 values"),
])
def test_malformed_lists_exit_before_the_gpu(value, msg):
    r = _run("clust-dbscan", ["--fast", "-l", "-i", "list.txt", "-o", "o.txt", "--eps-sweep", value])
    assert r.returncode == 1, r.stderr
    assert "--eps-sweep" in r.stderr and msg in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


@pytest.mark.parametrize("tool", ["clust-mst", "clust-greedy"])
@pytest.mark.parametrize("flag", [["--eps-sweep", "0.01,0.02"], ["--kdist"]])
def test_other_tools_do_not_learn_the_flags(tool, flag):
    r = _run(tool, ["-l", "-i", "list.txt", "-o", "o.txt"] + flag)
    assert r.returncode == 1 and "unknown option " + flag[0] in r.stderr


def _is_core(nbrs, p, min_pts):
    return len(nbrs[p]) + 1 >= min_pts


@pytest.mark.parametrize("seed", range(1, 4))
@pytest.mark.parametrize("max_posting", [0, 5])
def test_kdist_restatement_agrees_with_the_reference_predicate(seed, max_posting):
    """p's k-distance d is where p becomes a core point of the reference's own neighbour relation: core at eps = d (1 + 1e-6),
    not core at eps = d (1 - 1e-6).  1e-6 relative is far above the predicate's 1e-12 slack and double rounding at these
    sketch sizes, and the relation is monotone in eps, so both checks hold whatever lies between."""
    sk = S.family_sets(seed, use64=False)
    nb_cache = {}

    def nbrs(eps):
        if eps not in nb_cache:
            nb_cache[eps] = R.neighbour_lists(sk, eps, S.KMER, False, max_posting)
        return nb_cache[eps]
    checked = with_none = 0
    for min_pts in (2, 3, 5):
        for p, (common, size_p, size_q, q) in enumerate(KD.kdist(sk, min_pts, False, max_posting)):
            if q == KD.NONE:
                with_none += 1
                # fewer than k candidates: p is never core, however large eps (within the supported range)
                assert not _is_core(nbrs(1.0), p, min_pts)
                continue
            d = KD.distance(common, size_p, size_q, S.KMER)
            assert _is_core(nbrs(d * (1 + 1e-6) if d > 0 else 1e-9), p, min_pts), (p, min_pts, d)
            if d > 0:
                assert not _is_core(nbrs(d * (1 - 1e-6)), p, min_pts), (p, min_pts, d)
            checked += 1
    assert checked > 50 and with_none > 0


def test_kdist_restatement_hand_cases():
    a = np.arange(100, dtype=np.uint32)
    sk = [a, np.concatenate([a[:80], np.arange(1000, 1020, dtype=np.uint32)]), np.concatenate([a[:50], np.arange(2000, 2050, dtype=np.uint32)]),
          np.arange(5000, 5010, dtype=np.uint32), np.zeros(0, dtype=np.uint32), a.copy()]
    got = KD.kdist(sk, 2, False)
    assert got[0] == (100, 100, 100, 5) and got[5] == (100, 100, 100, 0)  # j = 1, the identical sketch
    assert got[1] == (80, 100, 100, 0)  # 0 and 5 tie at 80 / 120: the lower index
    assert got[3] == (0, 10, 0, KD.NONE) and got[4] == (0, 0, 0, KD.NONE)
    assert KD.kdist(sk, 3, False)[1] == (80, 100, 100, 5)
    assert KD.kdist(sk, 1, False)[2] == (100, 100, 100, 2) and KD.kdist(sk, 0, False)[4] == (0, 0, 0, 4)
    # u64: the empty sketches see each other at j = 1, the lower index first
    e = np.zeros(0, dtype=np.uint64)
    sk64 = [e, a.astype(np.uint64), e, e]
    assert KD.kdist(sk64, 2, True) == [(0, 0, 0, 2), (0, 100, 0, KD.NONE), (0, 0, 0, 0), (0, 0, 0, 0)]
    assert KD.kdist(sk64, 3, True)[0] == (0, 0, 0, 3) and KD.kdist(sk64, 4, True)[0] == (0, 0, 0, KD.NONE)
    assert KD.distance(0, 0, 0, 21) == 0.0 and KD.distance(100, 100, 100, 21) == 0.0
    # --max-posting: the hash every sketch holds no longer links anything
    sk2 = [np.array([1, 5], dtype=np.uint32), np.array([1, 6], dtype=np.uint32), np.array([1, 7], dtype=np.uint32)]
    assert KD.kdist(sk2, 2, False)[0] == (1, 2, 2, 1) and KD.kdist(sk2, 2, False, max_posting=2)[0] == (0, 2, 0, KD.NONE)


@pytest.mark.parametrize("use64,n_empty", [(False, 0), (False, 2), (True, 3)])
def test_sweep_sets_cut_differently_at_the_chosen_eps(use64, n_empty):
    """What tests/test_gpu_dbscan_sweep.py asserts before it touches the GPU, here for one seed on the reference restatement
    alone: the eps list gives at least three distinct label vectors; noise where it can exist (minPts >= 2: at minPts 1 every
    point is a core point) and a border point where one can exist (minPts >= 3: with a neighbour a point is core at minPts 2)."""
    sk = S.family_sets(1, use64, n_empty)
    for min_pts in (1, 2, 5):
        labs, cores = [], []
        for eps in S.EPS:
            nb = R.neighbour_lists(sk, eps, S.KMER, use64)
            lab, core = R.closed_form(nb, min_pts)
            assert lab == R.labels_of(sk, eps, min_pts, S.KMER, use64).tolist()
            labs.append(lab)
            cores.append(core)
        distinct, noise, border = S.describe(labs, cores)
        assert distinct >= 3
        assert noise == (min_pts >= 2)
        assert border == (min_pts >= 3)
