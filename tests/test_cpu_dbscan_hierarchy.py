"""clust-dbscan --hierarchy without a GPU: the exported symbols, the help text and the two flag errors (which exit before any
GPU is asked for); the restatement tests/refhier.py held to the reference's own compiled KssdDBSCAN through its cut property
(oracle/_ref via tests/reflib.py, as tests/test_cpu_refpin.py does); and the host-only rtc_hierarchy_cut / rtc_hierarchy_flat
through ctypes against the restatement."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from tests import refdbscan as R
from tests import refhier as RH
from tests import reflib, refpin_cases as P
from tests import sweep_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
LIB = os.path.join(ROOT, "rabbittclust_amd", "librtclust_hip.so")

EPS_MAX = 0.12
# candidates for the cut; a set keeps those whose t(eps) stays clear of every j (see _clear_eps), at least 8 of them
EPS_CUTS = [0.002, 0.005, 0.008, 0.011, 0.014, 0.02, 0.025, 0.03, 0.04, 0.05, 0.06, 0.08, 0.1, 0.12]
MARGIN = 1e-9


def _clear_eps(forest, core, all_js=()):
    """The exact order of j and the double predicate agree while no j lies within MARGIN of t(eps): rounding in the predicate
    is ~1e-16 relative and its slack 1e-12, both far below 1e-9."""
    out = [e for e in EPS_CUTS if RH.min_margin(forest, core, [e], S.KMER) > MARGIN
           and all(abs(j - R.jaccard_min(e, S.KMER)) > MARGIN for j in all_js)]
    assert len(out) >= 8, out
    return out


def _arrays(forest, core):
    from rabbittclust_amd import api
    f = np.array([tuple(e) for e in forest], dtype=api.HEDGE_DT) if forest else np.zeros(0, dtype=api.HEDGE_DT)
    c = np.array([tuple(x) for x in core], dtype=api.KDIST_DT) if core else np.zeros(0, dtype=api.KDIST_DT)
    return f, c


def test_library_exports_the_hierarchy():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"rtc_dbscan_hierarchy", "rtc_dbscan_sweep_hierarchy", "rtc_dbscan_hierarchy_counters", "rtc_hierarchy_cut", "rtc_hierarchy_flat"}
    assert want <= names
    from rabbittclust_amd import _lib, api
    assert want <= set(_lib.SIGNATURES)
    assert api.HEDGE_DT.itemsize == 20 == ctypes.sizeof(ctypes.c_uint32) * 5


def _run(tool, args):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        pytest.fail(tool + " missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, env=env)


def test_help_names_the_hierarchy_options():
    r = _run("clust-dbscan", ["-h"])
    assert r.returncode == 0 and "--hierarchy" in r.stdout and "--min-cluster-size" in r.stdout
    for tool in ("clust-mst", "clust-greedy"):
        h = _run(tool, ["-h"])
        assert h.returncode == 0 and "--hierarchy" not in h.stdout
        bad = _run(tool, ["-l", "-i", "list.txt", "-o", "o.txt", "--hierarchy"])
        assert bad.returncode == 1 and "unknown option --hierarchy" in bad.stderr


@pytest.mark.parametrize("args,msg", [
    (["--min-cluster-size", "4"], "--min-cluster-size needs --hierarchy"),
    (["--hierarchy", "--min-cluster-size", "1"], "--min-cluster-size must be >= 2"),
    (["--hierarchy", "--min-cluster-size", "0"], "--min-cluster-size must be >= 2"),
    (["--hierarchy", "--minpts", "1"], "--min-cluster-size must be >= 2"),  # the default is --minpts
])
def test_flag_errors_exit_before_the_gpu(args, msg):
    r = _run("clust-dbscan", ["--fast", "-l", "-i", "list.txt", "-o", "o.txt"] + args)
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


@pytest.mark.parametrize("seed", range(1, 4))
@pytest.mark.parametrize("use64,n_empty,max_posting", [(False, 0, 0), (False, 2, 5), (True, 3, 0), (True, 0, 5)])
def test_restated_cut_equals_the_reference_dbscan(seed, use64, n_empty, max_posting):
    """The anchor: at every eps <= eps_max, cutting the restated hierarchy gives the core points of the reference's neighbour
    relation and, on them, the labels of the reference's own KssdDBSCAN (compiled, oracle/_ref).  Where that library is not
    built the restated walk (tests/refdbscan.py, itself pinned to it by tests/test_cpu_refpin.py) stands in, with a warning."""
    L = reflib.ref_dbscan()
    if L is None:
        # a checkout where the other reference libraries were built must have this one too: the check must not lapse silently
        assert not os.path.isdir(reflib.REF_DIR) or not os.listdir(reflib.REF_DIR), "oracle/_ref exists without libref_dbscan.so"
        warnings.warn("oracle/_ref/libref_dbscan.so is not built: the restated KssdDBSCAN stands for the reference")
    sk = S.family_sets(seed, use64, n_empty)
    n = len(sk)
    sizes = [len(s) for s in sk]
    pair_js = [float(RH.KD.jaccard(c, sizes[p], sizes[q])) for (p, q), c in RH.kept_pairs(sk, EPS_MAX, S.KMER, use64, max_posting).items()]
    saw_noise = saw_two = False
    for min_pts in (2, 5):
        forest, core = RH.hierarchy(sk, EPS_MAX, min_pts, S.KMER, use64, max_posting)
        cuts = _clear_eps(forest, core, pair_js)
        distinct = set()
        for eps in cuts:
            lab, is_core = RH.cut(n, forest, core, eps, S.KMER)
            nb = R.neighbour_lists(sk, eps, S.KMER, use64, max_posting)
            want_core = [len(x) + 1 >= min_pts for x in nb]
            assert is_core == want_core, (eps, min_pts)
            if L is not None:
                genomes = P.genomes_of(n, True)
                ref, _, log = reflib.kssd_dbscan_print(L, sk, use64, eps, min_pts, S.KMER, genomes, True, threads=1 + seed % 4,
                                                       max_posting=max_posting)
                m = re.search(r"-----Core points: (\d+) ", log)
                assert (int(m.group(1)) if m else 0) == sum(is_core), (eps, min_pts)
            else:
                ref = R.labels_of(sk, eps, min_pts, S.KMER, use64, max_posting)
            idx = [v for v in range(n) if is_core[v]]
            assert [lab[v] for v in idx] == [int(ref[v]) for v in idx], (eps, min_pts)
            assert all(lab[v] == -1 for v in range(n) if not is_core[v])
            distinct.add(tuple(lab))
            saw_noise |= -1 in lab
            saw_two |= max(lab) >= 1
        assert len(distinct) >= 3  # the cuts are not all alike
    assert saw_noise and saw_two


def test_restated_hierarchy_hand_cases():
    a = np.arange(100, dtype=np.uint32)
    b = np.concatenate([a[:80], np.arange(1000, 1020, dtype=np.uint32)])   # j(a, b) = 80 / 120
    c = np.concatenate([a[:50], np.arange(2000, 2050, dtype=np.uint32)])   # j(a, c) = 50 / 150, j(b, c) = 50 / 150
    lone = np.arange(5000, 5010, dtype=np.uint32)
    sk = [a, b, c, lone, a.copy()]
    forest, core = RH.hierarchy(sk, 0.12, 2, 21, False)
    # k = 1: jcore = the best j; (0, 4) identical, m = 1; (0, 1) before (1, 4) at 80 / 120; c hangs at 50 / 150 on its lowest partner
    assert core[3][3] == RH.NONE and core[0] == (100, 100, 100, 4)
    assert forest == [(0, 4, 100, 100, 100), (0, 1, 80, 100, 100), (0, 2, 50, 100, 100)]
    # k = 2: jcore(0) = 80 / 120 now limits the edge (0, 4); the triple is the core triple of 0
    forest3, core3 = RH.hierarchy(sk, 0.12, 3, 21, False)
    assert core3[0] == (80, 100, 100, 1) and forest3[0] == (0, 1, 80, 100, 100) and forest3[1] == (0, 4, 80, 100, 100)
    assert RH.cut(5, forest, core, 0.001, 21) == ([0, -1, -1, -1, 0], [True, False, False, False, True])
    assert RH.cut(5, forest, core, 0.02, 21)[0] == [0, 0, -1, -1, 0]
    # u64: three empty sketches form a star from the first at m = 1
    e = np.zeros(0, dtype=np.uint64)
    f64, c64 = RH.hierarchy([e, a.astype(np.uint64), e, e], 0.05, 2, 21, True)
    assert f64 == [(0, 2, 0, 0, 0), (0, 3, 0, 0, 0)] and c64[1][3] == RH.NONE
    assert RH.cut(4, f64, c64, 0.01, 21) == ([0, -1, 0, 0], [True, False, True, True])


def test_cut_through_ctypes_equals_the_restatement():
    from rabbittclust_amd import api, _lib
    checked = 0
    for seed, use64, n_empty, mp in [(1, False, 2, 0), (2, True, 3, 0), (3, False, 0, 5)]:
        sk = S.family_sets(seed, use64, n_empty)
        for min_pts in (1, 2, 5, 40):
            forest, core = RH.hierarchy(sk, EPS_MAX, min_pts, S.KMER, use64, mp)
            f, c = _arrays(forest, core)
            for eps in EPS_CUTS:
                lab, is_core = api.hierarchy_cut(f, c, EPS_MAX, eps, S.KMER)
                want, want_core = RH.cut(len(sk), forest, core, eps, S.KMER)
                assert lab.tolist() == want and is_core.tolist() == want_core, (seed, min_pts, eps)
                checked += 1
    assert checked > 100
    # the errors: past eps_max, eps <= 0, jaccard_min <= 1e-12
    for eps, status in [(0.1200001, _lib.RTC_ERR_ARG), (0.0, _lib.RTC_ERR_ARG), (-1.0, _lib.RTC_ERR_ARG)]:
        with pytest.raises(api.RtcError) as ei:
            api.hierarchy_cut(f, c, EPS_MAX, eps, S.KMER)
        assert ei.value.status == status
    with pytest.raises(api.RtcError) as ei:
        api.hierarchy_cut(f, c, 2.0, 1.5, S.KMER)
    assert ei.value.status == _lib.RTC_ERR_UNSUPPORTED
    # nothing at all
    lab, is_core = api.hierarchy_cut(*_arrays([], []), 0.1, 0.05, 21)
    assert lab.size == 0 and is_core.size == 0


def _hand_forest():
    """Two dense groups of four (distances ~0.003) joined at ~0.02, a third group of three far off (~0.05), one straggler that
    leaves the first group at ~0.01, and a point without a core level.  Triples over sketches of 1000 hashes."""
    def tri(common):
        return (common, 1000, 1000)
    edges = [(0, 1, 940), (1, 2, 938), (2, 3, 936), (4, 5, 941), (5, 6, 939), (6, 7, 937), (8, 9, 930), (9, 10, 929),
             (3, 11, 800), (0, 4, 650), (7, 8, 350)]
    forest = sorted(((p, q) + tri(c) for p, q, c in edges), key=lambda e: (-RH.jac(e[2:]), e[0], e[1]))
    core = [(990, 1000, 1000, (v + 1) % 12) for v in range(12)] + [(0, 1000, 0, RH.NONE)]
    return forest, core


def test_flat_through_ctypes_equals_the_restatement():
    from rabbittclust_amd import api, _lib
    forest, core = _hand_forest()
    f, c = _arrays(forest, core)
    lab, stab, gap = RH.flat(13, forest, core, 21, 3)
    # the two dense groups and the far one; the straggler stays with the group it fell out of; no core level: -1
    assert lab == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 0, -1] and gap > 1e-9
    got, got_stab = api.hierarchy_flat(f, c, 21, 3, return_stability=True)
    assert got.tolist() == lab and got_stab.tolist() == stab
    # min_cluster_size 5: the pair of dense groups together (8 + the straggler) against the far three, which is too small
    lab5, stab5, _ = RH.flat(13, forest, core, 21, 5)
    assert lab5 == [0] * 8 + [-1] * 3 + [0, -1] or lab5 == [0] * 12 + [-1]
    got5, got_stab5 = api.hierarchy_flat(f, c, 21, 5, return_stability=True)
    assert got5.tolist() == lab5 and got_stab5.tolist() == stab5
    # forests of the restated hierarchy on the seeded sets
    checked = clusters = 0
    for seed, use64, n_empty in [(1, False, 2), (2, True, 3), (3, False, 0), (4, True, 0)]:
        sk = S.family_sets(seed, use64, n_empty)
        for min_pts, mcs in [(2, 2), (2, 4), (5, 5), (3, 7)]:
            forest, core = RH.hierarchy(sk, EPS_MAX, min_pts, S.KMER, use64)
            want, want_stab, gap = RH.flat(len(sk), forest, core, S.KMER, mcs)
            got, got_stab = api.hierarchy_flat(*_arrays(forest, core), S.KMER, mcs, return_stability=True)
            assert got.tolist() == want, (seed, min_pts, mcs)
            assert got_stab.tolist() == want_stab  # the same terms summed in the same order
            checked += 1
            clusters = max(clusters, len(want_stab))
    assert checked == 16 and clusters >= 3
    # sub-families inside super-families: true splits, and the selection has stabilities to compare
    for seed in range(1, 4):
        for use64 in (False, True):
            sk = RH.nested_sets(seed, use64)
            for min_pts, mcs in [(2, 3), (3, 4), (5, 5)]:
                forest, core = RH.hierarchy(sk, EPS_MAX, min_pts, S.KMER, use64)
                want, want_stab, gap = RH.flat(len(sk), forest, core, S.KMER, mcs)
                assert gap > 1e-9 and len(want_stab) == 5
                got, got_stab = api.hierarchy_flat(*_arrays(forest, core), S.KMER, mcs, return_stability=True)
                assert got.tolist() == want and got_stab.tolist() == want_stab, (seed, use64, min_pts, mcs)
    # the errors
    for mcs in (1, 0, -3):
        with pytest.raises(api.RtcError) as ei:
            api.hierarchy_flat(f, c, 21, mcs)
        assert ei.value.status == _lib.RTC_ERR_ARG
    cyc = forest[:2] + [forest[0]]  # an edge twice: not a forest
    with pytest.raises(api.RtcError):
        api.hierarchy_flat(*_arrays(cyc, core), S.KMER, 2)


def test_flat_ties_go_to_the_children_and_the_root_is_not_selected():
    from rabbittclust_amd import api
    # two pairs at one distance joined at twice that distance: each child's stability is 2 (l - l / 2) = l, the parent is the root
    tri = lambda c: (c, 100, 100)
    forest = [(0, 1) + tri(90), (2, 3) + tri(90), (1, 2) + tri(60)]
    core = [(95, 100, 100, (v + 1) % 4) for v in range(4)]
    lab, stab, _ = RH.flat(4, forest, core, 21, 2)
    assert lab == [0, 0, 1, 1]
    assert api.hierarchy_flat(*_arrays(forest, core), 21, 2).tolist() == lab
    # one tree without a split is the only cluster: the root is selected
    chain = [(0, 1) + tri(90), (1, 2) + tri(80), (2, 3) + tri(70)]
    assert RH.flat(4, chain, core, 21, 2)[0] == [0, 0, 0, 0]
    assert api.hierarchy_flat(*_arrays(chain, core), 21, 2).tolist() == [0, 0, 0, 0]
    # two trees: each is a top-level cluster and can be selected
    two = [(0, 1) + tri(90), (2, 3) + tri(90)]
    assert api.hierarchy_flat(*_arrays(two, core), 21, 2).tolist() == [0, 0, 1, 1] == RH.flat(4, two, core, 21, 2)[0]
