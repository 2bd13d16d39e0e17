"""clust-dbscan --knn without a GPU: the two closed forms rtc_dbscan_knn computes against the sequential steps
they replace -- the selection against the reference's min-heap on random arrival sequences, the walk against
refdbscan.sequential_walk on random directed lists -- the restated k-NN lists against the full neighbourhoods where they must
agree, the library's exports and the command line's flag errors.  Then the sets of tests/knn_sets.py: that they hold, on the
restatement, the cases tests/test_gpu_dbscan_knn.py runs them for (rows, k, tied groups and first-shared indices past one wave
of 64 lanes, labels that show which neighbours a row kept, the binary32 eps test, u16 saturation inside the score)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import knn_sets as K
from tests import refdbscan as R
from tests import refdbscan_knn as RK
from tests import sweep_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-dbscan")


def test_selection_closed_form_equals_the_heap():
    rng = np.random.default_rng(11)
    scores = [np.float32(x) for x in (0.125, 0.25, 0.3, 0.5, 0.75)]  # few distinct scores: ties dominate
    needed = truncated = short = 0
    for _ in range(12_000):
        n_cand = int(rng.integers(0, 14))
        k = int(rng.integers(1, 9))
        ids = rng.permutation(40)[:n_cand].tolist()  # arrival order is not id order
        n_scores = int(rng.integers(1, len(scores) + 1))
        arrivals = [(c, scores[int(rng.integers(0, n_scores))]) for c in ids]
        want = {c for c, _ in RK.heap_select(arrivals, k)}
        got, by_arrival = RK.closed_select(arrivals, k)
        assert got == want, (arrivals, k)
        short += n_cand < k
        truncated += n_cand > k
        needed += by_arrival
    assert short > 1000 and truncated > 1000 and needed > 1000  # every branch of the closed form was exercised


def test_walk_closed_form_equals_the_sequential_walk():
    rng = np.random.default_rng(12)
    borders = noise = 0
    for _ in range(2_500):
        n = int(rng.integers(1, 15))
        deg = int(rng.integers(0, 4))
        nbrs = []
        for v in range(n):
            others = [u for u in range(n) if u != v]
            m = min(len(others), int(rng.integers(0, deg + 1)))
            nbrs.append([others[i] for i in rng.permutation(len(others))[:m]])  # directed: u in N(v) says nothing about v in N(u)
        min_pts = int(rng.integers(1, 5))
        lab, n_core = R.sequential_walk(nbrs, min_pts)
        want = [x if x >= 0 else -1 for x in lab]
        got, core = RK.closed_walk(nbrs, min_pts)
        assert got == want, (nbrs, min_pts)
        assert sum(core) == n_core
        borders += any(g >= 0 and not c for g, c in zip(got, core))
        noise += -1 in got
    assert borders > 100 and noise > 100


@pytest.mark.parametrize("max_posting", [0, 5])
def test_knn_lists_with_a_large_k_are_the_full_neighbourhoods(max_posting):
    host = S.family_sets(2, False, n_empty=2)
    n = len(host)
    rows_checked = 0
    for eps in (0.02, 0.06):
        t = R.jaccard_min(eps, S.KMER)
        full = R.neighbour_lists(host, eps, S.KMER, False, max_posting)
        knn = RK.knn_lists(host, eps, S.KMER, n, max_posting)
        passers = RK.passers_in_arrival_order(host, eps, S.KMER, max_posting)
        for p in range(n):
            assert [c for c, _ in passers[p]] == full[p]  # the same scan, the same order
            if all(float(s) >= t for _, s in passers[p]):  # no passer fails the float test: the heap holds them all
                assert sorted(knn[p]) == sorted(full[p]), (eps, p)
                rows_checked += 1
            else:
                assert set(knn[p]) < set(full[p])
    assert rows_checked > n


def test_effective_k_and_labels_of_knn():
    host = S.family_sets(1, False)
    assert RK.effective_k(2, 5) == 4 and RK.effective_k(4, 5) == 4 and RK.effective_k(9, 5) == 9 and RK.effective_k(0, 5) == 0
    # k = n truncates nothing: where every row passes the float test the labels are the plain DBSCAN's
    eps = 0.04
    t = R.jaccard_min(eps, S.KMER)
    if all(float(s) >= t for row in RK.passers_in_arrival_order(host, eps, S.KMER) for _, s in row):
        assert np.array_equal(RK.labels_of_knn(host, eps, 5, S.KMER, len(host)), R.labels_of(host, eps, 5, S.KMER, False))
    assert not np.array_equal(RK.labels_of_knn(host, eps, 2, S.KMER, 1), R.labels_of(host, eps, 2, S.KMER, False))


def test_library_exports_the_knn_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "rabbittclust_amd", "librtclust_hip.so"))
    assert hasattr(lib, "rtc_dbscan_knn") and hasattr(lib, "rtc_dbscan_knn_counters")
    from rabbittclust_amd import api
    assert callable(api.Context.dbscan_knn) and callable(api.Context.dbscan_knn_counters)


def _run(args, cwd):
    if not os.path.exists(BIN):
        pytest.fail("clust-dbscan missing: run __graft_entry__.build()")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", RTC_NO_WARMUP="1")
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=60, env=env, cwd=cwd)


@pytest.mark.parametrize("extra,flag", [
    (["--minhash"], "--minhash"),
    (["--fast", "--eps-sweep", "0.01,0.02"], "--eps-sweep"),
    (["--fast", "--kdist"], "--kdist"),
    (["--fast", "--hierarchy"], "--hierarchy"),
    (["--fast", "--min-cluster-size", "3"], "--min-cluster-size"),
    (["--fast", "--db", "model.db", "--build"], "--db"),
    (["--fast", "--db", "model.db", "--assign"], "--db"),
])
def test_knn_excludes_the_flows_of_the_symmetric_relation(tmp_path, extra, flag):
    lst = tmp_path / "list.txt"
    lst.write_text("")
    r = _run(extra + ["-l", "-i", str(lst), "--knn", "3", "-o", "o.txt"], str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert "ERROR: --knn does not go with " + flag + "\n" in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr


def test_knn_run_on_a_missing_input_ends_before_the_gpu(tmp_path):
    r = _run(["--fast", "-l", "-i", "nowhere.txt", "--knn", "2", "--minpts", "5", "-o", "o.txt"], str(tmp_path))
    assert r.returncode == 1, r.stderr
    assert "ERROR: --knn: cannot open the input nowhere.txt\n" in r.stderr
    assert "context" not in r.stderr and "Running DBSCAN" not in r.stderr
    # --knn 0 is the run without the flag: its error path is the one it always was
    r0 = _run(["--fast", "-l", "-i", "nowhere.txt", "--knn", "0", "-o", "o.txt"], str(tmp_path))
    assert r0.returncode == 1 and "--knn" not in r0.stderr


def test_help_describes_the_flag():
    r = _run(["-h"], ROOT)
    assert r.returncode == 0 and "--knn K" in r.stdout and "not in this build" not in r.stdout


# ---- the sets of tests/knn_sets.py hold the cases the GPU tests rely on (rows, k, tied groups, first-shared indices past 64) ----

SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _stars(seed):
    host, info = K.star_set(seed)
    return host, info, RK.passers_in_arrival_order(host, K.EPS, K.KMER)


def _labels(nbrs, min_pts):
    lab, _ = R.sequential_walk(nbrs, min_pts)
    return [x if x >= 0 else -1 for x in lab]


def _lists(passers, select, k, t):
    return [[c for c, s in select(row, k) if float(s) >= t] for row in passers]


# Selection rules a kernel could follow instead of the heap's; each must show in the star set's labels.
def _lowest_id(row, k):
    return sorted(row, key=lambda x: (-float(x[1]), x[0]))[:k]


def _highest_id(row, k):
    return sorted(row, key=lambda x: (-float(x[1]), -x[0]))[:k]


def _earliest_arrival(row, k):
    return [row[i] for i in sorted(range(len(row)), key=lambda i: (-float(row[i][1]), i))[:k]]


WRONG_RULES = (_lowest_id, _highest_id, _earliest_arrival)


@pytest.mark.parametrize("seed", SEEDS)
def test_star_set_rows_are_what_the_stars_say(seed):
    host, info, passers = _stars(seed)
    assert len(host) == sum(1 + sum(s[1:]) for s in K.STARS)
    for hub, leaves in zip(info["hubs"], info["leaves"]):
        ids = [i for i, _ in leaves]
        assert min(ids) < hub < max(ids)
        assert [c for c, _ in passers[hub]] == ids  # every leaf passes, and they arrive in chunk order
        assert ids != sorted(ids)                   # which is not the id order
        for i, kind in leaves:
            assert [c for c, _ in passers[i]] == [hub]
            assert len(host[i]) == K.W + {"tied": 0, "worse": -2}.get(kind, 2)
        late = [i for i, kind in leaves if kind == "late"]
        assert all(i > j for i in late for j, kind in leaves if kind != "late")
        score = {kind: {float(s) for (c, s), (_, kd) in zip(passers[hub], leaves) if kd == kind} for kind in ("early", "worse", "tied", "late")}
        assert len(score["tied"]) == 1 and all(len(v) <= 1 for v in score.values())
        if score["early"]:
            assert score["early"] == score["late"] and min(score["early"]) > max(score["tied"])
        if score["worse"]:
            assert max(score["worse"]) < min(score["tied"])
    t = R.jaccard_min(K.EPS, K.KMER)
    assert all(float(s) >= t for row in passers for _, s in row)  # the float test drops nothing here


@pytest.mark.parametrize("seed", SEEDS)
def test_star_set_reaches_past_one_wave(seed):
    host, info, passers = _stars(seed)
    hubs = info["hubs"]
    exact_k = big_q = big_e = 0
    for k in K.KS:
        shapes = [K.row_shape(passers[h], k) for h in hubs]
        assert any(P <= k for P, *_ in shapes), k
        assert any(Q > k and G > 0 and h > 0 for P, G, Q, h, E in shapes), k
        exact_k += any(P > k and Q == k for P, G, Q, h, E in shapes)
        big_q += any(Q > k and Q > 64 for P, G, Q, h, E in shapes)
        big_e += any(Q > k and E > 64 for P, G, Q, h, E in shapes)
    assert exact_k >= 1 and big_q >= 1 and big_e >= 1 and max(K.KS) > 64
    # the passers that get an arrival key: the first Q of a row with Q > k.  Their keys are the chunk starts in the hub's list
    for hub, leaves in zip(hubs, info["leaves"]):
        assert [K.first_shared_index(host, hub, c) for c, _ in passers[hub]] == \
               np.cumsum([len(host[hub]) - sum(len(host[c]) for c, _ in leaves)] + [len(host[c]) for c, _ in leaves[:-1]]).tolist()
    listed = {}
    for k in K.KS:
        for hub in hubs:
            P, G, Q, h, E = K.row_shape(passers[hub], k)
            if Q > k:
                s_star = sorted((s for _, s in passers[hub]), reverse=True)[k - 1]
                listed.setdefault(hub, set()).update(K.first_shared_index(host, hub, c) for c, s in passers[hub] if s >= s_star)
    assert max(len({i // 64 for i in v}) for v in listed.values()) >= 3
    everything = set().union(*listed.values())
    assert {63, 64, 65} <= everything  # a first shared hash in the last lane of a block, and in the first two of the next


@pytest.mark.parametrize("seed", SEEDS)
def test_star_set_labels_show_the_selection(seed):
    host, info, passers = _stars(seed)
    t = R.jaccard_min(K.EPS, K.KMER)
    for k in K.KS:
        for row in passers:
            held = {c for c, _ in RK.heap_select(row, k)}
            got, by_arrival = RK.closed_select(row, k)
            assert got == held and by_arrival == (K.row_shape(row, k)[2] > k)
        nbrs = RK.knn_lists(host, K.EPS, K.KMER, k)
        assert nbrs == _lists(passers, RK.heap_select, k, t)
        want = _labels(nbrs, K.MIN_PTS)
        assert want == RK.labels_of_knn(host, K.EPS, K.MIN_PTS, K.KMER, k).tolist()
        closed, core = RK.closed_walk(nbrs, K.MIN_PTS)
        assert closed == want and [v for v in range(len(host)) if core[v]] == info["hubs"]
        # a leaf is in its hub's cluster exactly when the hub kept it
        for s, (hub, leaves) in enumerate(zip(info["hubs"], info["leaves"])):
            assert want[hub] == s
            for i, _ in leaves:
                assert want[i] == (s if i in nbrs[hub] else -1)
        assert any(K.row_shape(passers[h], k)[2] > k for h in info["hubs"])  # every k of the list has a row that needs the order
        for rule in WRONG_RULES:
            wrong = _lists(passers, rule, k, t)
            assert [len(x) for x in wrong] == [len(x) for x in nbrs]  # the same counts: only the labels can tell
            assert _labels(wrong, K.MIN_PTS) != want, (k, rule.__name__)


@pytest.mark.parametrize("low", [False, True])
def test_bridged_stars_are_one_cluster_many_hops_deep(low):
    host, info = K.bridged_star_set(1, low)
    passers = RK.passers_in_arrival_order(host, K.EPS, K.KMER)
    hubs, bridges = info["hubs"], info["bridges"]
    assert len(bridges) == len(hubs) - 1 and min(bridges) > max(hubs)
    for b, (h0, h1) in zip(bridges, zip(hubs, hubs[1:])):
        assert [c for c, _ in passers[b]] == [h0, h1]
        for h in (h0, h1):
            score = dict(passers[h])
            leaf = [score[c] for c in score if c not in bridges]
            assert score[b] < min(leaf) if low else score[b] > max(leaf)
            assert [c for c, _ in passers[h]].index(b) >= len(leaf)  # the bridges arrive last
    for k in ((200,) if low else (2, 64, 129)):
        nbrs = RK.knn_lists(host, K.EPS, K.KMER, k)
        want, core = RK.closed_walk(nbrs, K.MIN_PTS)
        assert want == RK.labels_of_knn(host, K.EPS, K.MIN_PTS, K.KMER, k).tolist()
        assert all(want[v] == 0 for v in hubs + bridges) and max(want) == 0
        assert all(core[v] for v in hubs + bridges) and sum(core) == len(hubs) + len(bridges)
        # the number of hub 0 reaches the last hub only through every bridge in turn
        depth = {hubs[0]: 0}
        queue = [hubs[0]]
        for p in queue:
            for q in nbrs[p]:
                if q not in depth:
                    depth[q] = depth[p] + 1
                    if core[q]:
                        queue.append(q)
        assert depth[hubs[-1]] == 2 * (len(hubs) - 1) >= len(hubs)
        if low:  # sorted by score the bridge is the last record of a row longer than one wave
            for h in hubs[1:]:
                by_score = sorted(passers[h], key=lambda x: (-float(x[1]), x[0]))
                assert by_score[-1][0] in bridges
            assert sum(len(passers[h]) > 64 for h in hubs) >= 3


def test_chunk_and_decoy_variants_hold_their_cases():
    host, info = K.chunk_star_set(1)
    n = len(host)
    assert n * (n - 1) // 2 > 64 * n + 1024  # the whole triangle is past the smallest edge budget
    assert all(int(s[-1]) == K.CHUNK_SHARED for s in host)
    passers = RK.passers_in_arrival_order(host, K.CHUNK_EPS, K.KMER)
    for hub, leaves in zip(info["hubs"], info["leaves"]):
        assert [c for c, _ in passers[hub]] == [i for i, _ in leaves]
        assert all([c for c, _ in passers[i]] == [hub] for i, _ in leaves)
    assert all(Q > 64 and G > 0 and h > 0 for P, G, Q, h, E in (K.row_shape(passers[h], 64) for h in info["hubs"]))
    # the decoy: pruning lowers some tied leaves' counts, which changes the kept sets
    host, info = K.star_set(1, decoy=True)
    assert len(R.kept_hashes(host, K.DECOY_MAX_POSTING)) < len(R.kept_hashes(host, 0))
    pruned = RK.passers_in_arrival_order(host, K.EPS, K.KMER, K.DECOY_MAX_POSTING)
    assert pruned[info["decoys"][0]] == []
    for hub, leaves in zip(info["hubs"], info["leaves"]):
        assert [c for c, _ in pruned[hub]] == [i for i, _ in leaves]
        assert len({float(s) for (_, s), (_, kind) in zip(pruned[hub], leaves) if kind == "tied"}) == 2
    hub = info["hubs"][3]
    keys = [K.first_shared_index(host, hub, c, K.DECOY_MAX_POSTING) for c, _ in pruned[hub]]
    assert keys == sorted(keys) and keys != [K.first_shared_index(host, hub, c) for c, _ in pruned[hub]]
    for k in (64, 128):
        want = RK.labels_of_knn(host, K.EPS, K.MIN_PTS, K.KMER, k, K.DECOY_MAX_POSTING)
        assert not np.array_equal(want, RK.labels_of_knn(host, K.EPS, K.MIN_PTS, K.KMER, k))
        assert any(Q > k and G > 0 for P, G, Q, h, E in (K.row_shape(pruned[h], k) for h in info["hubs"]))


@pytest.mark.parametrize("a,b,c", K.float_boundary_pairs())
def test_float_boundary_pairs_pass_in_doubles_and_fail_in_binary32(a, b, c):
    eps = K.float_boundary_eps(a, b, c)
    t = R.jaccard_min(eps, K.KMER)
    u = a + b - c
    assert float(np.float32(c) / np.float32(u)) < t <= c / u
    host = K.float_boundary_sketches(a, b, c)
    assert [len(s) for s in host] == [a, b] and len(np.intersect1d(*host)) == c
    assert [len(p) for p in RK.passers_in_arrival_order(host, eps, K.KMER)] == [1, 1]
    assert RK.knn_lists(host, eps, K.KMER, 5) == [[], []]
    assert R.neighbour_lists(host, eps, K.KMER, False) == [[1], [0]]
    assert RK.labels_of_knn(host, eps, 2, K.KMER, 5).tolist() == [-1, -1]
    assert R.labels_of(host, eps, 2, K.KMER, False).tolist() == [0, 0]


def test_saturated_counts_change_the_kept_neighbour():
    host = K.saturated_choice_set()
    eps = K.SATURATED_EPS
    t = R.jaccard_min(eps, K.KMER)
    capped = RK.knn_lists(host, eps, K.KMER, 1)
    assert capped == [[2], [2], [0]]
    assert RK.labels_of_knn(host, eps, 2, K.KMER, 1).tolist() == [0, 1, 0]
    # the same with exact counts, by hand: every pair passes, the best score of a row stays
    exact = []
    for p in range(3):
        row = []
        for c in range(3):
            if c != p:
                common = len(np.intersect1d(host[p], host[c], assume_unique=True))
                assert common * (1.0 + t) + 1e-12 >= t * len(host[p]) + t * len(host[c])
                row.append((np.float32(common) / np.float32(len(host[p]) + len(host[c]) - common), c))
        assert all(float(s) >= t for s, _ in row)
        exact.append([max(row)[1]])
    assert exact == [[1], [0], [0]] and exact[0] != capped[0]
    assert _labels(exact, 2) == [0, 0, 1]
