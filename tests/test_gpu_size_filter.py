"""GPU: the MST's size-ratio filter once radio * min(|A|,|B|) leaves 32 bits.  A pair is a candidate iff it shares
a hash and max <= R * min in exact integers, R = floor(2 e^(d (k-1)) - 1) saturated at INT32_MAX, R < 0: no size test.  Every
expectation here is a brute force in Python integers over np.intersect1d; no oracle."""
import math

import os

import numpy as np
import pytest

from oracle import brute

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
THR_C_INT = 0.6931471805862327  # k = 32: calr = 4 294 967 298, which a C int conversion modulo 2^32 turns into 2


def _radio(thr, k):
    return brute.radio(thr, k)


def _filter_sets(dt):
    """Sketches that all share hash 1: 1, 2 and 3 hashes beside 21, 22, 1000, 3000, 99 999 and 100 000.  With the radii of
    _RADII, R * min lands on 2^31 + 2 (min 2), 2^32 + 2 (min 3: modulo 2^32 that is 2 < max), exactly on max and one below."""
    rng = np.random.default_rng(5)
    top = np.iinfo(dt).max
    pool = np.unique(rng.integers(2, top, size=260_000, dtype=np.uint64).astype(dt))
    pool = pool[pool > 1]
    rng.shuffle(pool)
    one = np.array([1], dtype=dt)
    sets = []
    for size, lo in [(1, 0), (2, 0), (3, 0), (21, 10), (22, 10), (1000, 40), (3000, 40), (99_999, 5000), (100_000, 100_000)]:
        sets.append(np.unique(np.concatenate([one, pool[lo:lo + size - 1]])))
    assert [len(s) for s in sets] == [1, 2, 3, 21, 22, 1000, 3000, 99_999, 100_000]
    return sets


# 7: 3 * 7 = 21 keeps (3, 21), drops (3, 22); 33 333: 3 R = 99 999 keeps (3, 99 999), drops (3, 100 000);
# 2^30 + 1: 2 R = 2^31 + 2 (negative as an int product); 1 431 655 766: 3 R = 2^32 + 2 (2 modulo 2^32); saturated; no test
_RADII = [1, 7, 33_333, 2 ** 30 + 1, 1_431_655_766, INT32_MAX, -1]


def _brute_edges(sets, radio):
    out = []
    for i in range(len(sets)):
        for j in range(i):
            c = len(np.intersect1d(sets[i], sets[j], assume_unique=True))
            a, b = len(sets[i]), len(sets[j])
            if c and (radio < 0 or max(a, b) <= radio * min(a, b)):
                out.append((i, j, c))
    return np.array(sorted(out), dtype=np.int64).reshape(-1, 3)


def _sorted_edges(e, m):
    a = e[:m].cpu().numpy().view(np.uint32).astype(np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


@pytest.mark.parametrize("width", [8, 4])
def test_candidate_edges_size_filter_every_path(ctx, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    sets = _filter_sets(dt)
    n = len(sets)
    sk = api.SketchSet.from_host(sets, ctx.device, k=21, kind="minhash" if width == 8 else "kssd", width=width)
    cap = n * n
    for radio in _RADII:
        want = _brute_edges(sets, radio)
        for name, switches, path in [("join", {"RTC_PAIR_JOIN": 2}, 3), ("tiled", {"RTC_PAIR_JOIN": 0}, 2),
                                     ("merge", {"RTC_PAIR_FORCE_MERGE": 1}, 1)]:
            with ctx.env(**switches):
                e, m = ctx.pair_edges(sk, 1, n, 0, n - 1, radio, cap)
                assert ctx.pair_last_path() == path, (name, radio)
            assert np.array_equal(_sorted_edges(e, m), want), (name, width, radio)
        common = ctx.pair_common(sk, lower_only=False)
        e, cnt = ctx.extract_edges(common, sk, 0, n, 0, n, radio, cap)
        ctx.sync()
        assert np.array_equal(_sorted_edges(e, int(cnt.item())), want), ("extract_edges", width, radio)
    # what the radii exercise: (3, 100 000) is dropped only by 33 333; the 2^32 + 2 product keeps it
    assert len(_brute_edges(sets, 7)) < len(_brute_edges(sets, 33_333)) < len(_brute_edges(sets, 1_431_655_766))
    assert len(_brute_edges(sets, INT32_MAX)) == len(_brute_edges(sets, -1)) == n * (n - 1) // 2


def _mst_sets(dt, rng_seed):
    """ten s = 1000 sketches in two groups that share hashes, plus 1, 3 and 50 000 hash sketches linked to them"""
    rng = np.random.default_rng(rng_seed)
    pool = np.unique(rng.integers(1, np.iinfo(dt).max, size=80_000, dtype=np.uint64).astype(dt))
    rng.shuffle(pool)
    sets = []
    for g in range(10):
        core = pool[:400] if g < 5 else pool[400:800]
        sets.append(np.sort(np.concatenate([core, pool[1000 + 600 * g:1000 + 600 * (g + 1)]])))
    sets += [np.sort(pool[:1]), np.sort(pool[400:403]), np.sort(np.concatenate([pool[10_000:59_700], pool[:300]]))]
    assert [len(s) for s in sets[:10]] == [1000] * 10
    return sets


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _brute_forest(sets, k, containment, thr):
    return brute.mst_forest(sets, k, containment, thr)


def _records(mst):
    return [(float(d), int(a), int(b)) for d, a, b in zip(mst["dist"], mst["preNode"], mst["sufNode"])]


def _clusters(records, n, thr):
    """the clusters at thr: generateForest's cut (brute.generate_forest, pinned to ref_distance_half.npz below), then the
    connected groups"""
    return brute.partition(brute.generate_forest(records, thr), n)


def _assert_forest(got, forest, n, thr):
    assert len(got) == len(forest)
    assert np.array_equal(np.sort(got["dist"]).view(np.uint64), np.sort(np.array([f[0] for f in forest])).view(np.uint64))
    assert _clusters(_records(got), n, thr) == _clusters(forest, n, thr)


@pytest.mark.parametrize("kind", ["minhash", "kssd"])
def test_mst_and_dense_at_d07(ctx, kind):
    """d = 0.7, s = 1000: R = 2 405 207 (k = 21) / 5 044 160 (k = 22, KSSD's k is 2 half_k); R * 1000 is past 2^31"""
    from rabbittclust_amd import api
    width, dt, k = (8, np.uint64, 21) if kind == "minhash" else (4, np.uint32, 22)
    sets = _mst_sets(dt, 8 if kind == "minhash" else 9)
    n = len(sets)
    assert _radio(0.7, k) * 1000 >= 2 ** 31
    sk = api.SketchSet.from_host(sets, ctx.device, k=k, kind=kind, width=width)
    for containment in (False, True):
        cand, forest = _brute_forest(sets, k, containment, 0.7)
        assert len(cand) == sum(1 for i in range(n) for j in range(i) if len(np.intersect1d(sets[i], sets[j])))
        _assert_forest(ctx.mst(sk, 0.7, is_containment=containment), forest, n, 0.7)
        dm, dense, ani = ctx.mst_dense(sk, 0.7, is_containment=containment)
        _assert_forest(dm, forest, n, 0.7)
        assert int(ani.sum()) == len(cand)  # every sharing pair is a candidate


def _cint_sets():
    """two groups of 1000-hash sketches with a 300-hash member each: size ratio 3.3 > 2"""
    rng = np.random.default_rng(12)
    pool = np.unique(rng.integers(1, 1 << 63, size=30_000, dtype=np.uint64))
    rng.shuffle(pool)
    sets = []
    for g in range(12):
        core = pool[:500] if g < 6 else pool[500:1000]
        size = 300 if g % 6 == 0 else 1000
        sets.append(np.sort(np.unique(np.concatenate([core[:size // 2], pool[2000 + 800 * g:2000 + 800 * g + size - size // 2]]))))
    return sets


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_mst_at_c_int_wrap_threshold(world):
    """rtc_mst_sharded over in-process ranks at d = 0.6931471805862327, k = 32 equals the single-rank forest and the brute force"""
    from rabbittclust_amd import api
    sets = _cint_sets()
    n = len(sets)
    one = api.Context(0)
    ctxs = [api.Context(0) for _ in range(world)]
    comms = api.Comm.init_all(ctxs)
    try:
        sks = [api.SketchSet.from_host(sets, c.device, k=32) for c in ctxs]
        def rank_fn(r):
            def f():
                mst = ctxs[r].mst_sharded(comms[r], sks[r], THR_C_INT)[0].copy()
                ctxs[r].sync()
                return mst
            return f
        res = brute.run_ranks([rank_fn(r) for r in range(world)])
        single = one.mst(api.SketchSet.from_host(sets, one.device, k=32), THR_C_INT)
        _, forest = _brute_forest(sets, 32, False, THR_C_INT)
        _assert_forest(single, forest, n, THR_C_INT)
        for r in range(world):
            assert np.array_equal(res[r], single), f"rank {r}"
    finally:
        for c in comms:
            c.close()
        for c in ctxs + [one]:
            c.close()


def test_pipeline_step_at_c_int_wrap_threshold(ctx):
    """MstPipeline.step (torch-comm path) passes api.mst_radio through ctypes as a C int: at d = 0.6931471805862327, k = 32 the
    exact radio is past 2^32, and the forest must equal the native single-rank forest (every 300-hash genome joins its family)"""
    from rabbittclust_amd import api, pipeline
    desc = api.synth_family_descs(4, 5, global_seed=55, max_rate=0.01)
    L = 60_000
    off = np.arange(len(desc) + 1, dtype=np.uint64) * L
    seq = ctx.synth_genomes(desc, off)
    sizes = np.array([300 if g % 5 == 0 else 1000 for g in range(len(desc))], dtype=np.uint32)
    pipe = pipeline.MstPipeline(ctx, k=32, sketch_size=1000, threshold=THR_C_INT)
    stats = pipe.step(seq, off, sizes=sizes)
    host = pipe.last_sketches.to_host()
    n = len(host)
    cand, forest = _brute_forest(host, 32, False, THR_C_INT)
    assert any(max(len(host[i]), len(host[j])) > 2 * min(len(host[i]), len(host[j])) for _, i, j in forest)
    assert stats["cand_edges"] == len(cand)
    _assert_forest(pipe.last_mst, forest, n, THR_C_INT)
    native = ctx.mst(pipe.last_sketches, THR_C_INT)
    assert np.array_equal(np.sort(native["dist"]).view(np.uint64), np.sort(pipe.last_mst["dist"]).view(np.uint64))


def test_forest_cut_on_a_realized_distance(ctx):
    """the forest's doubles are the brute force's to the bit, so a threshold set on a realized distance cuts the same way as
    the reference's generateForest and one ulp below it cuts that edge.  The cut itself is first checked against what
    generateForest kept in tests/golden/ref_distance_half.npz (thresholds on an edge and one ulp either side)."""
    from rabbittclust_amd import api
    fx = np.load(os.path.join(GOLD, "ref_distance_half.npz"))
    i = 0
    while f"kr{i}_n" in fx:
        tree = _records(fx[f"kr{i}_tree"])
        for t, thr in enumerate(fx[f"kr{i}_thr"]):
            assert brute.generate_forest(tree, float(thr)) == _records(fx[f"kr{i}_forest{t}"]), (i, thr)
        i += 1
    assert i == 7
    sets = _mst_sets(np.uint64, 10)
    n = len(sets)
    sk = api.SketchSet.from_host(sets, ctx.device, k=21)
    got = ctx.mst(sk, 0.7)
    _, forest = _brute_forest(sets, 21, False, 0.7)
    _assert_forest(got, forest, n, 0.7)
    # realized distances where the cut matters: one ulp below, the edges at that distance leave the forest
    picked = 0
    for d in sorted(set(f[0] for f in forest if 0.0 < f[0] < 1.0), reverse=True):
        below = float(np.nextafter(d, 0.0))
        _, f_at = _brute_forest(sets, 21, False, d)
        _, f_below = _brute_forest(sets, 21, False, below)
        if len(_clusters(f_below, n, below)) <= len(_clusters(f_at, n, d)):
            continue
        for thr, f in ((d, f_at), (below, f_below)):
            _assert_forest(ctx.mst(sk, thr), f, n, thr)
        picked += 1
    assert picked >= 2


# ---- rtc_greedy at the common_min boundary ----------------------------------------------------------------------------
# The greedy decisions rest on common_min = ceil(...) of a double (rtc_greedy.hip; src/greedy.cpp:1112, :1216, :1218, :774)
# and then, off the fixed-size fast path, on dist <= threshold.  Thresholds d = -ln(x)/k (and one ulp either side) with
# x = 1/2, 1/4, 3/4 make jaccard_min = x / (2 - x) a simple fraction, so the ceil's argument is an exact integer or lies
# within an ulp of one for many sizes: a kernel or host that evaluated it in another order, or with a contraction, would
# decide differently there.  One representative and one query per call, the query sharing c = common_min - 1, common_min
# and common_min + 1 hashes with it; the expectation is the reference's rule in the same double expressions.

def _greedy_jm(thr, k):
    x = math.exp(-thr * k)  # src/greedy.cpp:1109 / :652
    return x / (2.0 - x)


def _greedy_arg(mode, thr, k, s_ref, s_qry):
    """the double whose ceil is common_min: s_ref is the query's size, s_qry the representative's (the reference's names)"""
    jm = _greedy_jm(thr, k)
    if mode == "fast":
        return jm * (2 * s_qry) / (1.0 + jm)  # :1112
    if mode == "containment":
        return jm * min(s_ref, s_qry)  # :1216
    return jm * (s_ref + s_qry) / (1.0 + jm)  # :1218, KSSD :774


def _greedy_dist(c, s_ref, s_qry, k, containment):
    """src/greedy.cpp:1245-1275"""
    if containment:
        m = min(s_ref, s_qry)
        if m == 0:
            return 1.0
        jac = c / m
    else:
        denom = s_ref + s_qry - c
        if denom == 0:
            return 0.0
        jac = c / denom
    if jac >= 1.0:
        return 0.0
    if jac <= 0.0:
        return 1.0
    return min(-math.log(2.0 * jac / (1.0 + jac)) / k, 1.0)


def _greedy_joins(mode, thr, k, c, s_ref, s_qry):
    if c < math.ceil(_greedy_arg(mode, thr, k, s_ref, s_qry)):
        return False
    if mode in ("fast", "kssd"):  # best by common / by Jaccard: no distance test (:1236, :785-794)
        return True
    return _greedy_dist(c, s_ref, s_qry, k, mode == "containment") <= thr  # :1277


def _boundary_thresholds(k):
    out = []
    for x in (0.5, 0.25, 0.75):
        d = -math.log(x) / k
        out += [float(np.nextafter(d, 0.0)), d, float(np.nextafter(d, 1.0))]
    return out


def _boundary_sizes(mode, thr, k, s_rep, lo, hi, take=4):
    """query sizes in [lo, hi) where the ceil's argument is an integer or within an ulp of one: up to `take` of each kind
    (exactly an integer, just above one, just below one)"""
    kinds = {"exact": [], "above": [], "below": []}
    for s in range(lo, hi):
        v = _greedy_arg(mode, thr, k, s, s if mode == "fast" else s_rep)
        r = round(v)
        if r < 2 or abs(v - r) > math.ulp(v):
            continue
        kinds["exact" if v == r else "above" if v > r else "below"].append(s)
    return {kind: sz[:: max(1, len(sz) // take)][:take] for kind, sz in kinds.items()}


@pytest.mark.parametrize("mode", ["fast", "variable", "containment", "kssd"])
def test_greedy_common_min_boundary(ctx, mode):
    from rabbittclust_amd import api
    kssd = mode == "kssd"
    k, dt = (22, np.uint32) if kssd else (21, np.uint64)
    s_rep = 1200
    rng = np.random.default_rng(61)
    pool = np.unique(rng.integers(1, np.iinfo(dt).max, size=8000, dtype=np.uint64).astype(dt))
    rng.shuffle(pool)
    seen = {"exact": 0, "above": 0, "below": 0}
    joined = {-1: 0, 0: 0, 1: 0}
    calls = 0
    for thr in _boundary_thresholds(k):
        lo, hi = (300, 1200) if mode != "fast" else (300, 2000)
        for kind, sizes in _boundary_sizes(mode, thr, k, s_rep, lo, hi).items():
            for s in sizes:
                rep_size = s if mode == "fast" else s_rep
                cm = math.ceil(_greedy_arg(mode, thr, k, s, rep_size))
                rep = np.sort(pool[:rep_size])
                for dc in (-1, 0, 1):
                    c = cm + dc
                    if c < 1 or c > min(s, rep_size):
                        continue
                    q = np.sort(np.concatenate([rep[:c], pool[rep_size:rep_size + s - c]]))
                    sets = [rep, q]
                    dev = api.SketchSet.from_host(sets, ctx.device, k=k, kind="kssd" if kssd else "minhash", width=4 if kssd else 8)
                    if kssd:
                        n_cl, rep_of = ctx.greedy(dev, thr)
                    else:
                        cfg = [rep_size, s] if mode != "fast" else rep_size
                        n_cl, rep_of = ctx.greedy(dev, thr, size_cfg=cfg, is_containment=mode == "containment")
                    want = _greedy_joins("fast" if mode == "fast" else mode, thr, k, c, s, rep_size)
                    assert (n_cl, rep_of.tolist()) == ((1, [0, 0]) if want else (2, [0, 1])), (mode, thr, s, kind, c, cm)
                    joined[dc] += want
                    calls += 1
                seen[kind] += 1
    # every kind of boundary point was met, the rule decided at common_min, and never below it
    assert all(v >= 2 for v in seen.values()), seen
    assert joined[-1] == 0 and joined[0] >= 6 and joined[1] >= 6, (joined, calls)
