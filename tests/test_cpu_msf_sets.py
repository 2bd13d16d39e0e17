"""CPU suite: the graphs of tests/msf_sets.py and the reference of tests/refmsf.py, checked without a GPU.

The reference's double keys are tied to exact rationals (forest_exact) and to the numpy restatement of the round primitives
(test_cpu_distributed.NumpyBoruvkaBackend under pipeline.boruvka_rounds, fused and three-pass); on sketch-made sets it gives
oracle.mst's distances.  Every case is shown to hold what it is for.  A restatement of the kernels' round (`model`: minimum per
component, hook, relabel) equals the reference on every case as it stands, and differs from it on named cases once one of the
mistakes the GPU suite has to catch is put into it."""
import numpy as np
import pytest

import msf_sets as S
import refmsf

NUM_CU = 256
SMALL = [name for name in S.names() if S.case(name)[0] <= 5000 and len(S.case(name)[1]) <= 50_000]


def _triples(a):
    return sorted(map(tuple, np.asarray(a).reshape(-1, 3).tolist()))


def _want(name):
    n, e, lens, wmode = S.case(name)
    return refmsf.sorted_list(e, lens, wmode) if name in S.IS_FOREST else refmsf.forest(n, e, lens, wmode)


# ---- the restatement of a round, with room for a mistake ----------------------------------------------------------------------
def _fused_size(n, lens):
    """the common size when all sizes are equal and the fused key fits, else 0 (rtc_msf_dev's choice)"""
    if n < 2 or int(lens.min()) != int(lens.max()) or int(lens[0]) == 0:
        return 0
    b, w = S.key_bits(n, int(lens[0]))
    return int(lens[0]) if w + 2 * b <= 63 else 0


def model(n, edges, lens, wmode, mutation=None, stop_after=None):
    """Boruvka as the kernels run it.  Returns (records in the order the hook pass appends them -- round by round, by the id
    of the root that records --, rounds, comp, succ of the last round run), or None when the successors form a cycle.
    mutation: "position" / "ji": ties broken by list position / by (j, i); "larger_root": the larger root kept on a mutual
    hook; "fifth": of the components the on-lanes of 64 consecutive entries name, the fifth is ignored; "narrow": the fused
    key packed with one index bit too few, so that fields of edges with equal low id bits run into each other and the
    count and the ids come out of the mix."""
    e = np.asarray(edges).reshape(-1, 3).astype(np.int64)
    i, j, c = e[:, 0], e[:, 1], e[:, 2]
    m = len(e)
    key = refmsf.keys(e, lens, wmode)
    ti, tj, tc = i, j, c  # what a chosen entry is decoded to
    if mutation == "position":
        perm = np.lexsort((np.arange(m), key))
    elif mutation == "ji":
        perm = np.lexsort((i, j, key))
    elif mutation == "narrow":
        s = _fused_size(n, np.asarray(lens))
        assert s, "the fused key only"
        b = S.key_bits(n, s)[0] - 1
        fused = ((s - c) << (2 * b)) | (i << b) | j
        perm = np.argsort(fused, kind="stable")
        ti, tj, tc = (fused >> b) & ((1 << b) - 1), fused & ((1 << b) - 1), s - (fused >> (2 * b))
    else:
        perm = np.lexsort((j, i, key))
    rank = np.empty(m, dtype=np.int64)
    rank[perm] = np.arange(m)
    comp = np.arange(n, dtype=np.int64)
    succ = comp.copy()
    raw, rounds = [], 0
    while rounds < 64:
        ci, cj = comp[i], comp[j]
        cross = ci != cj
        best = np.full(n, m, dtype=np.int64)
        if mutation == "fifth":
            for w0 in range(0, m, 64):
                for side in (ci, cj):
                    seen = []
                    for lane in range(w0, min(w0 + 64, m)):
                        if cross[lane]:
                            if side[lane] not in seen:
                                seen.append(side[lane])
                            if seen.index(side[lane]) != 4:
                                best[side[lane]] = min(best[side[lane]], rank[lane])
        else:
            np.minimum.at(best, ci[cross], rank[cross])
            np.minimum.at(best, cj[cross], rank[cross])
        roots = np.nonzero(best < m)[0]
        pick = perm[best[roots]]
        a, b = comp[ti[pick]], comp[tj[pick]]
        d = np.where(a == roots, b, a)
        other = np.full(n, -1, dtype=np.int64)
        other[roots] = d
        mutual = other[d] == roots
        keep = mutual & ((roots > d) if mutation == "larger_root" else (roots < d))
        succ = np.arange(n, dtype=np.int64)
        succ[roots] = np.where(keep, roots, d)
        rec = keep | ~mutual
        raw += list(zip(ti[pick][rec].tolist(), tj[pick][rec].tolist(), tc[pick][rec].tolist()))
        rounds += 1
        if not rec.any():
            break
        to = succ.copy()
        for _ in range(40):
            nxt = to[to]
            if np.array_equal(nxt, to):
                break
            to = nxt
        else:
            return None
        if not np.array_equal(succ[to], to):  # (a 2-cycle looks settled after one jump)
            return None
        comp = to[comp]
        if stop_after == rounds:
            break
    return raw, rounds, comp, succ


def _differs(name, mutation):
    n, e, lens, wmode = S.case(name)
    got = model(n, e, lens, wmode, mutation)
    return got is None or _triples(got[0]) != _triples(_want(name)) or got[1] != refmsf.rounds(n, e, lens, wmode)


@pytest.mark.parametrize("name", S.names())
def test_the_round_model_equals_the_reference(name):
    n, e, lens, wmode = S.case(name)
    raw, rounds, _, _ = model(n, e, lens, wmode)
    want = _want(name)
    got = np.array(raw, dtype=np.int64).reshape(-1, 3)
    got = got[refmsf.order(got, lens, wmode)] if len(got) else got
    assert np.array_equal(got, want)
    assert rounds == refmsf.rounds(n, e, lens, wmode)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_double_keys_order_as_the_exact_rationals(name):
    n, e, lens, wmode = S.case(name)
    assert int(lens.max()) < 1 << 26
    assert np.array_equal(refmsf.forest(n, e, lens, wmode), refmsf.forest_exact(n, e, lens, wmode))


def _backend(n, e, lens, wmode):
    from test_cpu_distributed import NumpyBoruvkaBackend
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (its own keys divide by a denom of 0; replaced below)
        b = NumpyBoruvkaBackend(e.astype(np.int64), lens, (wmode & 3) == 1, n)
    b.key = refmsf.keys(e, lens, wmode)  # every weight mode, and J = 0 where the denom is 0
    return b


@pytest.mark.parametrize("name", SMALL)
def test_forest_equals_the_numpy_round_primitives(name):
    from rabbittclust_amd import pipeline
    n, e, lens, wmode = S.case(name)
    want, want_rounds = _triples(_want(name)), refmsf.rounds(n, e, lens, wmode)
    forms = [0] + ([_fused_size(n, lens)] if _fused_size(n, lens) else [])
    for s_fixed in forms:
        sel, rounds = pipeline.boruvka_rounds(_backend(n, e, lens, wmode), n, None, s_fixed)
        got = sorted(zip(sel["i"].tolist(), sel["j"].tolist(), sel["common"].tolist()))
        assert got == want, (name, s_fixed)
        assert rounds == want_rounds, (name, s_fixed)


@pytest.mark.parametrize("containment", [False, True])
def test_forest_of_sketch_made_lists_gives_the_oracles_distances(oracle, containment):
    """the sets of test_cpu_oracle.test_oracle_mst_against_bruteforce_kruskal and of test_cpu_distributed"""
    from test_cpu_distributed import _make_sketches
    rng = np.random.default_rng(4)
    pool = np.unique(rng.integers(1, 1 << 60, size=900, dtype=np.uint64))
    sets = [[np.sort(rng.choice(pool, size=int(rng.integers(0, 120)), replace=False)) for _ in range(61)],
            _make_sketches(77, 90), _make_sketches(77, 90, 120)]
    for sk in sets:
        n = len(sk)
        radio = oracle.lib().orc_mst_radio(0.05, 21)
        lens = np.array([len(s) for s in sk], dtype=np.uint32)
        edges = []
        for i in range(n):
            for j in range(i):
                c = len(np.intersect1d(sk[i], sk[j]))
                if c and max(lens[i], lens[j]) <= radio * min(lens[i], lens[j]):
                    edges.append((i, j, c))
        f = refmsf.forest(n, np.array(edges, dtype=np.int32).reshape(-1, 3), lens, int(containment))
        dist = [oracle.lib().orc_mst_distance(int(c), int(lens[i]), int(lens[j]), 21, int(containment)) for i, j, c in f.tolist()]
        flat, start, ln = oracle.to_csr(sk)
        want = oracle.mst(flat, start, ln, 21, containment, 0.05, threads=1)
        assert np.array_equal(np.sort(np.array(dist)).view(np.uint64), np.sort(want["dist"]).view(np.uint64))


# ---- every case holds what it is for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.names())
def test_lists_are_well_formed(name):
    n, e, lens, wmode = S.case(name)
    assert e.dtype == np.int32 and e.shape == (len(e), 3) and lens.dtype == np.uint32 and lens.shape == (n,)
    if len(e):
        i, j, c = (e[:, q].astype(np.int64) for q in range(3))
        assert (i > j).all() and (j >= 0).all() and (i < n).all() and (c >= 0).all()
        top = np.minimum(lens[i], lens[j]).astype(np.int64)
        assert (c <= (np.minimum(top, wmode >> 2) if (wmode & 3) == 2 else top)).all()
        assert len(np.unique(i * n + j)) == len(e), "a pair twice"


@pytest.mark.parametrize("name", ["chain", "chain_var"])
def test_chain_is_one_successor_chain(name):
    n, e, lens, wmode = S.case(name)
    assert n == 20_000 and refmsf.rounds(n, e, lens, wmode) == 2
    succ = model(n, e, lens, wmode, stop_after=1)[3]
    v = np.arange(n)
    assert np.array_equal(succ[:n - 2], v[:n - 2] + 1) and succ[n - 2] == n - 2 and succ[n - 1] == n - 2
    assert int((succ != v).sum()) == n - 1  # every vertex but the root hooks; the walk from vertex 0 has n - 2 links


def test_ruler_rounds_cross_the_groups():
    for name in ("ruler", "ruler_var"):
        n, e, lens, wmode = S.case(name)
        assert n == 4097 and refmsf.rounds(n, e, lens, wmode) == 13
    got = [refmsf.rounds(*S.case("ruler_%d" % n)) for n in S.RULER_SMALL]
    assert got == [2, 3, 4, 5]  # the round that finds nothing: the second of the first group, then each of the three places of the next


@pytest.mark.parametrize("name", ["star_equal", "star_equal_var", "star_distinct", "star_distinct_var"])
def test_star_has_both_ends_of_the_pooling(name):
    n, e, lens, wmode = S.case(name)
    assert n == 5000 and len(e) == n - 1 and ((e[:, 0] == S.STAR_HUB) | (e[:, 1] == S.STAR_HUB)).all()
    assert (e[:, 0] == S.STAR_HUB).sum() == S.STAR_HUB and refmsf.rounds(n, e, lens, wmode) == 2
    distinct = len(np.unique(refmsf.keys(e, lens, wmode)))
    assert distinct == (n - 1 if "distinct" in name else 1)
    if "equal" in name:
        raw = model(n, e, lens, wmode)[0]
        hub = [r for r in raw if r[:2] == (S.STAR_HUB, 0)]
        assert len(hub) == 1  # the hub's own choice is the smallest id pair, and vertex 0 picked the same edge
    assert ("var" in name) == (int(lens.min()) != int(lens.max()))


@pytest.mark.parametrize("name", ["pooling", "pooling_var"])
def test_pooling_waves_name_four_five_and_many_components(name):
    n, e, lens, wmode = S.case(name)
    first_bridge = S.pooling()[1]
    comp = model(n, e, lens, wmode, stop_after=1)[2]
    assert len(np.unique(comp)) == n // S.POOL_CLIQUE and all(len(np.unique(comp[q:q + 8])) == 1 for q in range(0, n, 8))
    seen = {0: [], 1: []}
    for w0 in range(first_bridge, len(e), 64):
        for side in (0, 1):
            c = comp[e[w0:w0 + 64, side]]
            on = comp[e[w0:w0 + 64, 0]] != comp[e[w0:w0 + 64, 1]]
            assert on.all()
            seen[side].append(len(np.unique(c)))
    for side in (0, 1):
        assert seen[side][:3] == [4, 4, 4]
        assert any(k in (5, 6) for k in seen[side]) and max(seen[side]) >= 10
    assert np.array_equal(_want(name), _want(name.replace("pooling", "pooling_shuffled")))


def test_complete_graphs_pass_one_and_two_turns():
    turn = S.turn(NUM_CU)
    assert turn == 524_288 and S.complete_size(NUM_CU, 1) == 1100 and S.complete_size(NUM_CU, 2) == 1500
    for name, m, keys_at_most in (("k_one_turn", 604_450, 10), ("k_one_turn_var", 604_450, 20), ("k_two_turns_var", 1_124_250, 20)):
        n, e, lens, wmode = S.case(name)
        assert len(e) == m and (m > 2 * turn if "two" in name else turn < m <= 2 * turn)
        assert len(np.unique(refmsf.keys(e, lens, wmode))) <= keys_at_most  # ties abound
    n, e, lens, wmode = S.case("k300_equal")
    assert np.array_equal(_want("k300_equal"), np.array([(v, 0, 40) for v in range(1, 300)]))
    for cu in (304, 128):  # another device: still past its turns
        assert S.complete_size(cu, 1) * (S.complete_size(cu, 1) - 1) // 2 > S.turn(cu)
        assert S.complete_size(cu, 2) * (S.complete_size(cu, 2) - 1) // 2 > 2 * S.turn(cu)


@pytest.mark.parametrize("name", ["ratios_mode0", "ratios_mode1", "ratios_s_below", "ratios_s_inside", "ratios_s_above"])
def test_ratio_cases_tie_doubles_of_different_counts(name):
    """at least half the edges share their key with an edge of another count: the counts aim at seven ratios wherever the two
    sizes allow one of them (measured 0.80 and above)"""
    n, e, lens, wmode = S.case(name)
    key, d, c = refmsf.keys(e, lens, wmode), refmsf.denoms(e, lens, wmode), e[:, 2].astype(np.int64)
    tied = 0
    for k in np.unique(key):
        at = key == k
        if len(np.unique(c[at])) > 1:
            tied += int(at.sum())
    print(name, "tied share %.3f" % (tied / len(e)))
    if name == "ratios_s_below":  # every denom is s = 3: equal doubles have equal counts here, and there are three doubles in all
        assert (d == 3).all() and len(np.unique(key)) == 3
    else:
        assert tied >= len(e) // 2
    if (wmode & 3) == 2:
        s, u = wmode >> 2, lens[e[:, 0]].astype(np.int64) + lens[e[:, 1]] - c
        where = {"below": (u > s).all(), "inside": (u > s).any() and (u < s).any(), "above": (u < s).all()}
        assert where[name.rsplit("_", 1)[1]]


@pytest.mark.parametrize("name", ["zeros_mode0", "zeros_mode1"])
def test_zero_cases_hold_their_zeros(name):
    n, e, lens, wmode = S.case(name)
    d, c = refmsf.denoms(e, lens, wmode), e[:, 2]
    assert (d == 0).sum() >= 3 and (c == 0).sum() >= len(e) // 5
    assert (refmsf.keys(e, lens, wmode)[c == 0] == refmsf.KEY_ONE).all()
    touched = np.zeros(n, dtype=bool)
    touched[e[:, 0]] = touched[e[:, 1]] = True
    assert (~touched).sum() >= 9 and touched[(~touched).nonzero()[0][0] + 1:].any()  # isolated vertices among connected ones
    assert n - len(_want(name)) >= 3 + 9  # several components
    assert [refmsf.rounds(*S.case(k)) for k in ("empty", "pair_without", "pair_with")] == [1, 1, 2]


def test_layout_cases_sit_on_both_sides_of_63_bits():
    from rabbittclust_amd import _lib
    lib = _lib.load()
    for n, var in ((65536, False), (65537, False), (65536, True), (65537, True)):
        name = "layout_%d%s" % (n, "_var" if var else "")
        _, e, lens, wmode = S.case(name)
        b, w = S.key_bits(n, int(lens.max()))
        assert w == 31 and b == (16 if n == 65536 else 17) and (w + 2 * b == 63 if n == 65536 else w + 2 * b > 63)
        assert (int(lens.min()) != int(lens.max())) == var and int(lens.min()) >= 1 << 30 and int(lens.max()) < 1 << 31
        if not var:
            assert int(lens[0]) == (1 << 30) + 5 and lib.rtc_boruvka_key_bits(n, int(lens[0])) == (16 if n == 65536 else 0)
        assert 200_000 < len(e) <= 300_000 and (e[:, 0] == n - 1).sum() >= 40
        top = np.minimum(lens[e[:, 0]], lens[e[:, 1]]).astype(np.int64)
        assert (e[:, 2] <= 3).sum() > len(e) // 4 and (top - e[:, 2] <= 3).sum() > len(e) // 4 and (e[:, 2] == 0).any() and (e[:, 2] == top).any()


def test_forest_case_is_a_forest_past_one_turn():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n, e, lens, wmode = S.case("forest")
    assert n == 600_000 and n > S.turn(NUM_CU) and S.forest_size(304) > S.turn(304)
    parts = connected_components(coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)[0]
    assert parts == n - len(e) and 0.005 * n < parts < 0.015 * n
    assert len(np.unique(refmsf.keys(e, lens, wmode))) < len(e) // 20  # the order within equal keys is the sort's to get right


# ---- the sets tell wrong kernels from right ones ----------------------------------------------------------------------------------
_TELLS = {
    "position": ["k300_equal", "ratios_mode1", "zeros_mode0", "layout_65537"],
    "ji": ["pooling", "ratios_mode0", "zeros_mode1", "layout_65536"],
    "fifth": ["pooling", "pooling_var", "star_equal"],
    "narrow": ["star_distinct", "k300_equal", "layout_65536"],
}


@pytest.mark.parametrize("mutation", sorted(_TELLS))
def test_a_wrong_rule_changes_the_forest_or_the_rounds(mutation):
    for name in _TELLS[mutation]:
        assert _differs(name, mutation), (mutation, name)


def test_the_larger_root_on_a_mutual_hook_changes_what_the_hook_pass_leaves():
    """Which of two roots that picked each other stays the root changes neither the edges chosen nor the rounds -- the labels
    name the same partition -- so the sorted forest cannot tell; what the hook pass appends can: the recording root's id
    places the record.  On hook_order (one workgroup, so the order is the ids') the records come out in another order, and
    the GPU suite compares that order on the cases of one workgroup."""
    n, e, lens, wmode = S.case("hook_order")
    right, wrong = model(n, e, lens, wmode), model(n, e, lens, wmode, "larger_root")
    assert right[0] == [(2, 0, 9), (1, 0, 4)] and wrong[0] == [(1, 0, 4), (2, 0, 9)]
    from rabbittclust_amd import pipeline
    sel, _ = pipeline.boruvka_rounds(_backend(n, e, lens, wmode), n, None, 0)
    assert list(zip(sel["i"].tolist(), sel["j"].tolist(), sel["common"].tolist())) == right[0]
    for name in ("pooling", "ratios_mode0", "ruler_17"):
        assert not _differs(name, "larger_root")
