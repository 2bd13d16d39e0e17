"""The dendrogram kernels of clust-mst (complete linkage, neighbour joining, UPGMA) where only a large cluster takes them: the
later turns of four loops that every matrix of test_gpu_linkage.py, test_gpu_nj.py and test_gpu_upgma.py (m <= 300) leaves at
their first.

  a. a scan workgroup's rows past the first (agg_scan on the grid path, under either rule): RTC_*_SCAN_BLOCKS of 1, 2 and 3 at small m
  b. the join / merge kernels' reduce of the scan's minima past the first 256: m = 1 030 and 1 300, no switch
  c. lk_wg_kernel's steps 1 and 2 past 1 024 rows and past 1 280
  d. the shipped cap of 1 024 scan workgroups, once per kernel: m = 4 104 and 4 102, no switch
  e. neighbour joining, UPGMA and neighbour joining again on one context, once per path: the two share their kernels' source
     and their host side, and each keeps its own records, counters and path bits

Every comparison is exact, against the restatements or a closed form (tests/dendrogram_sets.py; tests/test_cpu_dendrogram_sets.py
holds the inputs to what is assumed of them here).

What each group is for was tried once on an MI355X with the later turns of one loop dropped, the older three files passing every
time: step 1 or step 2 of lk_wg_kernel kept to x0 < 1024 fails the five linkage cases other than star (c); the reduce kept to
b < 256 fails top_chain(1300), top_group(1030) and top_chain(4104) (b, d) but not the random matrices, which win in low rows;
a grid scan workgroup kept to its first row fails 20 cases of (a) and both of (d); the join / merge launch told of 75 minima, the
most m = 300 uses, fails all four of (b) and top_chain(4104)."""
import functools

import numpy as np
import pytest

from tests import dendrogram_sets as DS
from tests import linkage_sets as LS
from tests import nj_sets as N
from tests import reflinkage as RL
from tests import refnj as RN
from tests import refupgma as RU
from tests import upgma_sets as U

pytestmark = pytest.mark.gpu

GRID = 4
SWITCHES = ("RTC_NJ_GRID_MIN", "RTC_NJ_SCAN_BLOCKS", "RTC_UPGMA_GRID_MIN", "RTC_UPGMA_SCAN_BLOCKS")
# 1: one workgroup walks every row; 2, 3: strides of 8 and 12 rows, and 12 divides no list length that is met
SCAN_BLOCKS = (1, 2, 3)


@pytest.fixture
def switch(ctx, monkeypatch):
    def set_switch(name, v):
        assert name in SWITCHES
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
        ctx.reload_options()
    for name in SWITCHES:
        set_switch(name, None)
    yield set_switch
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


def _nj_tuples(joins):
    return [(int(r["a"]), int(r["b"]), int(r["c"]), float(r["len_a"]), float(r["len_b"]), float(r["len_c"])) for r in joins]


def _first_difference(got, want):
    return [(t, g, w) for t, (g, w) in enumerate(zip(got, want)) if g != w][:2]


def _defaults_hold(ctx):
    from rabbittclust_amd import api
    assert ctx.nj_scan_blocks() == api.NJ_SCAN_BLOCKS == 1024 and ctx.upgma_scan_blocks() == api.UPGMA_SCAN_BLOCKS == 1024


# ---- a. scan rows past one grid, at small m --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _upgma_sets():
    return {name: (Sm, w) for name, Sm, w in U.dev_sets()}


@functools.lru_cache(maxsize=None)
def _upgma_want(name):
    Sm, w = _upgma_sets()[name]
    return RU.rowcache(Sm, w)[0]  # test_cpu_upgma.py holds it to the naive scan on every set


@pytest.mark.parametrize("name", [name for name, _, _ in U.dev_sets()])
def test_upgma_scan_workgroups_take_further_rows(ctx, switch, name):
    Sm, w = _upgma_sets()[name]
    m, want = len(Sm), _upgma_want(name)
    arr = np.array(Sm, dtype=np.uint64)
    switch("RTC_UPGMA_GRID_MIN", 4)
    for nb in SCAN_BLOCKS:
        switch("RTC_UPGMA_SCAN_BLOCKS", nb)
        assert ctx.upgma_scan_blocks() == nb  # the switch took hold: a misspelt name would leave 1024 and the test vacuous
        got = RU.as_tuples(ctx.upgma(arr, w))
        assert got == want, (name, nb, _first_difference(got, want))
        c = ctx.upgma_counters()
        assert c["merges"] == m - 1
        if m >= 4:
            assert c["paths"] == GRID and c["grid_components"] == 1, (name, nb, c)
    switch("RTC_UPGMA_SCAN_BLOCKS", None)
    _defaults_hold(ctx)


def test_scan_switches_are_clamped(ctx, switch):
    for given, held in ((0, 1), (-5, 1), (1, 1), (1024, 1024), (1025, 1024), (1 << 40, 1024)):
        switch("RTC_NJ_SCAN_BLOCKS", given)
        switch("RTC_UPGMA_SCAN_BLOCKS", given)
        assert (ctx.nj_scan_blocks(), ctx.upgma_scan_blocks()) == (held, held), given
    switch("RTC_NJ_SCAN_BLOCKS", 7)
    assert (ctx.nj_scan_blocks(), ctx.upgma_scan_blocks()) == (7, 1024)  # each its own
    switch("RTC_NJ_SCAN_BLOCKS", None)
    switch("RTC_UPGMA_SCAN_BLOCKS", None)
    _defaults_hold(ctx)


@functools.lru_cache(maxsize=None)
def _nj_want_case(name, m):
    return RN.nj(N.case(name, m))


@functools.lru_cache(maxsize=None)
def _nj_want_additive(m):
    return RN.nj(N.additive(m)[0])


def _nj_on_few_scan_workgroups(ctx, switch, D, want, what):
    m = len(D)
    switch("RTC_NJ_GRID_MIN", 4)
    for nb in SCAN_BLOCKS:
        switch("RTC_NJ_SCAN_BLOCKS", nb)
        assert ctx.nj_scan_blocks() == nb
        got = _nj_tuples(ctx.nj(D))
        assert RN.bits(got) == RN.bits(want), (what, nb, _first_difference(got, want))
        c = ctx.nj_counters()
        assert c["paths"] == GRID and c["grid_components"] == 1 and c["records"] == m - 2, (what, nb, c)
    switch("RTC_NJ_SCAN_BLOCKS", None)
    _defaults_hold(ctx)


@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_nj_scan_workgroups_take_further_rows(ctx, switch, name):
    for m in N.CASE_SIZES:
        _nj_on_few_scan_workgroups(ctx, switch, N.case(name, m), _nj_want_case(name, m), (name, m))


@pytest.mark.parametrize("m", [m for m in N.ADDITIVE_SIZES if m >= 5])
def test_nj_scan_workgroups_take_further_rows_additive(ctx, switch, m):
    D, tree = N.additive(m)
    want = _nj_want_additive(m)
    assert RN.splits(want, m) == tree
    _nj_on_few_scan_workgroups(ctx, switch, D, want, ("additive", m))


# ---- b. the minima reduce past 256 -----------------------------------------------------------------------------------------------
def test_upgma_reduce_past_256_minima_chain(ctx, switch):
    """top_chain(1300): 275 steps win in scan workgroups 256 to 324, which the merge kernel's lanes reach on their second turn"""
    m = DS.CHAIN_M
    got = RU.as_tuples(ctx.upgma(DS.top_chain(m)))
    want = DS.top_chain_records(m)
    assert got == want, _first_difference(got, want)
    assert ctx.upgma_counters()["paths"] == GRID
    _defaults_hold(ctx)


def test_upgma_reduce_past_256_minima_random_ties(ctx, switch):
    m = DS.REDUCE_M
    Sm = U.random_ties(m)
    want = RU.rowcache(Sm)[0]
    got = RU.as_tuples(ctx.upgma(np.array(Sm, dtype=np.uint64)))
    assert got == want, _first_difference(got, want)
    assert ctx.upgma_counters()["paths"] == GRID


def test_nj_reduce_past_256_minima_top_group(ctx, switch):
    """top_group(1030): the first five joins win at list positions 1 024 and up, scan workgroup 256"""
    m, g = DS.REDUCE_M, DS.GROUP
    D = DS.top_group(m)
    want = RN.nj(D)
    assert all(a >= m - g and b >= m - g for a, b, *_ in want[:g - 1]) and (m - g) // 4 >= 256  # the input's side, before the device is asked
    got = _nj_tuples(ctx.nj(D))
    assert RN.bits(got) == RN.bits(want), _first_difference(got, want)
    c = ctx.nj_counters()
    assert c["paths"] == GRID and c["records"] == m - 2
    _defaults_hold(ctx)


def test_nj_reduce_past_256_minima_additive(ctx, switch):
    m = DS.REDUCE_M
    D, tree = N.additive(m)
    want = RN.nj(D)
    assert RN.splits(want, m) == tree
    got = _nj_tuples(ctx.nj(D))
    assert RN.bits(got) == RN.bits(want), _first_difference(got, want)
    assert RN.splits(got, m) == tree and ctx.nj_counters()["paths"] == GRID


# ---- c. complete linkage past 1 024 and 1 280 rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,m,seed,bounded", DS.LINKAGE_CASES, ids=["%s_%d" % (c[0], c[1]) for c in DS.LINKAGE_CASES])
def test_linkage_workgroup_kernel_past_1024_rows(ctx, case, m, seed, bounded):
    keys = DS.linkage_keys(case, m, seed)
    for kmin in ((0, 1),) + ((LS.median_bound(keys),) if bounded else ()):
        want, rescans = RL.rowbest(keys, kmin)
        # the input's side: a merge whose lower row is past the first turn of step 1, and for random_ties at 1 300 past slot 0
        if case != "star":
            assert any(a >= 1024 for a, *_ in want), (case, m, kmin)
        if (case, m) == ("random_ties", 1300):
            assert any(a >= 1280 for a, *_ in want), kmin
        got = [tuple(int(v) for v in r) for r in ctx.linkage(keys, kmin).tolist()]
        assert got == want, (case, m, kmin, _first_difference(got, want))
        c = ctx.linkage_counters()
        assert c["merges"] == len(want) and c["rescans"] == rescans, (case, m, kmin, c["rescans"], rescans)
        assert (c["wave_components"], c["workgroup_components"], c["largest_m"]) == (0, 1, m)
        if kmin != (0, 1):
            assert 0 < len(got) < m - 1
        elif case == "star":
            assert [(a, b) for a, b, *_ in got] == [(0, j) for j in range(1, m)] and rescans == (m - 1) * m // 2
        elif case in ("tie_free", "near_2_31"):
            assert len(got) == m - 1 and got[-1][4] == m


# ---- d. the shipped cap of 1 024 scan workgroups ---------------------------------------------------------------------------------
def test_upgma_scan_past_the_shipped_cap(ctx, switch):
    """top_chain(4104), all 4 103 records against the closed form.  The first seven steps win in row r - 2 >= 4 096 of the list,
    which a scan workgroup reaches only on its second pass (p += 4 * 1024); every step down to r = 1 026 wins past the reduce's
    first turn."""
    m = DS.CAP_UPGMA_M
    got = RU.as_tuples(ctx.upgma(DS.top_chain(m)))
    want = DS.top_chain_records(m)
    assert len(got) == m - 1 and got == want, _first_difference(got, want)
    assert ctx.upgma_counters()["paths"] == GRID
    _defaults_hold(ctx)


def test_nj_scan_past_the_shipped_cap(ctx, switch):
    """top_group(4102): the first five joins are inside the group, at list positions 4 096 and up, which a scan workgroup reaches
    only on its second pass; they are compared on bits with the restatement cut short.  The records of r <= 4 097 come from the
    single-pass scan that the tests above pin at m = 1 030 and below, and the restatement would take minutes on them: they are
    not compared, only counted and checked for retiring every index exactly once."""
    m, g = DS.CAP_NJ_M, DS.GROUP
    D = DS.top_group(m)
    assert DS.on_grid_64(D)  # what lets the restatement form R with numpy's sums
    want = RN.nj(D, steps=g - 1, exact_sums=True)
    assert len(want) == g - 1 and all(a >= 4096 and b >= 4096 for a, b, *_ in want)
    got = _nj_tuples(ctx.nj(D))
    assert RN.bits(got[:g - 1]) == RN.bits(want), _first_difference(got, want)
    assert len(got) == m - 2
    c = ctx.nj_counters()
    assert c["paths"] == GRID and c["records"] == m - 2
    alive = set(range(m))
    for a, b, cc, *_ in got[:-1]:
        assert a < b and a in alive and b in alive and cc == RN.NONE, (a, b, cc)
        alive.remove(b)
    a, b, cc, *_ = got[-1]
    assert a < b < cc and alive == {a, b, cc}
    _defaults_hold(ctx)


# ---- e. the two methods in turn on one context -----------------------------------------------------------------------------------
# Neighbour joining and UPGMA run one skeleton (rtc_agglom.h) under two rules.  m = 3: NJ's closing record alone; 5, 64: the wave
# path; 65: the workgroup path; 9 with the switches at 4 and 1: the grid path, one scan workgroup walking every row.
WAVE, WORKGROUP = 1, 2
IN_TURN = ((3, False, WAVE), (5, False, WAVE), (64, False, WAVE), (65, False, WORKGROUP), (9, True, GRID))


@functools.lru_cache(maxsize=None)
def _in_turn_inputs(m):
    D = N.case("random_ties", m) if m >= 5 else N.additive(m)[0]
    Sm = DS.top_chain(m)
    want_up = RU.rowcache(Sm.tolist())[0]
    assert want_up == DS.top_chain_records(m)  # the restatement and the closed form agree before the device is asked
    return D, RN.nj(D), Sm, want_up


def _without_times(c):
    return {k: v for k, v in c.items() if not k.endswith("_ns")}


@pytest.mark.parametrize("m,on_grid,path", IN_TURN, ids=["m%d_path%d" % (m, p) for m, _, p in IN_TURN])
def test_nj_and_upgma_in_turn_on_one_context(ctx, switch, m, on_grid, path):
    D, want_nj, Sm, want_up = _in_turn_inputs(m)
    if on_grid:
        for name in ("RTC_NJ_GRID_MIN", "RTC_UPGMA_GRID_MIN"):
            switch(name, 4)
        for name in ("RTC_NJ_SCAN_BLOCKS", "RTC_UPGMA_SCAN_BLOCKS"):
            switch(name, 1)
        assert (ctx.nj_scan_blocks(), ctx.upgma_scan_blocks()) == (1, 1)
    components = {"wave_components": int(path == WAVE), "workgroup_components": int(path == WORKGROUP), "grid_components": int(path == GRID)}
    nj_own = dict(components, components=1, records=max(m - 2, 1), batches=1, paths=path)
    up_own = dict(components, components=1, merges=m - 1, row_rescans=0, paths=path)

    first = ctx.nj(D)
    c_first = ctx.nj_counters()
    assert RN.bits(_nj_tuples(first)) == RN.bits(want_nj), _first_difference(_nj_tuples(first), want_nj)
    assert _without_times(c_first) == nj_own

    got_up = RU.as_tuples(ctx.upgma(Sm))
    c_up = ctx.upgma_counters()
    assert got_up == want_up, _first_difference(got_up, want_up)
    assert _without_times(c_up) == up_own
    assert ctx.nj_counters() == c_first  # the UPGMA call left neighbour joining's counters alone, times included

    second = ctx.nj(D)
    assert second.tobytes() == first.tobytes()  # every field of every record, the padding too
    assert RN.bits(_nj_tuples(second)) == RN.bits(want_nj)
    assert _without_times(ctx.nj_counters()) == nj_own
    assert ctx.upgma_counters() == c_up  # and the other way round
