"""GPU suite: rtc_rep_screen against the restatement of its definition (tests/refscreen.py) on the sets of
tests/screen_edge_sets.py, where the one generated set of tests/test_gpu_screen.py never takes its kernels:

  a. winners that retire more positions than a workgroup has lanes (the later turns of the retire loop), on each gather path, and
     positions held by dozens of candidates
  b. a sample at each side of each path boundary, round 1 won by the last candidate, the path counters pinned
  c. the fill pass at each side of SCREEN_SHORT_RUN and of a wave's 64 records, long runs in lanes 63 and 0, in a whole wave, of
     two samples in one wave, at the last position of a partial wave
  d. 600 samples, with chunks of no hash, of no match and of no candidate between chunks that have hits, and a halved call
  e. every threshold decided by the equal case, empty and retired representatives
  f. the hashes at the ends of both widths, and 64-bit hashes that agree in one half

Every comparison is equality of integer tuples; tests/test_cpu_screen_edges.py holds each set to what is assumed of it here.

What each group is for was tried once on an MI355X, on copies of the library with one computed value changed (no index, bound
or address), this file and tests/test_gpu_screen.py (without its end-to-end case) run under each:
  1. the retire loop of screen_gather_kernel stopped after its first turn (j < min(cw, B)): all eight cases of (a) and both of
     (c) fail; tests/test_gpu_screen.py passes whole -- no winner there has more positions than a wave has lanes
  2. the argmax tie broken towards the higher index: the workgroup and global builds of (a), whose fillers tie, and (b), (c),
     (d) and (f) fail, the wave and nested builds of (a) and the hand-sized (e) have no tie and pass; the older file fails too
  3. > for >= in the containment test of screen_elig_kernel: (e) fails at "quarter" (8 of 32) and "whole" (5 of 5), and (c) and
     (d) fail; the older file fails as well, in its second configuration (a quarter), so it was not blind here
  4. a run of exactly SCREEN_SHORT_RUN records sent down the wave route (< for <= in the lane route, >= in the ballot): every
     case of both files passes, the two routes write the same records; the lane route then made to write position 0 into its
     last record's mpos: every case of both files fails
A fifth change, the two searches of screen_count_kernel comparing the high words alone, failed test_extreme_hashes[8] and left
every other width-8 case of this file passing."""
import pytest

import refscreen as R
import screen_edge_sets as E

pytestmark = pytest.mark.gpu

CHUNKS = (0, 3)
_SETS = {}


def _device_set(ctx, group, name, width):
    """(the set on the device, the number of representatives, live): uploaded once per (set, width)"""
    from rabbittclust_amd import api
    key = (group, name, width)
    if key not in _SETS:
        reps, samples, live = E.the_set(group, name)
        if group == "extremes":
            arrays = E.extremes_arrays(reps + samples, width)
        else:
            arrays = E.as_width(reps + samples, width, monotone=(group == "fill"))  # the fill set's positions are part of the case
        _SETS[key] = (api.SketchSet.from_host(arrays, ctx.device, k=21, kind="kssd", width=width), len(reps), live)
    return _SETS[key]


def _tuples(a):
    return [tuple(int(x) for x in r) for r in a]


def _first_difference(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3], len(got), len(want)


def _check(ctx, dev, ref, config, chunk=0, forced=False):
    """one call against the reference's (hits, sums, info): the hits, the sums and every counter the reference can give"""
    sk, n_reps, live = dev
    hits, sums, info = ref
    want_hits, want_sums = R.flat(hits), [s + (0,) for s in sums]
    got_hits, got_sums = ctx.rep_screen(sk, n_reps, *config, live=live, query_chunk=chunk)
    assert _tuples(got_sums) == want_sums, (config, chunk, _first_difference(_tuples(got_sums), want_sums))
    assert _tuples(got_hits) == want_hits, (config, chunk, _first_difference(_tuples(got_hits), want_hits))
    cnt = ctx.rep_screen_counters()
    nq = len(sums)
    with_cand = sum(1 for s in sums if s[3])
    assert cnt["chunks"] == (1 if chunk == 0 else (nq + chunk - 1) // chunk)
    assert cnt["wave_queries"] + cnt["workgroup_queries"] + cnt["global_queries"] == with_cand
    assert cnt["eligible"] == len(want_hits) and cnt["picks"] == sum(s[4] for s in sums) and cnt["candidates"] >= cnt["eligible"]
    assert cnt["rounds_max"] == max(i["rounds"] for i in info) and cnt["matches"] == sum(i["matches"] for i in info)
    if forced:
        assert cnt["wave_queries"] == cnt["workgroup_queries"] == 0 and cnt["global_queries"] == with_cand
    return cnt


def _forced_global(ctx, dev, ref, config):
    from rabbittclust_amd import api
    with ctx.env(RTC_SCREEN_GLOBAL="1"):
        _check(ctx, dev, ref, config, forced=True)
        assert ctx.rep_screen_last_path() == (api.SCREEN_PATH_GLOBAL if any(s[3] for s in ref[1]) else 0)


# ---- a ----
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", ["wave", "workgroup", "global", "nested"])
def test_wide_winners_on_every_path(ctx, name, width):
    from rabbittclust_amd import api
    dev = _device_set(ctx, "wide", name, width)
    path = {"wave": api.SCREEN_PATH_WAVE, "nested": api.SCREEN_PATH_WAVE, "workgroup": api.SCREEN_PATH_BLOCK, "global": api.SCREEN_PATH_GLOBAL}[name]
    for config in E.WIDE_CONFIGS:
        ref = E.reference("wide", name, config)
        for chunk in CHUNKS:
            _check(ctx, dev, ref, config, chunk)
        if config == E.WIDE_CONFIGS[0]:
            assert ctx.rep_screen_last_path() == path
    _forced_global(ctx, dev, E.reference("wide", name, E.WIDE_CONFIGS[0]), E.WIDE_CONFIGS[0])


# ---- b ----
@pytest.mark.parametrize("width", [4, 8])
def test_exact_path_boundaries(ctx, width):
    _, block, _ = E.constants()
    dev = _device_set(ctx, "boundaries", None, width)
    config = (1, 0, 1, 0)
    ref = E.reference("boundaries", None, config)
    for chunk in CHUNKS:
        cnt = _check(ctx, dev, ref, config, chunk)
        assert (cnt["wave_queries"], cnt["workgroup_queries"], cnt["global_queries"]) == (6, 3, 1), "a sample went to another launch than the header says"
        assert cnt["rounds_max"] == block + 1
    _forced_global(ctx, dev, ref, config)
    for max_picks in E.boundary_picks():
        config = (1, 0, 1, max_picks)
        cnt = _check(ctx, dev, E.reference("boundaries", None, config), config)
        assert (cnt["wave_queries"], cnt["workgroup_queries"], cnt["global_queries"]) == (6, 3, 1)


# ---- c ----
@pytest.mark.parametrize("width", [4, 8])
def test_fill_runs(ctx, width):
    dev = _device_set(ctx, "fill", None, width)
    total = sum(c for _, c in E.fill_positions())
    for config in E.FILL_CONFIGS:
        ref = E.reference("fill", None, config)
        for chunk in CHUNKS:
            assert _check(ctx, dev, ref, config, chunk)["matches"] == total
    _forced_global(ctx, dev, E.reference("fill", None, E.FILL_CONFIGS[0]), E.FILL_CONFIGS[0])


# ---- d ----
def _need(info, samples, qs):
    from rabbittclust_amd import api
    return sum(len(samples[q]) for q in qs) * api.SCREEN_POS_BYTES + sum(info[q]["matches"] for q in qs) * api.SCREEN_MATCH_BYTES


@pytest.mark.parametrize("width", [4, 8])
def test_many_samples_and_empty_chunks(ctx, width):
    dev = _device_set(ctx, "many", None, width)
    sk, n_reps, live = dev
    reps, samples, _ = E.many()
    for config in E.MANY_CONFIGS:
        ref = E.reference("many", None, config)
        for chunk in E.MANY_CHUNKS:
            _check(ctx, dev, ref, config, chunk)
    _forced_global(ctx, dev, ref, config)
    # a budget of three times what the largest sample needs: the call is halved until its chunks fit
    config = E.MANY_CONFIGS[0]
    hits, sums, info = E.reference("many", None, config)
    every = range(len(samples))
    budget = 3 * max(_need(info, samples, [q]) for q in every)
    total = _need(info, samples, every)
    assert budget < total
    with ctx.env(RTC_SCREEN_BYTES=str(budget)):
        got_hits, got_sums = ctx.rep_screen(sk, n_reps, *config, live=live)
        assert ctx.rep_screen_counters()["chunks"] >= (total + budget - 1) // budget
    assert _tuples(got_hits) == R.flat(hits)
    assert len(got_sums) == len(samples) and _tuples(got_sums) == [s + (0,) for s in sums], "the sums are not complete"
    assert [int(s["n_hashes"]) for s in got_sums] == [len(x) for x in samples]
    for h in got_hits:  # every hit is of its own sample: the hashes it counts are that sample's
        assert len(set(reps[int(h["slot"])]) & set(samples[int(h["query"])])) == int(h["common"])


# ---- e ----
@pytest.mark.parametrize("name", sorted(E.THRESHOLDS))
def test_thresholds_at_equality(ctx, name):
    config = E.THRESHOLDS[name][1]
    dev = _device_set(ctx, "thresholds", name, 8)
    ref = E.reference("thresholds", name, config)
    _check(ctx, dev, ref, config)
    _forced_global(ctx, dev, ref, config)


# ---- f ----
@pytest.mark.parametrize("width", [4, 8])
def test_extreme_hashes(ctx, width):
    """SketchSet.from_host takes every value, 0 and the all-ones hash included: none is left out."""
    dev = _device_set(ctx, "extremes", width, width)
    ref = E.reference("extremes", width, E.EXTREME_CONFIG)
    for chunk in (0, 1):
        _check(ctx, dev, ref, E.EXTREME_CONFIG, chunk)
    _forced_global(ctx, dev, ref, E.EXTREME_CONFIG)
