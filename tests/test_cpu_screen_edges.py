"""The sets of tests/screen_edge_sets.py without a GPU: on the restatement (tests/refscreen.py) alone, every set is shown to have
the property its test in tests/test_gpu_screen_edges.py stands on.  A set that stops meeting its condition -- after a changed
constant, say -- fails here and does not pass silently there.  The threshold cases are held to hit lists written out by hand."""
import pytest

import refscreen as R
import screen_edge_sets as E

Q20 = R.Q20


def test_constants_are_read():
    wave, block, short = E.constants()
    assert 64 < wave and wave + 1 < block - 1 and 5 < short < 10 and short + 1 < 63
    assert len(set(E.boundary_sizes())) == 10 and len(set(E.fill_lengths())) == 9


def test_refscreen_new_keys_on_the_hand_case():
    import screen_sets as S
    reps, x = S.hand()
    _, _, info = R.screen(reps, x, 1, 0, 1, 0)  # picks A (6 common), B (4), D (1): D is the highest slot, the hashes 5 and 6 are in A and B
    assert info[0]["widest_pick"] == 6 and info[0]["holders_max"] == 2 and info[0]["last_index_picks"] == [3]
    _, _, info = R.screen(reps, x, 1, 0, 1, 0, live=[0, 0, 0, 0])
    assert info[0]["widest_pick"] == 0 and info[0]["holders_max"] == 0 and info[0]["last_index_picks"] == []


# ---- a ----
@pytest.mark.parametrize("name", ["wave", "workgroup", "global", "nested"])
def test_wide_winners(name):
    wave, block, _ = E.constants()
    reps, samples, _ = E.wide(name)
    n_fill, n_nested = E.wide_builds()[name]
    assert len(reps) == 12 + n_fill + n_nested and len(samples) == 1 and 2800 <= len(samples[0]) <= 3200
    hits, sums, info = E.reference("wide", name, E.WIDE_CONFIGS[0])
    picks = [r for r in hits[0] if r[4]]
    print(name, "n_hits", sums[0][3], "picks", len(picks), "common of the first picks", [r[1] for r in picks[:4]], "unique", [r[3] for r in picks[:4]],
          "holders_max", info[0]["holders_max"])
    assert picks[0][1] > 4 * 256, "the first pick retires no more positions than four turns of 256 lanes"
    assert any(r[3] < r[1] / 4 and r[1] > 256 for r in picks[1:]), "no later pick whose count was mostly taken away by earlier rounds"
    n_hits = sums[0][3]
    if name in ("wave", "nested"):
        assert 0 < n_hits <= wave
    elif name == "workgroup":
        assert wave < n_hits <= block
    else:
        assert n_hits > block
    if name == "nested":
        assert info[0]["holders_max"] >= 32 and info[0]["widest_pick"] > 1024
    # the other configurations keep a wide first pick, and the third stops the rounds early
    _, sums2, info2 = E.reference("wide", name, E.WIDE_CONFIGS[1])
    assert info2[0]["widest_pick"] > 4 * 256 and 0 < sums2[0][3] <= n_hits
    _, sums3, _ = E.reference("wide", name, E.WIDE_CONFIGS[2])
    assert sums3[0][4] == 3 < sums[0][4]


# ---- b ----
def test_boundaries():
    wave, block, _ = E.constants()
    sizes = E.boundary_sizes()
    assert sizes == (1, 63, 64, 65, wave - 1, wave, wave + 1, block - 1, block, block + 1)
    reps, samples, _ = E.boundaries()
    assert len(reps) == block + 1 and all(len(r) in (4, 5) for r in reps)
    hits, sums, info = E.reference("boundaries", None, (1, 0, 1, 0))
    for q, ne in enumerate(sizes):
        assert sums[q][3] == ne and sorted(r[0] for r in hits[q]) == list(range(ne)), ne
        assert info[q]["rounds"] == ne == sums[q][4]
        order = [r[0] for r in hits[q]]
        if ne > 1:
            assert info[q]["last_index_picks"] == [1] and order[0] == ne - 1, "round 1 is not the highest eligible slot's"
            assert order != sorted(order)
        assert len(info[q]["ties"]) >= ne - 2
    assert sum(1 for ne in sizes if ne <= wave) == 6 and sum(1 for ne in sizes if wave < ne <= block) == 3 and sum(1 for ne in sizes if ne > block) == 1
    assert max(i["rounds"] for i in info) == block + 1
    # max_picks at, below and above the number of candidates of the samples at W, W + 1 and B + 1
    assert set(E.boundary_picks()) == {1} | {ne + d for ne in (wave, wave + 1, block + 1) for d in (0, 1)}
    for mp in E.boundary_picks():
        _, s, _ = E.reference("boundaries", None, (1, 0, 1, mp))
        assert [x[4] for x in s] == [min(mp, ne) for ne in sizes]


# ---- c ----
def test_fill_runs():
    _, _, short = E.constants()
    reps, samples, live = E.fill_runs()
    assert len(reps) == E.FILL_REPS and 0.08 < 1.0 - live.mean() < 0.12 and all(x == sorted(set(x)) for x in samples) and len(samples) == 4
    pos = E.fill_positions()
    P = len(pos)
    run = [c for _, c in pos]
    sample = [q for q, _ in pos]
    assert set(E.fill_lengths()) <= set(run), "a run length of the list is not met"
    # retired representatives hold the long runs' hashes too: the run counts live slots only
    everyone = {}
    for r in reps:
        for h in r:
            everyone[h] = everyone.get(h, 0) + 1
    flat = [h for x in samples for h in x]
    assert all(everyone[flat[p]] > run[p] for p in range(P) if run[p] > short)
    long_ = [c > short for c in run]
    short_ = [0 < c <= short for c in run]
    assert run[0] == 0, "position 0 is matched"
    assert any(p % 64 == 63 and long_[p] and long_[p + 1] for p in range(P - 1)), "no long run in lane 63 with one in lane 0 behind it"
    waves = [range(w, min(w + 64, P)) for w in range(0, P, 64)]

    def two_samples(w):
        lp = [p for p in w if long_[p]]
        return any(sample[a] != sample[b] and any(short_[p] and sample[p] == sample[a] for p in range(a, b)) and
                   any(short_[p] and sample[p] == sample[b] for p in range(a, b)) for a in lp for b in lp if a < b)
    assert any(two_samples(w) for w in waves), "no wave with long runs of two samples and short runs between them"
    assert any(len(w) == 64 and all(long_[p] for p in w) for w in waves), "no wave of 64 long runs"
    assert any(len(w) == 64 and all(run[p] == 0 for p in w) for w in waves), "no wave without a matched hash"
    assert P % 64 != 0 and long_[P - 1], "no long run at the last position of a partial wave"
    assert any(c == short for c in run) and any(c == short + 1 for c in run)
    for config in E.FILL_CONFIGS:
        hits, sums, info = E.reference("fill", None, config)
        for q in range(len(samples)):
            assert info[q]["expansion"] == max(c for s, c in pos if s == q)
            assert sums[q][0] == len(samples[q])
        assert sum(i["matches"] for i in info) == sum(run)
        print(config, "hits", [s[3] for s in sums], "picks", [s[4] for s in sums])
        assert all(s[3] >= 2 for s in sums) and sum(1 for s in sums if s[4] >= 2) >= 2, "the rounds have nothing to do"
    assert [i["expansion"] for i in E.reference("fill", None, E.FILL_CONFIGS[0])[2]] == [300, 64, 300, 129]


# ---- d ----
def _chunk_kinds(samples, sums, info, chunk):
    kinds = []
    for q0 in range(0, len(samples), chunk):
        qs = range(q0, min(q0 + chunk, len(samples)))
        P, M, E_ = sum(len(samples[q]) for q in qs), sum(info[q]["matches"] for q in qs), sum(sums[q][3] for q in qs)
        kinds.append("P0" if P == 0 else "M0" if M == 0 else "E0" if E_ == 0 else "hits")
    return kinds


def test_many_samples():
    reps, samples, _ = E.many()
    assert len(samples) == E.MANY and len(reps) == 200 and all(10 <= len(r) <= 30 for r in reps) and all(len(x) <= 12 for x in samples)
    empty = [not x for x in samples]
    assert empty[0] and empty[1] and empty[2] and not empty[3] and empty[-1] and empty[-2] and not empty[-3]
    assert all(empty[E.EMPTY_RUN[0]:E.EMPTY_RUN[1]]) and E.EMPTY_RUN[1] - E.EMPTY_RUN[0] == 70
    hits1, sums1, info1 = E.reference("many", None, E.MANY_CONFIGS[0])
    hits2, sums2, info2 = E.reference("many", None, E.MANY_CONFIGS[1])
    assert E.MANY_CONFIGS[1] == (2, Q20 // 2, 1, 0)
    unmatched = sum(1 for q, x in enumerate(samples) if x and info1[q]["matches"] == 0)
    unfit = sum(1 for q in range(E.MANY) if info2[q]["matches"] and sums2[q][3] == 0)
    with_hits = sum(1 for s in sums2 if s[3])
    print("unmatched", unmatched, "matched without a candidate", unfit, "with hits", with_hits, "of", E.MANY)
    assert unmatched >= 5 and unfit >= 5 and with_hits >= 100
    assert any(s[4] >= 2 for s in sums1), "no sample of two picks"
    assert 7 in E.MANY_CHUNKS and 0 in E.MANY_CHUNKS
    kinds = _chunk_kinds(samples, sums2, info2, 7)
    for kind in ("P0", "M0", "E0"):
        assert kind in kinds, kind
        assert "hits" in kinds[kinds.index(kind) + 1:], "no chunk with hits behind the first chunk of kind " + kind
    assert kinds[0] == "hits" and kinds[-1] == "hits"
    kinds1 = _chunk_kinds(samples, sums1, info1, 7)
    assert "P0" in kinds1 and "M0" in kinds1


# ---- e ----
# (slot, common, size, unique, rank) and (n_hashes, n_matched, n_explained, n_hits, n_picks), by hand
A, B, C, D = 0, 1, 2, 3
EXPECT = {
    "quarter": ([(1, 8, 32, 8, 1)], (23, 8, 8, 1, 1)),              # 7 / 32 and 8 / 33 are below a quarter, 8 / 32 is a quarter
    "three_tenths": ([(1, 4, 10, 4, 1)], (7, 4, 4, 1, 1)),          # 3 / 10 is below round(0.3 * 2^20) / 2^20
    "whole": ([(0, 5, 5, 5, 1)], (10, 5, 5, 1, 1)),                 # 5 / 6 is not one
    "min_common_at": ([(1, 4, 5, 4, 1), (0, 3, 4, 3, 2)], (7, 7, 7, 2, 2)),
    "min_common_above": ([(1, 4, 5, 4, 1)], (7, 4, 4, 1, 1)),
    # X = {1..12}, A = {1..6}, B = {5..9}, C = {10, 11, 50}, D = {12, 60, 61}: the rounds take 6, 3, 2, 1
    "min_unique_at_last": ([(A, 6, 6, 6, 1), (B, 5, 5, 3, 2), (C, 2, 3, 2, 3), (D, 1, 3, 1, 0)], (12, 12, 11, 4, 3)),
    "min_unique_at_second": ([(A, 6, 6, 6, 1), (B, 5, 5, 3, 2), (C, 2, 3, 2, 0), (D, 1, 3, 1, 0)], (12, 12, 9, 4, 2)),
    "min_unique_above_second": ([(A, 6, 6, 6, 1), (B, 5, 5, 3, 0), (C, 2, 3, 2, 0), (D, 1, 3, 1, 0)], (12, 12, 6, 4, 1)),
    "max_picks_all": ([(A, 6, 6, 6, 1), (B, 5, 5, 3, 2), (C, 2, 3, 2, 3), (D, 1, 3, 1, 4)], (12, 12, 12, 4, 4)),
    "max_picks_less_one": ([(A, 6, 6, 6, 1), (B, 5, 5, 3, 2), (C, 2, 3, 2, 3), (D, 1, 3, 1, 0)], (12, 12, 11, 4, 3)),
    "empty_slots": ([(1, 3, 3, 3, 1), (3, 2, 2, 1, 2)], (5, 4, 4, 2, 2)),      # slots 0, 2 and 4 are empty
    "retired_winner": ([(1, 3, 3, 3, 1), (2, 2, 2, 2, 2)], (8, 5, 5, 2, 2)),   # slot 0 holds all eight and is retired
}


@pytest.mark.parametrize("name", sorted(E.THRESHOLDS))
def test_thresholds_by_hand(name):
    (reps, samples, live), config = E.THRESHOLDS[name]
    hits, sums, _ = E.reference("thresholds", name, config)
    assert len(samples) == 1 and (hits, sums) == ([EXPECT[name][0]], [EXPECT[name][1]])


def test_thresholds_are_at_equality():
    assert set(EXPECT) == set(E.THRESHOLDS)
    (reps, _, _), (_, cont, _, _) = E.THRESHOLDS["quarter"]
    assert [len(r) for r in reps] == [32, 32, 33] and (8 << 20) == cont * 32 and (7 << 20) < cont * 32 and (8 << 20) < cont * 33
    cont = E.THRESHOLDS["three_tenths"][1][1]
    assert cont == 314_573 and (3 << 20) == 3_145_728 < cont * 10 == 3_145_730 <= (4 << 20)
    assert E.THRESHOLDS["whole"][1][1] == Q20
    (reps, _, live), _ = E.THRESHOLDS["retired_winner"]
    assert len(reps[0]) > max(len(r) for r in reps[1:]) and not live[0]
    reps = E.THRESHOLDS["empty_slots"][0][0]
    assert [len(r) for r in reps] == [0, 3, 0, 2, 0]
    assert E.THRESHOLDS["max_picks_all"][1][3] == len(E.THRESHOLDS["max_picks_all"][0][0])


# ---- f ----
@pytest.mark.parametrize("width", [4, 8])
def test_extreme_hashes(width):
    reps, samples, _ = E.extremes(width)
    in_reps, in_samples = set().union(*reps), set().union(*samples)
    top = 2 ** (8 * width) - 1
    assert all(0 <= h <= top for h in in_reps | in_samples) and {0, top} <= in_reps & in_samples
    assert set(E.ENDS[width]) <= in_reps & in_samples, "an end value is not shared"
    arrays = E.extremes_arrays(reps + samples, width)
    assert [[int(h) for h in a] for a in arrays] == reps + samples, "a value does not survive the array's type"
    hits, sums, _ = E.reference("extremes", width, E.EXTREME_CONFIG)
    assert all(s[3] == 3 for s in sums)
    if width == 8:
        lo = lambda h: h & 0xffffffff
        hi = lambda h: h >> 32
        for a, b in E.HALF_PAIRS:
            assert a in in_reps and a not in in_samples and b in in_samples and b not in in_reps
            assert (lo(a) == lo(b)) != (hi(a) == hi(b))
        assert sum(1 for a, b in E.HALF_PAIRS if lo(a) == lo(b)) >= 2 and sum(1 for a, b in E.HALF_PAIRS if hi(a) == hi(b)) >= 2
        # a compare on one half alone gives other results: the set tells them apart
        for half in (lo, hi):
            wrong = R.screen([sorted(set(half(h) for h in r)) for r in reps], [sorted(set(half(h) for h in x)) for x in samples], *E.EXTREME_CONFIG)
            assert [[r[1] for r in sorted(hs)] for hs in wrong[0]] != [[r[1] for r in sorted(hs)] for hs in hits]
