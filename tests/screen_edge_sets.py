"""The inputs of tests/test_gpu_screen_edges.py and tests/test_cpu_screen_edges.py: sketch sets that take rtc_rep_screen's kernels
where the generated set of tests/screen_sets.py never goes -- a winner that retires more positions than a workgroup has lanes,
positions held by dozens of candidates, a sample at each side of each gather path's boundary, the fill pass at each side of
SCREEN_SHORT_RUN and of a wave's 64 records, hundreds of samples with empty chunks between full ones, every threshold decided
by the equal case, and the hashes at the ends of both widths.  Every builder is deterministic and computed once; so is the
reference's result per (set, config).  Every size comes from the library's constants, so that a changed constant moves the sets."""
import functools
import os
import re

import numpy as np

import refscreen as R
import screen_sets as S

Q20 = R.Q20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def constants():
    """(SCREEN_WAVE_CANDS, SCREEN_BLOCK_CANDS, SCREEN_SHORT_RUN): the first two as rabbittclust_amd.api mirrors them, the third
    from csrc/rtc_screen.h, which alone has it"""
    from rabbittclust_amd import api
    text = open(os.path.join(ROOT, "rabbittclust_amd", "csrc", "rtc_screen.h")).read()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint(?:32|64)_t (SCREEN_\w+) = (\d+);", text)}
    return api.SCREEN_WAVE_CANDS, api.SCREEN_BLOCK_CANDS, c["SCREEN_SHORT_RUN"]


def as_width(lists, width, monotone=False):
    """screen_sets.as_width; monotone: width 8 through h * (2^33 + 1), which keeps the order of the hashes (and so every
    position of a sample) and still differs in the high words"""
    if width == 8 and monotone:
        return [np.asarray([int(h) * ((1 << 33) + 1) for h in x], dtype=np.uint64) for x in lists]
    return S.as_width(lists, width)


# ---- a. wide winners -------------------------------------------------------------------------------------------------------------
FAMILY = 2000
WIDE_CONFIGS = S.CONFIGS  # (1, 0, 1, 0), (2, Q20 // 4, 2, 0), (1, 0, 1, 3)
NESTED = 40


def wide_builds():
    """name -> (the number of 3-hash fillers, the number of nested subsets)"""
    wave, block, _ = constants()
    return {"wave": (0, 0), "workgroup": (wave + 100, 0), "global": (block + 100, 0), "nested": (0, NESTED)}


@functools.lru_cache(maxsize=None)
def wide(name):
    """Three families of FAMILY hashes; a dozen representatives, each 35 % to 95 % of one family plus 100 to 400 hashes of its
    own; one sample of about 3 000 hashes: 85 % of family 2, half of family 0 and 300 of noise.  Fillers: representatives of 3
    hashes, 1 or 2 of them the sample's, one half in the slots before the dozen and the other behind.  Nested: the prefixes of
    one order of family 2, 2 000 down to 440 hashes, behind the dozen.  -> (reps, samples, live None)"""
    n_fill, n_nested = wide_builds()[name]
    rng = np.random.default_rng(11)
    fam = [[int(x) for x in 10_000 * (f + 1) + rng.choice(6000, size=FAMILY, replace=False)] for f in range(3)]
    dozen, own = [], 100_000
    for i, frac in enumerate(np.linspace(0.35, 0.95, 12)):
        part = rng.choice(fam[i % 3], size=int(round(frac * FAMILY)), replace=False)
        n_own = int(rng.integers(100, 401))
        dozen.append(sorted([int(x) for x in part] + list(range(own, own + n_own))))
        own += 1000
    noise = [int(x) for x in 200_000 + rng.choice(50_000, size=300, replace=False)]
    x = sorted([int(h) for h in rng.choice(fam[2], size=FAMILY * 85 // 100, replace=False)] +
               [int(h) for h in rng.choice(fam[0], size=FAMILY // 2, replace=False)] + noise)
    fill, own = [], 1_000_000
    for j in range(n_fill):
        k = 1 + j % 2
        fill.append(sorted([int(h) for h in rng.choice(x, size=k, replace=False)] + list(range(own, own + 3 - k))))
        own += 4
    order = [int(h) for h in rng.permutation(fam[2])]
    nested = [sorted(order[: FAMILY - 40 * i]) for i in range(n_nested)]
    return fill[: n_fill // 2] + dozen + nested + fill[n_fill // 2:], [x], None


# ---- b. exact path boundaries ----------------------------------------------------------------------------------------------------
def boundary_sizes():
    wave, block, _ = constants()
    return (1, 63, 64, 65, wave - 1, wave, wave + 1, block - 1, block, block + 1)


def boundary_picks():
    """max_picks of the extra calls: 1, ne and ne + 1 of the samples at W, W + 1 and B + 1"""
    wave, block, _ = constants()
    return sorted({1, wave, wave + 1, wave + 2, block + 1, block + 2})


def _own(i, j):
    return 16 + 8 * i + j


def _link(i):
    return 16 + 8 * i + 4


@functools.lru_cache(maxsize=None)
def boundaries():
    """SCREEN_BLOCK_CANDS + 1 representatives in a chain: representative i has three hashes of its own and shares a link hash
    with representative i + 1.  The sample of ne takes two own hashes of each of the representatives 0 .. ne - 1, the third of
    representative ne - 1, the link below it (between ne - 2 and ne - 1), and every third link (between 0 and 1, 3 and 4, ...) below
    the one between ne - 3 and ne - 2: that one is left out even where it is a third one, since with it slot ne - 2 has four
    hashes as slot ne - 1 does and, being lower, takes round 1 from it.  No link reaches representative ne, so exactly ne are candidates;
    slot ne - 1 alone has 4, the slots next to a link have 3 and tie, the rest have 2 and tie."""
    n = boundary_sizes()[-1]
    reps = [sorted([_own(i, 0), _own(i, 1), _own(i, 2)] + ([_link(i - 1)] if i else []) + ([_link(i)] if i + 1 < n else [])) for i in range(n)]
    samples = []
    for ne in boundary_sizes():
        x = set()
        for i in range(ne):
            x |= {_own(i, 0), _own(i, 1)}
        x.add(_own(ne - 1, 2))
        x |= {_link(i) for i in range(0, ne - 3, 3)}
        if ne > 1:
            x.add(_link(ne - 2))
        samples.append(sorted(x))
    return reps, samples, None


# ---- c. fill runs ----------------------------------------------------------------------------------------------------------------
FILL_REPS = 340     # every tenth retired: 306 live, so that a run of 300 live slots exists
FILL_CONFIGS = ((1, 0, 1, 0), (2, Q20 // 4, 2, 0))
_STEP = 1000        # matched hashes are multiples of _STEP, everything between them is free for padding


def fill_lengths():
    s = constants()[2]
    return (1, s, s + 1, 63, 64, 65, 128, 129, 300)


def _fill_hashes():
    """the matched hashes by value: ten short ones below, the runs of fill_lengths() in that order, the 64 consecutive ones, ten
    short ones above"""
    low = [_STEP * (1 + k) for k in range(10)]
    run = {L: _STEP * (20 + i) for i, L in enumerate(fill_lengths())}
    block = [_STEP * (40 + j) for j in range(64)]
    high = [_STEP * (200 + k) for k in range(10)]
    return low, run, block, high


class _Chunk:
    """the samples of one chunk as they are laid out: hashes ascending within a sample, padded to the position wanted"""

    def __init__(self):
        self.samples, self.p = [[]], 0

    def at(self, p, h):
        """the matched hash h at position p of the chunk, the unmatched hashes just below h before it"""
        x, n = self.samples[-1], p - self.p
        assert h % _STEP == 0 and 0 <= n < _STEP - 1 and (not x or h - n > x[-1])
        x.extend(range(h - n, h))
        x.append(h)
        self.p = p + 1

    def pad_to(self, p):
        """unmatched hashes just above the sample's last, up to position p"""
        x, n = self.samples[-1], p - self.p
        base = x[-1] if x else 0
        assert 0 <= n and base % _STEP + n < _STEP
        x.extend(range(base + 1, base + 1 + n))
        self.p = p

    def close(self):
        self.samples.append([])


@functools.lru_cache(maxsize=None)
def fill_runs():
    """FILL_REPS representatives, every tenth retired.  For each L of fill_lengths() one hash is held by exactly L live
    representatives and by three retired ones; 64 consecutive hashes are held by the same SCREEN_SHORT_RUN + 1 live
    representatives; twenty hashes are held by 1 .. SCREEN_SHORT_RUN.  Four samples, laid out for query_chunk = 0 (positions p of
    the chunk, a wave being 64 of them):
      sample 0  short runs, a long run at p = 63, a long run at p = 64, the longest at p = 70, short runs; ends at p = 90
      sample 1  short runs from p = 91, a long run at p = 100 (the wave 64 .. 127 holds long runs of two samples, short ones
                between them), p = 128 .. 191 all long, p = 192 .. 255 all unmatched
      sample 2  every length of fill_lengths() once more, spread over two waves
      sample 3  short runs and, at its last position, a long run; P is no multiple of 64
    -> (reps, samples, live)"""
    s = constants()[2]
    low, run, block, high = _fill_hashes()
    rng = np.random.default_rng(17)
    live = np.array([0 if i % 10 == 9 else 1 for i in range(FILL_REPS)], dtype=np.uint8)
    alive, retired = np.flatnonzero(live), np.flatnonzero(live == 0)
    reps = [[2_000_000 + 4 * i + k for k in range(3)] for i in range(FILL_REPS)]
    for L, h in run.items():
        for i in list(rng.choice(alive, size=L, replace=False)) + list(rng.choice(retired, size=3, replace=False)):
            reps[int(i)].append(h)
    same = [int(i) for i in rng.choice(alive, size=s + 1, replace=False)] + [int(retired[0])]
    for h in block:
        for i in same:
            reps[i].append(h)
    for k, h in enumerate(low + high):
        for i in rng.choice(alive, size=1 + k % s, replace=False):
            reps[int(i)].append(h)
    c = _Chunk()
    # sample 0
    for k in range(6):
        c.at(10 * k + 3, low[k])
    c.at(63, run[65])
    c.at(64, run[128])
    c.at(70, run[300])
    for k in range(5):
        c.at(75 + 3 * k, high[k])
    c.pad_to(91)
    c.close()
    # sample 1
    c.at(92, low[1])
    c.at(93, low[4])
    c.at(95, low[s - 1])  # a run of exactly SCREEN_SHORT_RUN
    c.at(100, run[64])
    for j, h in enumerate(block):
        c.at(128 + j, h)
    c.pad_to(256)
    c.close()
    # sample 2
    p = 256
    for k in range(10):
        c.at(p + 2 * k, low[k])
    p += 30
    for L in fill_lengths():
        c.at(p, run[L])
        p += 11
    for k in range(10):
        c.at(p + 3 * k, high[k])
    c.pad_to(p + 40)
    c.close()
    # sample 3
    p = c.p
    c.at(p + 5, low[7])
    c.at(p + 6, low[8])
    c.at(p + 30, run[129])
    assert (c.p) % 64 != 0
    return [sorted(r) for r in reps], [list(x) for x in c.samples], live


def fill_positions():
    """[(sample, run)] per position of the chunk of all samples: the live representatives that hold its hash, counted from the
    lists alone"""
    reps, samples, live = fill_runs()
    held = {}
    for i, r in enumerate(reps):
        if live[i]:
            for h in r:
                held[h] = held.get(h, 0) + 1
    return [(q, held.get(h, 0)) for q, x in enumerate(samples) for h in x]


# ---- d. many samples -------------------------------------------------------------------------------------------------------------
MANY = 600
MANY_CONFIGS = ((1, 0, 1, 0), (2, Q20 // 2, 1, 0))
MANY_CHUNKS = (0, 7, 64)
EMPTY_RUN = (301, 371)       # 70 consecutive empty samples
NOISE_CHUNK = (14, 21)       # chunk 2 of 7: hashes, none matched
SINGLE_CHUNK = (21, 28)      # chunk 3 of 7: one matched hash each, so no candidate under min_common 2


@functools.lru_cache(maxsize=None)
def many():
    """200 representatives of 10 to 30 hashes from a pool of 3 000; MANY samples of 0 to 12 hashes: most take 5 to 12 hashes of
    one representative (and are its candidates at containment one half where it is short enough), every fifth draws from the
    pool at large, every eleventh holds noise alone; samples 0 to 2, EMPTY_RUN and the last two are empty."""
    rng = np.random.default_rng(23)
    pool = np.arange(1000, 4000)
    reps = [sorted(int(h) for h in rng.choice(pool, size=int(rng.integers(10, 31)), replace=False)) for _ in range(200)]
    samples = []
    for q in range(MANY):
        noise = [int(h) for h in 100_000 + rng.choice(50_000, size=int(rng.integers(1, 13)), replace=False)]
        r = reps[int(rng.integers(0, len(reps)))]
        if q < 3 or EMPTY_RUN[0] <= q < EMPTY_RUN[1] or q >= MANY - 2:
            x = []
        elif NOISE_CHUNK[0] <= q < NOISE_CHUNK[1]:
            x = noise if q % 2 else []
        elif SINGLE_CHUNK[0] <= q < SINGLE_CHUNK[1]:
            x = [r[q % len(r)]] + noise[:11]
        elif q % 11 == 5:
            x = noise
        elif q % 5 == 2:
            x = [int(h) for h in rng.choice(pool, size=int(rng.integers(1, 13)), replace=False)]
        else:
            k = int(rng.integers(5, min(12, len(r)) + 1))
            x = [int(h) for h in rng.choice(r, size=k, replace=False)] + noise[: min(12 - k, len(noise), q % 3)]
        samples.append(sorted(set(x)))
    return reps, samples, None


# ---- e. thresholds at equality ---------------------------------------------------------------------------------------------------
def _r(shared, size, own):
    """a representative of `size` hashes: `shared` and hashes of its own from `own` up"""
    return sorted(list(shared) + list(range(own, own + size - len(shared))))


_PEEL = ([list(range(1, 7)), [5, 6, 7, 8, 9], [10, 11, 50], [12, 60, 61]], [list(range(1, 13))], None)  # A, B, C, D and X = {1..12}
# name -> ((reps, samples, live), config); tests/test_cpu_screen_edges.py has the expected hits, worked out by hand
THRESHOLDS = {
    # common 7 of 32, 8 of 32, 8 of 33 at a quarter
    "quarter": (([_r(range(1, 8), 32, 1000), _r(range(11, 19), 32, 2000), _r(range(21, 29), 33, 3000)],
                 [list(range(1, 8)) + list(range(11, 19)) + list(range(21, 29))], None), (1, Q20 // 4, 1, 0)),
    # round(0.3 * Q20) = 314 573: 3 of 10 misses it (3 * 2^20 = 3 145 728 < 3 145 730), 4 of 10 does not
    "three_tenths": (([_r([1, 2, 3], 10, 1000), _r([11, 12, 13, 14], 10, 2000)], [[1, 2, 3, 11, 12, 13, 14]], None),
                     (1, int(round(0.3 * Q20)), 1, 0)),
    "whole": (([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 1000]], [list(range(1, 11))], None), (1, Q20, 1, 0)),
    "min_common_at": (([[1, 2, 3, 1000], [4, 5, 6, 7, 1001]], [list(range(1, 8))], None), (3, 0, 1, 0)),
    "min_common_above": (([[1, 2, 3, 1000], [4, 5, 6, 7, 1001]], [list(range(1, 8))], None), (4, 0, 1, 0)),
    "min_unique_at_last": (_PEEL, (1, 0, 2, 0)),     # the picks' counts are 6, 3, 2 (and 1)
    "min_unique_at_second": (_PEEL, (1, 0, 3, 0)),
    "min_unique_above_second": (_PEEL, (1, 0, 4, 0)),
    "max_picks_all": (_PEEL, (1, 0, 1, 4)),
    "max_picks_less_one": (_PEEL, (1, 0, 1, 3)),
    "empty_slots": (([[], [1, 2, 3], [], [3, 4], []], [[1, 2, 3, 4, 5]], None), (1, 0, 1, 0)),
    "retired_winner": (([list(range(1, 9)), [1, 2, 3], [4, 5]], [list(range(1, 9))], (0, 1, 1)), (1, 0, 1, 0)),
}


# ---- f. extreme hashes -----------------------------------------------------------------------------------------------------------
EXTREME_CONFIG = (1, 0, 1, 0)
ENDS = {4: (0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff),
        8: (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)}
# (in a representative, in a sample): equal in one 32-bit half, different in the other -- never a match
HALF_PAIRS = ((0x00000001_DEADBEEF, 0x00000002_DEADBEEF), (0x80000000_00000005, 0x00000000_00000005),
              (0x00000000_FFFFFFFE, 0x7FFFFFFF_FFFFFFFE),   # the low words agree
              (0xFFFFFFFF_00000000, 0xFFFFFFFF_00000002), (0xCAFEF00D_00000007, 0xCAFEF00D_00000008),
              (0x80000000_00000001, 0x80000000_80000001))   # the high words agree


@functools.lru_cache(maxsize=None)
def extremes(width):
    """The six hashes of ENDS[width] over three representatives and three samples, each shared at least once; width 8 also has
    HALF_PAIRS, one member in a representative and the other in a sample.  The values go to the library as they are, through
    no bijection.  (SketchSet.from_host takes every value, 0 included.)"""
    a, b, c, d, e, f = ENDS[width]
    reps = [[a, c, f], [b, d, e], [a, b, d, f]]
    samples = [[a, d, f], [b, c, e], [a, b, c, d, e, f]]
    if width == 4:
        samples[0].append(5)
    else:
        for i, (in_rep, in_sample) in enumerate(HALF_PAIRS):
            reps[i % 3].append(in_rep)
            samples[(i + 1) % 3].append(in_sample)
            samples[(i + 2) % 3].append(in_sample)
    return [sorted(r) for r in reps], [sorted(set(x)) for x in samples], None


def extremes_arrays(lists, width):
    return [np.asarray(x, dtype=np.uint64 if width == 8 else np.uint32) for x in lists]


# ---- the reference, once per (set, config) ---------------------------------------------------------------------------------------
def the_set(group, name):
    if group == "wide":
        return wide(name)
    if group == "boundaries":
        return boundaries()
    if group == "fill":
        return fill_runs()
    if group == "many":
        return many()
    if group == "thresholds":
        return THRESHOLDS[name][0]
    if group == "extremes":
        return extremes(name)
    raise KeyError(group)


@functools.lru_cache(maxsize=None)
def reference(group, name, config):
    """refscreen.screen over one set for one config (min_common, min_cont_q20, min_unique, max_picks): (hits, sums, info)"""
    reps, samples, live = the_set(group, name)
    mc, cont, mu, picks = config
    return R.screen(reps, samples, mc, cont, mu, picks, live)
