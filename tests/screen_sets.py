"""The sketch sets of the rtc_rep_screen tests (tests/test_cpu_screen.py asserts on the reference alone that they reach the
ground the GPU tests stand on; tests/test_gpu_screen.py runs the library over them) and the reference's results, computed once."""
import functools

import numpy as np

import refscreen as S

Q20 = S.Q20
SEED = 3
HUB = 7
# (min_common, min_cont_q20, min_unique, max_picks)
CONFIGS = ((1, 0, 1, 0), (2, Q20 // 4, 2, 0), (1, 0, 1, 3))
# the samples of generated()
MIX6, MIX2, DRAWN, DISJOINT, EMPTY, SMALL = range(6)
# the representatives MIX6 takes whole: slot 0 has an exact duplicate at slot 4900, slot 10 lies between them
WHOLE_A, WHOLE_B, DUP_OF_A = 0, 10, 4900


def hand():
    """X = {1..10}, A = {1..6}, B = {5,6,7,8}, C = {1,2,3}, D = {9,20,21,22}"""
    return [list(range(1, 7)), [5, 6, 7, 8], [1, 2, 3], [9, 20, 21, 22]], [list(range(1, 11))]


@functools.lru_cache(maxsize=None)
def generated():
    """5 000 representatives of 20 to 59 hashes from a pool of 30 000, one hub hash in the first 4 900, 100 exact duplicates of
    earlier representatives, about a tenth of the slots retired.  -> (reps, samples, live) as lists of sorted int lists."""
    rng = np.random.default_rng(SEED)
    pool = np.unique(rng.integers(1000, 1000 + 30_000, size=30_000, dtype=np.int64))
    reps = []
    for r in range(5000):
        s = set(int(x) for x in rng.choice(pool, size=int(rng.integers(20, 60)), replace=False))
        if r < 4900:
            s.add(HUB)
        reps.append(sorted(s))
    for r in range(0, 300, 3):  # duplicates of earlier representatives
        reps[4900 + r // 3] = list(reps[r])
    live = (rng.random(len(reps)) > 0.1).astype(np.uint8)
    part = [600, 1200, 1800, 2400]  # taken in part by MIX6
    two = sorted(range(1000, 1100), key=lambda s: (-len(reps[s]), s))[:2]  # MIX2: the two longest of a hundred, whole
    small = [4970, 4980]            # SMALL: a dozen hashes of each
    for s in [WHOLE_A, WHOLE_B, DUP_OF_A] + part + two + small:
        live[s] = 1
    assert live[:4900].min() == 0, "no retired slot among the hub's"
    noise = [int(x) for x in rng.integers(100_000, 200_000, size=200)]
    mix6 = set(reps[WHOLE_A]) | set(reps[WHOLE_B]) | {HUB} | set(noise)
    for i, s in enumerate(part):
        mix6 |= set(reps[s][: len(reps[s]) * (i + 2) // 6])
    mix2 = (set(reps[two[0]]) | set(reps[two[1]])) - {HUB}
    drawn = set(int(x) for x in rng.choice(pool, size=3000, replace=False))
    disjoint = set(int(x) for x in rng.integers(300_000, 400_000, size=50))
    sm = (set(reps[small[0]][:12]) | set(reps[small[1]][:11])) - {HUB}
    samples = [sorted(mix6), sorted(mix2), sorted(drawn), sorted(disjoint), [], sorted(sm)]
    return reps, samples, live


def as_width(lists, width):
    """the lists as ascending arrays of the width's type.  Width 8 sends every hash through a bijection of the 64-bit integers
    (an odd multiplier), so that the high words differ and the order of the hashes is another one; which sets share which hashes
    stays as it is, and with it every result."""
    if width == 4:
        return [np.asarray(x, dtype=np.uint32) for x in lists]
    mul = np.uint64(0x9E3779B97F4A7C15)
    return [np.sort(np.asarray(x, dtype=np.uint64) * mul) for x in lists]


@functools.lru_cache(maxsize=None)
def reference(config):
    """refscreen.screen over generated() for one of CONFIGS, computed once and shared"""
    reps, samples, live = generated()
    mc, cont, mu, picks = config
    return S.screen(reps, samples, mc, cont, mu, picks, live)
