"""GPU parity of the packed-input MinHash kernel where its walk changes hands: a wave's load (C = 4 096 bases) is the unit
that takes the express walk or the general one, a tile (T = 131 072 bases: four loads per lane) the unit of the workgroup's
protocol, and a segment's first tile starts outside safe mode when its starting threshold lets few k-mers through.  Every
sketch is compared bit for bit with the CPU oracle and with the ASCII kernel on the characters the batch was packed from."""
import os

import numpy as np
import pytest

from test_gpu_sketch_minhash import _random_genomes
from test_gpu_sketch_minhash_packed import ACGT, _check, _reload_options, _sketch_packed

pytestmark = pytest.mark.gpu

C = 4096       # bases of one wave load
T = 131072     # bases of one tile


@pytest.mark.parametrize("k", [17, 21, 28, 16, 29])  # 17..28 take the express walk; 16 and 29 are its neighbours
def test_lengths_around_load_and_tile(ctx, oracle, k):
    """genomes one base short of, exactly and one base over a load and a tile, and with k - 1 and k bases behind a load,
    in one batch: each starts wherever the one before it ended, at any offset inside a load"""
    rng = np.random.default_rng(500 + k)
    seq, off = _random_genomes(rng, [C - 1, C, C + 1, C + 20, C + 21, T - 1, T, T + 1, 2 * T + C + 21, 3 * C + 5])
    for s in (1, 64, 1000):
        _check(ctx, oracle, seq, off, k, size=s)


@pytest.mark.parametrize("s", [64, 1000])  # 64: the first tile starts outside safe mode, its loads walk express
def test_single_runs_break_a_stretch_of_loads(ctx, oracle, s):
    """one character outside ACGT at, in front of and behind a load's and a tile's first position, and an 8-base run across
    a load boundary: that load takes the general walk between two that walk express"""
    k = 21
    base = np.random.default_rng(77).choice(ACGT, size=3 * T + 1000)
    off = np.array([0, len(base)], dtype=np.uint64)
    for p in (C - 1, C, C + k - 1, 2 * C - 1, T - 1, T, T + k - 2):
        g = base.copy()
        g[p] = ord("N")
        _check(ctx, oracle, g, off, k, size=s)
    g = base.copy()
    g[2 * C - 4:2 * C + 4] = ord("N")
    _check(ctx, oracle, g, off, k, size=s)


def test_queue_loss_in_the_middle_of_a_tile(ctx, oracle):
    """a period-7 repeat in the middle of a genome: equal small hashes fill a wave's queue, the load is handed to the
    general walk and the buffer overflows outside safe mode; twice, with identical output"""
    rng = np.random.default_rng(78)
    g = rng.choice(ACGT, size=400_000)
    g[150_000:250_000] = np.tile(rng.choice(ACGT, size=7), 100_000 // 7 + 1)[:100_000]
    off = np.array([0, len(g)], dtype=np.uint64)
    _check(ctx, oracle, g, off, 21, size=1000)
    a = _sketch_packed(ctx, g, off, 21, size=1000).to_host()
    b = _sketch_packed(ctx, g, off, 21, size=1000).to_host()
    assert np.array_equal(a[0], b[0])


def _with_t0_factor(f, fn):
    os.environ["RTC_SKETCH_T0_FACTOR"] = f
    _reload_options()
    try:
        fn()
    finally:
        del os.environ["RTC_SKETCH_T0_FACTOR"]
        _reload_options()


@pytest.mark.parametrize("s", [1000, 3574])  # 3574: the smallest room the candidate buffer is planned with
def test_first_tile_under_a_forced_starting_threshold(ctx, oracle, s):
    """RTC_SKETCH_T0_FACTOR = 1000 and 0 (no starting threshold: safe mode from the first tile)"""
    rng = np.random.default_rng(79 + s)
    seq, off = _random_genomes(rng, [200_000, 200_000])
    for f in ("1000", "0"):
        _with_t0_factor(f, lambda: _check(ctx, oracle, seq, off, 21, size=s))


def test_optimistic_first_tile_overflows_and_is_walked_again(ctx, oracle):
    """A starting threshold under which a tile of random bases expects a few hundred candidates (the first tile starts
    outside safe mode), and a first tile that is a period-16 repeat one of whose k-mers hashes below that threshold:
    thousands of equal candidates -- the queue fills, the buffer overflows, the tile is walked again in safe mode."""
    k, s, L = 21, 1000, 600_000
    t0 = 3 * s / L  # start_threshold's rule for this genome, as a fraction of 2^64
    assert T * t0 < 708  # a quarter of the room at s = 1000, k = 21
    rng = np.random.default_rng(80)
    for _ in range(200):
        unit = rng.choice(ACGT, size=16)
        rep = np.tile(unit, 4)
        lowest = oracle.sketch_minhash_batch(rep, np.array([0, len(rep)], dtype=np.uint64), k, 1)[0]
        if len(lowest) and int(lowest[0]) < int(t0 * 2.0 ** 64):
            break
    else:
        pytest.fail("no repeat unit with a k-mer under the threshold")
    g = rng.choice(ACGT, size=L)
    g[:100_000] = np.tile(unit, 100_000 // 16)  # 6 250 copies: more than the buffer holds
    _check(ctx, oracle, g, np.array([0, L], dtype=np.uint64), k, size=s)


def test_partial_segments_alone_and_among_short_genomes(ctx, oracle):
    """a 6 Mbp genome cut into segments whose partial sketches are merged: alone, and behind 20 genomes of 50 kbp"""
    big = oracle.synth_genome(4321, 98, 300, 6_000_000)
    _check(ctx, oracle, big, np.array([0, len(big)], dtype=np.uint64), 21, size=1000)
    rng = np.random.default_rng(81)
    small, off = _random_genomes(rng, [50_000] * 10)
    small2, _ = _random_genomes(rng, [50_000] * 10)
    seq = np.concatenate([small, big, small2])
    lens = [50_000] * 10 + [len(big)] + [50_000] * 10
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    _check(ctx, oracle, seq, off, 21, size=1000)
