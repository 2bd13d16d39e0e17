"""GPU parity for the k2-type word's tabulated cross product (csrc/rtc_minhash_core.h: build_kmer_lut, word_k2): sketches of a
handful of small genomes, hash for hash against the CPU oracle -- for the k whose second, or second and fourth, 8-base word
takes a path of its own (a table pair with a whole or a partial second half, a table of its own, the express and the general
walk), both input formats, a small sketch on the plain tables and one just large enough that the plan picks the packed
tables (which keep the four-instruction word and a P.hi of their own), and both sides of the plain / packed boundary at
k = 21."""
import numpy as np
import pytest
import torch

from test_gpu_sketch_kssd_packed import pack_batch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = [13, 16, 17, 21, 24, 25, 28, 29, 31, 32]
LENS = [3000, 20_000, 7001, 12_345, 4097]


@pytest.fixture(scope="module")
def genomes():
    """five genomes of 3 000 - 20 000 bases; the second holds an N run: its loads take the general walk, the clean ones
    the express walk (17 <= k <= 28)"""
    rng = np.random.default_rng(2108)
    parts = [rng.choice(ACGT, size=L) for L in LENS]
    parts[1][9000:9040] = ord("N")
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(LENS)
    seq = np.concatenate(parts)
    packed, n_bases, runs = pack_batch(seq)
    return seq, off, packed, n_bases, runs


_want = {}


def _oracle(oracle, genomes, k, s):
    if (k, s) not in _want:
        _want[(k, s)] = oracle.sketch_minhash_batch(genomes[0], genomes[1], k, s)
    return _want[(k, s)]


def _sketch(ctx, genomes, staging, k, s):
    seq, off, packed, n_bases, runs = genomes
    if staging == "packed":
        sk = ctx.sketch_minhash_packed(torch.from_numpy(packed).to(ctx.device), off, k=k, size=s, n_bases=n_bases,
                                       runs=torch.from_numpy(runs).to(ctx.device))
    else:
        sk = ctx.sketch_minhash(ctx.upload_sequences(seq), off, k=k, size=s)
    ctx.sync()
    return sk.to_host()


def _first_packed_size(ctx, k):
    """the smallest sketch size for which the plan picks the packed tables (None: this k never does)"""
    return next((s for s in range(65, 6145) if ctx.sketch_minhash_plan(k, s)["packed_tables"]), None)


def _check(ctx, oracle, genomes, staging, k, s):
    got = _sketch(ctx, genomes, staging, k, s)
    want = _oracle(oracle, genomes, k, s)
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"genome {g}: k={k} s={s} {staging}: got {len(a)} hashes, want {len(b)}"


@pytest.mark.parametrize("staging", ["ascii", "packed"])
@pytest.mark.parametrize("k", KS)
def test_small_sketch_on_the_plain_tables(ctx, oracle, genomes, k, staging):
    plan = ctx.sketch_minhash_plan(k, 64)
    assert not plan["packed_tables"] and plan["wgs_per_cu"] == 3
    _check(ctx, oracle, genomes, staging, k, 64)


@pytest.mark.parametrize("staging", ["ascii", "packed"])
@pytest.mark.parametrize("k", KS)
def test_sketch_size_that_takes_the_packed_tables(ctx, oracle, genomes, k, staging):
    s = _first_packed_size(ctx, k)
    assert s is not None, f"k={k}: the plan never picks the packed tables"
    assert ctx.sketch_minhash_plan(k, s)["packed_tables"] and not ctx.sketch_minhash_plan(k, s - 1)["packed_tables"]
    assert ctx.sketch_minhash_plan(k, s)["wgs_per_cu"] == ctx.sketch_minhash_plan(k, s - 1)["wgs_per_cu"] == 3
    _check(ctx, oracle, genomes, staging, k, s)


@pytest.mark.parametrize("staging", ["ascii", "packed"])
def test_both_sides_of_the_plain_packed_boundary_at_k21(ctx, oracle, genomes, staging):
    """19 KiB of plain tables leave three workgroups per CU room for s <= 3 190 (3 318 while the second word's second-half
    table held 4-byte entries); the packed tables take over up to 3 574"""
    below, above = ctx.sketch_minhash_plan(21, 3190), ctx.sketch_minhash_plan(21, 3191)
    assert not below["packed_tables"] and above["packed_tables"] and below["wgs_per_cu"] == above["wgs_per_cu"] == 3
    _check(ctx, oracle, genomes, staging, 21, 3190)
    _check(ctx, oracle, genomes, staging, 21, 3191)
