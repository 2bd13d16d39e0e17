"""CPU suite: the k2-type word of the MinHash kernels' table hash (csrc/rtc_minhash_core.h: build_kmer_lut, word_k2), restated
in numpy.  The plain table layout folds the word's cross product (AH + BL) * hi(2 c1), which is linear in its two table
indices mod 2^32, into the tables: the AH term inside P.hi, the BL term as a second dword beside BL.  What the three
instructions add, mad, add then give must be MurmurHash3's rotl64(w * c2, 33) * c1 for every word -- all 65 536 8-base words
at 5, 6, 7 and 8 bytes (the masked second half of a partial word), all 256 at 1..4 bytes (no second half).  And the LDS plan
that follows from the tables' size: where the plain layout ends, and that no sketch size lost its third workgroup per CU."""
import ctypes as C

import numpy as np
import pytest

C1 = 0x87C37B91114253D5
C2 = 0x4CF5AD432745937F
M64 = (1 << 64) - 1
K2_CROSS = ((C1 << 1) & M64) >> 32
C1X2_LO = (C1 << 1) & 0xFFFFFFFF
U64 = np.uint64


def _ascii4(e):
    """the four ASCII bytes of the 2-bit codes in e (first base in bits 7..6), first base lowest: codes_to_ascii"""
    lut = np.array([0x41, 0x43, 0x47, 0x54], dtype=np.uint64)
    e = np.asarray(e, dtype=np.uint64)
    return lut[(e >> U64(6)) & U64(3)] | lut[(e >> U64(4)) & U64(3)] << U64(8) | lut[(e >> U64(2)) & U64(3)] << U64(16) | lut[e & U64(3)] << U64(24)


def _lo32(x):
    return x & U64(0xFFFFFFFF)


def _tables(nb):
    """build_kmer_lut for a k2-type word of nb bytes, plain layout: per first-half index {P.lo, P.hi', AH}, per second-half
    index {BL, BLc}"""
    e = np.arange(256, dtype=np.uint64)
    a4 = _ascii4(e)
    am = U64(0xFFFFFFFF) if nb >= 4 else U64((1 << (8 * nb)) - 1)
    bm = U64(0xFFFFFFFF) if nb >= 8 else U64((1 << (8 * (nb - 4))) - 1 if nb > 4 else 0)
    with np.errstate(over="ignore"):
        A = (a4 & am) * U64(C2)                      # < 2^32 times a 64-bit constant, mod 2^64
        AL, AH = _lo32(A), A >> U64(32)
        P = ((_lo32(AL << U64(1)) << U64(32)) | (AL >> U64(31))) * U64(C1)
        Phi = _lo32((P >> U64(32)) + _lo32(AH * U64(K2_CROSS)))
        BL = _lo32((a4 & bm) * U64(C2 & 0xFFFFFFFF))
        BLc = _lo32(BL * U64(K2_CROSS))
    return _lo32(P), Phi, AH, BL, BLc, a4 & am, a4 & bm


def _word_k2(Plo, Phi, AH, BL, BLc):
    """v_add_u32, v_mad_u64_u32, v_add_u32"""
    with np.errstate(over="ignore"):
        SH = _lo32(AH + BL)
        R = SH * U64(C1X2_LO) + (Plo | (Phi << U64(32)))   # 32 x 32 -> 64 plus a 64-bit addend, mod 2^64
        return _lo32(R) | (_lo32((R >> U64(32)) + BLc) << U64(32))


def _reference(w):
    with np.errstate(over="ignore"):
        S = w * U64(C2)
        return ((S << U64(33)) | (S >> U64(31))) * U64(C1)


@pytest.mark.parametrize("nb", [5, 6, 7, 8])
def test_k2_word_from_tables_all_8_base_words(nb):
    Plo, Phi, AH, BL, BLc, a, b = _tables(nb)
    ia, ib = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    ia, ib = ia.ravel(), ib.ravel()
    got = _word_k2(Plo[ia], Phi[ia], AH[ia], BL[ib], BLc[ib])
    want = _reference(a[ia] | (b[ib] << U64(32)))
    assert got.shape == (65536,) and np.array_equal(got, want)
    if nb < 8:  # the mask matters: the unmasked second half gives another word
        assert not np.array_equal(want, _reference(a[ia] | (_ascii4(ib) << U64(32))))


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
def test_k2_word_without_a_second_half(nb):
    """at most four bytes: no BL, no BLc -- the whole cross product sits in P.hi"""
    Plo, Phi, AH, BL, BLc, a, b = _tables(nb)
    assert not BL.any() and not BLc.any() and not b.any()
    zero = np.zeros(256, dtype=np.uint64)
    assert np.array_equal(_word_k2(Plo, Phi, AH, zero, zero), _reference(a))


def test_cross_term_is_what_the_four_instruction_form_multiplies():
    """the packed layout keeps P.hi plain and multiplies (AH + BL) * hi(2 c1): same word"""
    Plo, Phi, AH, BL, BLc, a, b = _tables(8)
    rng = np.random.default_rng(5)
    ia, ib = rng.integers(0, 256, 4096), rng.integers(0, 256, 4096)
    with np.errstate(over="ignore"):
        Phi_plain = _lo32(Phi - _lo32(AH * U64(K2_CROSS)))
        SH = _lo32(AH[ia] + BL[ib])
        R = SH * U64(C1X2_LO) + (Plo[ia] | (Phi_plain[ia] << U64(32)))
        four = _lo32(R) | (_lo32((R >> U64(32)) + _lo32(SH * U64(K2_CROSS))) << U64(32))
    assert np.array_equal(four, _word_k2(Plo[ia], Phi[ia], AH[ia], BL[ib], BLc[ib]))


# ---- the LDS plan that follows from the tables' size ------------------------------------------------------------------
def _lut_bytes(k, pk):
    """lut_bytes of rtc_minhash_core.h"""
    words = (k + 7) // 8
    last_nb = k - 8 * (words - 1)
    direct = last_nb <= 5
    los = words - (1 if direct else 0)
    his = los if direct else (k + 3) // 8
    hi = 0 if pk else sum(2048 if w & 1 else 1024 for w in range(his))
    return los * 4096 + hi + ((8 << (2 * last_nb)) if direct else 0), his


def _max_s(k, pk, wgs):
    share = (156 * 1024 // wgs) & ~2047
    return (share - _lut_bytes(k, pk)[0] - 80 - 4096) // 8 - 512   # Ctrl, the wave queues, the minimum room


def _plan(lib, k, size):
    wgs, pk, lds = C.c_int(0), C.c_int(0), C.c_uint64(0)
    assert lib.rtc_sketch_minhash_plan(None, k, size, C.byref(wgs), C.byref(pk), C.byref(lds)) == 0
    return wgs.value, bool(pk.value), lds.value


def test_plain_layout_ends_at_3190_for_k21_and_no_size_lost_a_workgroup(monkeypatch):
    from rabbittclust_amd import _lib
    monkeypatch.delenv("RTC_SKETCH_PACKED", raising=False)
    monkeypatch.delenv("RTC_SKETCH_NO_PACKED", raising=False)
    lib = _lib.load()
    assert _lut_bytes(21, False)[0] == 19 * 1024 and _lut_bytes(21, True)[0] == 16 * 1024
    assert _max_s(21, False, 3) == 3190 and _max_s(21, True, 3) == 3574
    assert _plan(lib, 21, 1000)[:2] == (3, False) and _plan(lib, 21, 2000)[:2] == (3, False)   # the bench's shapes
    assert _plan(lib, 21, 3190)[:2] == (3, False) and _plan(lib, 21, 3191)[:2] == (3, True)
    assert _plan(lib, 21, 3574)[:2] == (3, True) and _plan(lib, 21, 3575)[:2] == (2, False)
    # every k: three workgroups per CU up to the packed layout's limit (its tables did not change), the plain layout
    # wherever it fits, and an allocation inside the workgroup's share
    for k in range(1, 33):
        his = _lut_bytes(k, False)[1]
        plain3, pk3 = _max_s(k, False, 3), _max_s(k, True, 3) if his else _max_s(k, False, 3)
        assert plain3 <= pk3
        for s in sorted({1, 64, 1000, plain3 - 1, plain3, plain3 + 1, pk3, pk3 + 1, 6144}):
            wgs, pk, lds = _plan(lib, k, s)
            assert wgs == (3 if s <= pk3 else 2 if s <= max(_max_s(k, False, 2), _max_s(k, True, 2)) else 1), (k, s)
            if s <= pk3:
                assert pk == (s > plain3), (k, s)
            assert lds <= ((156 * 1024 // wgs) & ~2047), (k, s)
