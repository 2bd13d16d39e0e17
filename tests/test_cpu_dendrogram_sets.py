"""What tests/test_gpu_dendrogram_turns.py takes for granted about its inputs (tests/dendrogram_sets.py) and its references: the
closed form of top_chain, where top_group's first joins sit and that its sums are exact, refnj.nj cut short, and the two scan
switches' accessors."""
import numpy as np
import pytest

from tests import dendrogram_sets as DS
from tests import refnj as RN
from tests import refupgma as RU


@pytest.mark.parametrize("m", [2, 5, 70, 131])
def test_top_chain_is_its_closed_form(m):
    S = DS.top_chain(m)
    assert S.dtype == np.uint64 and np.array_equal(S, S.T) and not S.diagonal().any()
    want = DS.top_chain_records(m)
    assert len(want) == m - 1
    assert RU.rowcache(S.tolist())[0] == want
    if m <= 70:
        assert RU.naive(S.tolist()) == want
    # the winner is the last row of the active list at every step, and its mean is the one least: row k's is 8 (m - k)
    assert [(a, b) for a, b, *_ in want] == [(m - 2 - t, m - 1 - t) for t in range(m - 1)]
    assert all(s == 8 * (m - a) * na * nb for a, _, na, nb, s in want)


def test_top_chain_sizes_reach_the_turns_they_are_for():
    # the reduce of the merge kernel reads min((r + 2) / 4, 1024) minima; the winner's workgroup is (r - 2) / 4
    steps = [r for r in range(DS.CHAIN_M, 1, -1) if (r - 2) // 4 >= 256]
    assert len(steps) == 275 and ((steps[0] - 2) // 4, (steps[-1] - 2) // 4) == (324, 256)
    # a scan of 1 024 workgroups has 4 096 first rows; the winner's row r - 2 is past them for seven steps
    assert sum(1 for r in range(DS.CAP_UPGMA_M, 1, -1) if r - 2 >= 4096) == 7
    assert DS.CAP_NJ_M - DS.GROUP >= 4096 and (DS.REDUCE_M - DS.GROUP) // 4 >= 256


@pytest.mark.parametrize("m", [140, 600])
def test_top_group_joins_inside_the_group_first_and_is_exact(m):
    g = DS.GROUP
    D = DS.top_group(m)
    assert np.array_equal(D, D.T) and not D.diagonal().any() and DS.on_grid_64(D)
    first = RN.nj(D, steps=g - 1)
    assert len(first) == g - 1 and all(a >= m - g and b >= m - g for a, b, *_ in first)
    assert [(a - m, b - m) for a, b, *_ in first] == [(-6, -5), (-2, -1), (-4, -3), (-6, -4), (-6, -2)]
    # the sums are exact in any order: numpy's row sums give the same records, to the bit, as the ordered loop
    assert RN.bits(RN.nj(D, steps=g - 1, exact_sums=True)) == RN.bits(first)


def test_nj_cut_short_is_a_prefix_of_the_whole_run():
    m = 140
    D = DS.top_group(m)
    whole = RN.nj(D)
    assert len(whole) == m - 2
    for k in (0, 1, DS.GROUP - 1, m - 3, m - 2, m):
        assert RN.bits(RN.nj(D, steps=k)) == RN.bits(whole[:k]), k
    assert RN.bits(RN.nj(D, exact_sums=True)) == RN.bits(whole)


def test_library_exports_the_scan_switch_accessors():
    from rabbittclust_amd import _lib, api
    lib = _lib.load()
    for name in ("rtc_nj_scan_blocks", "rtc_upgma_scan_blocks"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name)(None) == 0  # no context: nothing to report, as the last_path calls
    assert callable(api.Context.nj_scan_blocks) and callable(api.Context.upgma_scan_blocks)
    assert api.NJ_SCAN_BLOCKS == api.UPGMA_SCAN_BLOCKS == 1024
