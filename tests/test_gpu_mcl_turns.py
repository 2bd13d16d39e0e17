"""rtc_mcl past a workgroup's first column, against tests/refmcl.py entry for entry: the turn sets of tests/mcl_sets.py give
every launch more columns than it has workgroups (the re-cleared table, the counters' reset and the closing barrier of
mcl_column_kernel, the reused reduction words), send one workgroup of the global path through tables of 1024, 8192 and 32768
slots in a row, wrap the probe chains of all three tables off the last slot, give mcl_start_kernel a column of more than its
256 lanes, and the high inflations take mcl_inflate's product loop through two to seven turns.  tests/test_cpu_mcl.py proves
on the restatement that the sets hold these cases on 256 CUs; every test here asks the device it runs on for its CUs and
fails if its grids are no longer passed."""
import pytest

from tests import mcl_sets as S
from tests.test_gpu_mcl import _check, global_path  # noqa: F401  (global_path is a fixture)

pytestmark = pytest.mark.gpu

_COUNTS = {}


def _sets():
    return S.turn_sets()


def _per_iteration(name, h, T):
    """the restatement's (wave, workgroup, global) columns of every iteration that a call at max_iter = T runs"""
    mats, _ = S.trajectory(name, h, _sets(), upto=T)
    for t in range(min(T, len(mats) - 1)):
        if (name, h, t) not in _COUNTS:
            _COUNTS[(name, h, t)] = S.path_counts(mats[t])
    return [_COUNTS[(name, h, t)] for t in range(min(T, len(mats) - 1))]


def _paths(c):
    return c["wave_columns"], c["workgroup_columns"], c["global_columns"]


def _run(ctx, name, h, T, rec=None, all_global=False):
    """_check, and the call's path and cut counters against the restatement's; -> (the counters, the columns per iteration)"""
    c = _check(ctx, name, h, T, rec=rec, sets=_sets())
    per = _per_iteration(name, h, T)
    assert len(per) == c["iterations"]
    if not all_global:
        assert _paths(c) == tuple(sum(p[i] for p in per) for i in range(3)), (name, h, T)
    assert c["cut_columns"] == S.cuts(name, h, T, _sets()), (name, h, T)
    return c, per


@pytest.fixture
def grids(ctx):
    start, wave, block, glob = S.grids(ctx.num_cu(), S.TURNS_N)
    assert S.TURNS_N > start  # mcl_start_kernel's workgroups take a second vertex
    return {"start": start, "wave": wave, "block": block, "global": glob}


def test_turns_10k_at_inflation_2(ctx, grids):
    """iterations 1, 2 and 3 and the fixed point: in each of the first three, more wave columns than the wave launch has
    workgroups and more workgroup columns than the workgroup launch has; from the second, global columns at two table sizes"""
    seen = [(0, 0, 0)]
    for T in (1, 2, 3):
        c, per = _run(ctx, "turns_10k", 4, T)
        assert c["iterations"] == T and c["converged"] == 0
        seen.append(_paths(c))
    for t in range(3):  # iteration t + 1 by the calls' own counters
        wave, block, glob = (seen[t + 1][i] - seen[t][i] for i in range(3))
        assert (wave, block, glob) == per[t]
        assert wave > grids["wave"] and block > grids["block"], (t, wave, block, grids)
        assert (glob > 0) == (t > 0)
    c, per = _run(ctx, "turns_10k", 4, 100)
    assert c["converged"] == 1 and c["iterations"] > 3 and c["cut_columns"] == 0
    assert all(p[0] > grids["wave"] for p in per)
    from rabbittclust_amd import api
    assert ctx.mcl_last_path() == api.MCL_PATH_WAVE | api.MCL_PATH_WORKGROUP | api.MCL_PATH_GLOBAL


@pytest.mark.parametrize("h", [3, 5])
def test_turns_10k_at_the_half_steps(ctx, grids, h):
    c, per = _run(ctx, "turns_10k", h, 2)
    assert c["iterations"] == 2
    assert all(p[0] > grids["wave"] and p[1] > grids["block"] for p in per) and per[1][2] > 0


def test_turns_10k_through_the_global_tables(ctx, grids, global_path):
    """RTC_MCL_GLOBAL=1: all 10240 columns of every iteration on the global launch, ten a workgroup on 256 CUs, which so goes
    through tables of 1024, 8192 and 32768 slots in the order its list has them"""
    from rabbittclust_amd import api
    n, _, sel = _sets()["turns_10k"]
    for T in (1, 3, 100):
        c, per = _run(ctx, "turns_10k", 4, T, all_global=True)
        assert _paths(c) == (0, 0, n * c["iterations"]) and n > grids["global"]
        assert ctx.mcl_last_path() == api.MCL_PATH_GLOBAL
    assert c["converged"] == 1
    # the tables of the second and the third iteration by the kernel's rule: the columns are the restatement's, as checked
    mats, _ = S.trajectory("turns_10k", 4, _sets())
    for M in mats[1:3]:
        assert {S.table_log2(w, n, sel) for w in S.work(M)} == {10, 13, 15}


def test_turns_10k_cut_at_8(ctx, grids):
    """S = 8: every column on the wave path in every iteration, thousands of them cut; the cut columns are counted exactly"""
    n = S.TURNS_N
    seen = [0]
    for T in (1, 3, 100):
        c, per = _run(ctx, "turns_10k_s8", 4, T)
        assert _paths(c) == (n * c["iterations"], 0, 0) and n > grids["wave"]
        seen.append(c["cut_columns"])
    assert c["converged"] == 1
    assert seen[1] > 1000 and seen[2] - seen[1] > 1000 and seen[3] >= seen[2]


@pytest.mark.parametrize("name", ["hub_300_s64", "hub_300_s1024"])
def test_hub_300_start_column_past_256_lanes(ctx, grids, name):
    """the hub's column of 301 keys: cut to 64 among equals, or written whole in two turns of the lanes"""
    n, rec, sel = _sets()[name]
    for T in (0, 1):
        c, per = _run(ctx, name, 4, T)
        assert c["iterations"] == T and c["converged"] == 0
        hub = sum(1 for col, _, _ in S.expected(name, 4, 0, _sets())[3] if col == S.HUB_300)
        assert hub == min(sel, 301) and (c["cut_columns"] > 0) == (sel < 301)
    assert S.cuts(name, 4, 0, _sets()) == (1 if sel < 301 else 0)


@pytest.mark.parametrize("h", [6, 7, 8, 11, 16])
@pytest.mark.parametrize("name", S.HIGH_INFLATION_SETS)
def test_high_inflation(ctx, name, h):
    for T in (1, 2, 100):
        c = _check(ctx, name, h, T)
        assert c["cut_columns"] == S.cuts(name, h, T)
    assert c["converged"] == 1


@pytest.mark.parametrize("h", [7, 16])
def test_high_inflation_on_turns_10k_cut_at_8(ctx, grids, h):
    c, per = _run(ctx, "turns_10k_s8", h, 2)
    assert _paths(c) == (2 * S.TURNS_N, 0, 0) and S.TURNS_N > grids["wave"] and c["cut_columns"] > 2000


def test_turns_10k_record_order_does_not_matter(ctx, grids):
    c, per = _run(ctx, "turns_10k", 4, 2, rec=S.shuffled(_sets()["turns_10k"][1]))
    assert all(p[0] > grids["wave"] and p[1] > grids["block"] for p in per)
