"""rtc_pangenome past one turn of its grids: the device-sized sets of tests/pangenome_sets.py (many_small, many_block,
past_the_bins; tests/test_cpu_pangenome_turns.py shows what they reach) against the restatement, exactly, through the check of
tests/test_gpu_pangenome.py.  A workgroup of pan_lds_kernel counts a second, third and fourth cluster into its LDS arrays, among
them clusters whose histogram does not fit the LDS copy; with every cluster in the arena a workgroup of pan_sweep_kernel takes
several tiles across several tables; counts on either side of the sweep's last bin meet in one wave; and a byte budget reuses
the per-group buffers with LDS clusters in them.  The path counters are asserted against the grids, and every case prints the
restatement's time and the call's."""
import time

import pytest

import test_gpu_pangenome as T  # the module pytest itself imports: its sets and its shared references
from test_gpu_pangenome import switch  # noqa: F401  (the fixture)
from tests import pangenome_sets as PS

pytestmark = pytest.mark.gpu

_CU = []  # the device's CU count, known once a test holds the context

T._SETS.update({
    "many_small": lambda w: PS.many_small(_CU[0]),
    "many_block": lambda w: PS.many_block(_CU[0]),
    "bins": lambda w: PS.past_the_bins(w),
})
T._PATHS["bins"] = (0, 0, 1)


def _timed_check(ctx, name, width, mode, switch):
    from rabbittclust_amd import api
    if not _CU:
        _CU.append(ctx.num_cu())
    assert _CU[0] == ctx.num_cu()
    t0 = time.perf_counter()
    hashes, labels, want = T._reference(name, width)
    t1 = time.perf_counter()
    cnt = T._check(ctx, name, width, mode, switch)
    t2 = time.perf_counter()
    print("%s-%d-%s: %d sketches, %d records, %d clusters (wave %d, workgroup %d, arena %d), %d group(s); set and restatement %.2f s "
          "(0 when shared), upload, GPU call and comparison %.3f s, the call %.4f s, its kernels %.4f s" %
          (name, width, mode, len(hashes), cnt["records"], cnt["clusters"], cnt["wave_clusters"], cnt["block_clusters"], cnt["global_clusters"],
           cnt["groups"], t1 - t0, t2 - t1, cnt["total_ns"] / 1e9, cnt["kernel_ns"] / 1e9))
    return cnt, want, api


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("width", T.WIDTHS)
def test_many_small_clusters(ctx, switch, width, mode):
    cnt, want, api = _timed_check(ctx, "many_small", width, mode, switch)
    num_cu = ctx.num_cu()
    assert cnt["clusters"] == 2 * api.PAN_GLOBAL_WGS_PER_CU * num_cu + 531
    if mode == "paths":
        assert cnt["wave_clusters"] > api.PAN_WAVE_WGS_PER_CU * num_cu and cnt["wave_clusters"] == cnt["clusters"]
        assert (cnt["block_clusters"], cnt["global_clusters"]) == (0, 0) and ctx.pangenome_last_path() == api.PAN_PATH_WAVE
    else:
        assert cnt["global_clusters"] > 2 * api.PAN_GLOBAL_WGS_PER_CU * num_cu and ctx.pangenome_last_path() == api.PAN_PATH_GLOBAL
    assert cnt["groups"] == 1
    assert int(want[0]["size"].max()) == PS.SMALL_TALL_MEMBERS > api.PAN_WAVE_HIST


@pytest.mark.parametrize("width", T.WIDTHS)
def test_many_workgroup_clusters(ctx, switch, width):
    cnt, want, api = _timed_check(ctx, "many_block", width, "paths", switch)
    num_cu = ctx.num_cu()
    assert cnt["block_clusters"] > api.PAN_BLOCK_WGS_PER_CU * num_cu and cnt["block_clusters"] == cnt["clusters"]
    assert (cnt["wave_clusters"], cnt["global_clusters"]) == (0, 0) and ctx.pangenome_last_path() == api.PAN_PATH_BLOCK
    assert int(want[0]["size"].max()) == PS.BLOCK_TALL_MEMBERS > api.PAN_BLOCK_HIST


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("width", T.WIDTHS)
def test_counts_past_the_sweeps_bins(ctx, switch, width, mode):
    cnt, want, api = _timed_check(ctx, "bins", width, mode, switch)  # the arena in either mode: T._PATHS
    assert (cnt["wave_clusters"], cnt["block_clusters"], cnt["global_clusters"]) == (0, 0, 1)
    hist = want[1]
    assert int(hist[api.PAN_SWEEP_BINS]) == 3 and int(hist[api.PAN_SWEEP_BINS + 1]) == 3  # occ 1 025: the last bin; 1 026: past them


@pytest.mark.parametrize("width", T.WIDTHS)
def test_groups_of_lds_clusters_reuse_the_buffers(ctx, switch, width):
    """RTC_PAN_BYTES at a third of what the set is charged: three groups or more, each with wave-path clusters, through the same
    per-group buffers"""
    from rabbittclust_amd import api
    if not _CU:
        _CU.append(ctx.num_cu())
    hashes, labels, want = T._reference("many_small", width)
    charged = [api.pan_cluster_bytes(int(r["total"]), int(r["size"])) for r in want[0]]
    assert max(charged) < sum(charged) // 3
    switch("RTC_PAN_BYTES", sum(charged) // 3)
    cnt, _, _ = _timed_check(ctx, "many_small", width, "paths", switch)
    assert cnt["groups"] >= 3, cnt
    assert cnt["wave_clusters"] == cnt["clusters"] > api.PAN_WAVE_WGS_PER_CU * ctx.num_cu()
