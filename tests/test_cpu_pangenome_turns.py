"""What the device-sized sets of tests/pangenome_sets.py reach, shown without a GPU for 64, 256 and 304 CUs by replaying the launch
grids of rtc_pangenome.hip: every cluster is on the path it is meant for and a path has more clusters than its grid has
workgroups; a cluster that a workgroup counts in a later turn shares hashes with the one it counted before, and counted on top
of that one's table it would give another histogram; with every cluster in the arena the sweep's workgroups cross from table to
table, start in the middle of tables whose all-ones word is set, and leave clusters with filled bins; the counts on either side
of the sweep's last bin sit in one wave.  tests/test_gpu_pangenome_turns.py runs the same sets on the device."""
import functools

import numpy as np
import pytest

from rabbittclust_amd import api
from tests import pangenome_sets as PS
from tests import refpangenome as R

NUM_CU = (64, 256, 304)
WIDTHS = (4, 8)


@functools.lru_cache(maxsize=None)
def _set(name, num_cu):
    return getattr(PS, name)(num_cu)


@functools.lru_cache(maxsize=None)
def _clusters(name, num_cu, width):
    """the clusters of a set in list order: (members' hash arrays, hash -> occ, restatement's histogram) each"""
    sketches, labels = _set(name, num_cu)
    hashes = PS.materialise(sketches, width)
    cluster_of, sizes = R.number_clusters(labels)
    assert cluster_of.tolist() == sorted(cluster_of.tolist())  # the clusters stand in input order: cluster c is the c-th of its list
    clusters, hist, genomes = R.pangenome(hashes, labels)
    assert R.identities(clusters, hist, genomes, labels) == []
    out, at = [], 0
    for c, (m, h) in enumerate(zip(sizes.tolist(), R.cluster_hists(clusters, hist))):
        mem = hashes[at:at + m]
        at += m
        out.append((mem, _occ(mem), [int(x) for x in h]))
    return out


def _occ(members, onto=None):
    """hash -> the members that hold it; onto: counted on top of another cluster's table.  The all-ones value's word is one more
    slot: it is cleared, counted and swept with the table"""
    vals, cnt = np.unique(np.concatenate(list(members) + [np.zeros(0, dtype=np.uint64)]), return_counts=True)
    occ = dict(zip(vals.tolist(), cnt.tolist()))
    for h, f in (onto or {}).items():
        occ[h] = occ.get(h, 0) + f
    return occ


def _hist(occ, m):
    """the histogram the sweep forms of a table's counts: a count above m is left out (rtc_pangenome.hip)"""
    h = [0] * m
    for f in occ.values():
        if 1 <= f <= m:
            h[f - 1] += 1
    return h


def _records(cl):
    return sum(len(s) for s in cl[0])


@pytest.mark.parametrize("num_cu", NUM_CU)
def test_every_cluster_is_on_its_path_and_the_paths_exceed_their_grids(num_cu):
    small = _clusters("many_small", num_cu, 4)
    lay = PS.many_small_layout(num_cu)
    assert len(small) == lay["clusters"] == 2 * api.PAN_GLOBAL_WGS_PER_CU * num_cu + 531
    assert all(_records(cl) <= api.PAN_WAVE_RECORDS for cl in small)  # by records: all on the wave path
    assert len(small) > 3 * api.PAN_WAVE_WGS_PER_CU * num_cu  # a fourth turn
    assert len(small) > 2 * api.PAN_GLOBAL_WGS_PER_CU * num_cu  # RTC_PAN_GLOBAL=1: what the GPU test asserts of global_clusters
    for c in lay["tall"]:
        assert len(small[c][0]) == PS.SMALL_TALL_MEMBERS > api.PAN_WAVE_HIST and _records(small[c]) == 450
    for c in lay["around"]:
        assert len(small[c][0]) <= 5
    for c in lay["big"]:
        assert _records(small[c]) == PS.SMALL_BIG_RECORDS and api.pan_table_log2(PS.SMALL_BIG_RECORDS, True) == 10  # four tiles
    assert abs(len(lay["big"]) - len(small) / PS.SMALL_BIG_EVERY) <= 3
    sizes = {len(cl[0]) for c, cl in enumerate(small) if c not in lay["tall"] and c not in lay["big"]}
    lens = {len(s) for c, cl in enumerate(small) if c not in lay["tall"] and c not in lay["big"] for s in cl[0]}
    assert sizes == {2, 3, 4, 5} and lens == {0, 1, 2, 3, 4, 5}
    distinct = set()
    for cl in small:
        distinct |= set(cl[1])
    assert len(distinct) == PS.SMALL_POOL + 1  # the pool and the all-ones value

    block = _clusters("many_block", num_cu, 4)
    lay = PS.many_block_layout(num_cu)
    assert len(block) == lay["clusters"] == api.PAN_BLOCK_WGS_PER_CU * num_cu + 37 > api.PAN_BLOCK_WGS_PER_CU * num_cu
    assert all(api.PAN_WAVE_RECORDS < _records(cl) <= api.PAN_BLOCK_RECORDS for cl in block)
    assert _records(block[1]) == api.PAN_WAVE_RECORDS + 1 and _records(block[2]) == api.PAN_BLOCK_RECORDS
    for c in lay["tall"]:
        assert len(block[c][0]) == PS.BLOCK_TALL_MEMBERS > api.PAN_BLOCK_HIST and _records(block[c]) == 1500
    assert all(2 <= len(cl[0]) <= 4 for c, cl in enumerate(block) if c not in lay["tall"])


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("num_cu", NUM_CU)
@pytest.mark.parametrize("name,per_cu,hist_entries", [("many_small", api.PAN_WAVE_WGS_PER_CU, api.PAN_WAVE_HIST),
                                                      ("many_block", api.PAN_BLOCK_WGS_PER_CU, api.PAN_BLOCK_HIST)])
def test_a_later_turn_meets_the_keys_of_the_turn_before(name, per_cu, hist_entries, num_cu, width):
    """pan_lds_kernel: workgroup b counts the clusters b, b + grid, b + 2 grid, ... of the list into the same LDS arrays"""
    cls = _clusters(name, num_cu, width)
    lay = getattr(PS, name + "_layout")(num_cu)
    grid = min(len(cls), per_cu * num_cu)
    assert grid == lay["grid"] < len(cls)
    later = differ = 0
    for c in range(grid, len(cls)):
        mem, occ, hist = cls[c]
        before = cls[c - grid][1]
        assert set(occ) & set(before), c  # a slot left from the turn before is a slot of this cluster
        assert _hist(occ, len(mem)) == hist  # the model, cleared, is the restatement
        later += 1
        differ += _hist(_occ(mem, onto=before), len(mem)) != hist
    assert later == len(cls) - grid and 10 * differ >= 9 * later, (differ, later)
    # the clusters whose histogram does not fit the LDS copy: from the copy to global adds and back, in one workgroup
    second, first = lay["tall"]
    assert grid <= second < 2 * grid and first < grid < first + grid < len(cls)
    fits = lambda c: len(cls[c][0]) <= hist_entries  # noqa: E731
    assert fits(second - grid) and not fits(second) and not fits(first) and fits(first + grid)
    if name == "many_small":
        assert second + grid < len(cls) and fits(second + grid)
    for c in (second, first + grid) + ((second + grid,) if name == "many_small" else ()):
        assert _hist(_occ(cls[c][0], onto=cls[c - grid][1]), len(cls[c][0])) != cls[c][2], c


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("num_cu", NUM_CU)
def test_the_sweep_crosses_tables_and_starts_inside_them(num_cu, width):
    """pan_sweep_kernel over many_small with every cluster in the arena: aoff and the tile split tiles * b / B, replayed"""
    cls = _clusters("many_small", num_cu, width)
    slots = [1 << api.pan_table_log2(_records(cl), True) for cl in cls]
    aoff = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
    tiles = int(aoff[-1]) >> 8
    B = min(tiles, api.PAN_GLOBAL_WGS_PER_CU * num_cu)
    assert B == api.PAN_GLOBAL_WGS_PER_CU * num_cu and tiles > 2 * B  # more than two tiles a workgroup
    ones = [cl[1].get(api.PAN_EMPTY, 0) if width == 8 else 0 for cl in cls]  # at width 4 the largest value is a key like any other
    several = inside = inside_ones = leaves = 0
    offsets = set()
    for b in range(B):
        t0, t1 = tiles * b // B, tiles * (b + 1) // B
        assert t1 - t0 >= 2
        table = (np.searchsorted(aoff, np.arange(t0, t1) << 8, side="right") - 1).tolist()  # the table of every tile of the workgroup
        several += table[0] != table[-1]
        for i, a in enumerate(table):
            if (t0 + i) << 8 == int(aoff[a]):
                offsets.add(i)  # a table begins at the workgroup's i-th tile
        if t0 << 8 != int(aoff[table[0]]):
            inside += 1
            inside_ones += ones[table[0]] > 0
        for a, nxt in zip(table, table[1:]):
            if a == nxt or slots[a] != 256 or (a == table[0] and t0 << 8 != int(aoff[a])):
                continue  # a table of one tile that the workgroup swept whole
            m = len(cls[a][0])
            filled = any(2 <= f < m for f in cls[a][1].values())
            leaves += filled and cls[a][2] != cls[nxt][2]
    assert 2 * several >= B, (several, B)
    assert offsets >= {0, 1, 2}  # table boundaries at every offset of a workgroup's range
    assert inside >= 20 and leaves >= 20, (inside, leaves)
    if width == 8:
        assert inside_ones >= 20, inside_ones
    else:
        assert inside_ones == 0


def _probe(keys, lg):
    """the slots linear probing gives the keys of a table of 1 << lg slots, in this insertion order"""
    taken = {}
    for k in keys:
        s = api.pan_slot(k, lg)
        while s in taken:
            s = (s + 1) & ((1 << lg) - 1)
        taken[s] = k
    return {k: s for s, k in taken.items()}


@pytest.mark.parametrize("width", WIDTHS)
def test_past_the_bins_holds_its_counts_in_one_wave(width):
    sketches, labels = PS.past_the_bins(width)
    hashes = PS.materialise(sketches, width)
    m = len(sketches)
    assert m == PS.BINS_MEMBERS == 1100 and set(labels) == {0}
    records = sum(len(s) for s in hashes)
    assert records == sum(PS.BINS_COUNTS) == 10481 > api.PAN_BLOCK_RECORDS  # the arena in either mode
    lg = api.pan_table_log2(records)
    assert lg == 15 == api.pan_table_log2(records, True)
    occ = _occ(hashes)
    assert sorted(occ.values()) == sorted(PS.BINS_COUNTS) and len(occ) == 12
    keys = sorted(occ)
    for order in (keys, keys[::-1], keys[5:] + keys[:5]):  # whichever member's wave claims first
        at = _probe(order, lg)
        assert {s >> 6 for s in at.values()} == {PS.BINS_RUN}, order  # one 64-slot run: one wave of one tile
        assert sorted(at.values()) == sorted(_probe(keys, lg).values())
    counts = sorted(occ.values())
    bins = api.PAN_SWEEP_BINS
    assert bins + 1 in counts and bins + 2 in counts  # the last count with a bin and the first without
    past = [f for f in counts if f - 2 >= bins and f != m]
    assert len(past) > len(set(past)) >= 2  # equal ones and different ones: the ballot that gathers equal counts
    assert counts.count(bins + 1) >= 2 and m in counts and 1 in counts and 2 in counts
    clusters, hist, genomes = R.pangenome(hashes, labels)
    assert R.identities(clusters, hist, genomes, labels) == []
    assert [int(hist[f - 1]) for f in (1, 2, 1025, 1026, 1027, 1099, 1100)] == [1, 1, 3, 3, 1, 2, 1] and int(hist.sum()) == 12
