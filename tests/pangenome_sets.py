"""The sketch sets of tests/test_gpu_pangenome.py and tests/test_cpu_pangenome.py: every set is (sketches, labels), the sketches
ascending arrays of distinct 32-bit values held as uint64.  materialise() turns them into the hashes of a width: themselves at
width 4, spread over all 64 bits at width 8, with the largest 32-bit value becoming the largest 64-bit one.  The sets at the end
take the device's CU count and have more clusters than a launch has workgroups (tests/test_cpu_pangenome_turns.py shows what they
reach, tests/test_gpu_pangenome_turns.py runs them)."""
import numpy as np

from rabbittclust_amd import api

ONES32 = 0xFFFFFFFF


def widen(s):
    """a strictly increasing map of the 32-bit values onto hashes that use all 64 bits (tests/test_gpu_support.py: _widen); the
    all-ones value stays all ones"""
    s = np.asarray(s, dtype=np.uint64)
    out = (s << np.uint64(32)) | ((s * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF))
    out[s == np.uint64(ONES32)] = np.uint64(api.PAN_EMPTY)
    return out


def materialise(sketches, width):
    return [np.asarray(s, dtype=np.uint64) if width == 4 else widen(s) for s in sketches]


def _sk(values):
    return np.unique(np.asarray(list(values), dtype=np.uint64))


def family(rng, members, core, shell, own, base):
    """a cluster: `core` hashes everybody holds, `shell` hashes each held by a random half, `own` hashes per member; values from
    base on, below base + 2^20"""
    pool = base + rng.choice(1 << 20, size=core + shell + own * members, replace=False).astype(np.uint64)
    c, s, o = pool[:core], pool[core:core + shell], pool[core + shell:]
    out = []
    for i in range(members):
        keep = s[rng.random(shell) < 0.5]
        out.append(_sk(np.concatenate([c, keep, o[i * own:(i + 1) * own]])))
    return out


def exact_records(rng, members, records, base):
    """a cluster of exactly `records` records over `members` members that share about a third of their hashes"""
    per = [records // members + (1 if i < records % members else 0) for i in range(members)]
    shared = base + np.arange(per[-1] // 3, dtype=np.uint64) * np.uint64(7)
    out, at = [], base + (1 << 18)
    for p in per:
        own = at + np.arange(p - len(shared), dtype=np.uint64) * np.uint64(3)
        at += 3 * p + 11
        out.append(_sk(np.concatenate([shared, own])))
        assert len(out[-1]) == p
    return out


def path_edges():
    """four clusters whose record counts sit at and one past the two LDS limits, interleaved in input order"""
    rng = np.random.default_rng(5)
    groups = [exact_records(rng, 4, api.PAN_WAVE_RECORDS, 1 << 21), exact_records(rng, 3, api.PAN_WAVE_RECORDS + 1, 2 << 21),
              exact_records(rng, 8, api.PAN_BLOCK_RECORDS, 3 << 21), exact_records(rng, 3, api.PAN_BLOCK_RECORDS + 1, 4 << 21)]
    sketches, labels = [], []
    for i in range(8):
        for c, grp in enumerate(groups):
            if i < len(grp):
                sketches.append(grp[i])
                labels.append(c)
    return sketches, labels


def wide():
    """300 members that share 5 hashes and hold one of their own each: occ and m past a wave and past 256"""
    shared = [10, 20, 30, 40, 50]
    return [_sk(shared + [1000 + i]) for i in range(300)], [0] * 300


def tall():
    """cluster 0: 1 100 members of 3 hashes (one everybody's, one of seven, one own): the histogram has 1 100 entries.
    cluster 1: 1 100 members of whom 100 hold 15 hashes and the rest nothing: a workgroup-path cluster whose histogram does not
    fit its LDS copy"""
    a = [_sk([7, 100 + i % 7, 10_000 + i]) for i in range(1100)]
    b = [_sk([5] + [200_000 + 14 * (i // 11) + k for k in range(14)]) if i % 11 == 0 else _sk([]) for i in range(1100)]
    return a + b, [0] * 1100 + [1] * 1100


def second_turn(members):
    """one cluster of `members` members of 3 hashes: one everybody's, one shared by 50, one own"""
    return [_sk([3, 1_000 + i // 50, 1_000_000 + i]) for i in range(members)], [0] * members


def wrapping(width, members=10, per=250):
    """one arena cluster of members x per records; four of everybody's hashes start their probe in the table's last slot"""
    records = members * per
    lg = api.pan_table_log2(records)
    assert lg is not None
    vals = np.arange(1, 400_000, dtype=np.uint64)
    keys = vals if width == 4 else widen(vals)
    with np.errstate(over="ignore"):
        slots = (keys * np.uint64(api.PAN_MULT)) >> np.uint64(64 - lg)
    last = vals[slots == np.uint64((1 << lg) - 1)][:4]
    assert len(last) == 4
    for v in last.tolist():
        key = v if width == 4 else int(widen([v])[0])
        assert api.pan_slot(key, lg) == (1 << lg) - 1
    out = []
    for i in range(members):
        own = 500_000 + i * 1000 + np.arange(per - 4, dtype=np.uint64)
        out.append(_sk(np.concatenate([last, own])))
        assert len(out[-1]) == per
    return out, [0] * members


def markers():
    """0 and the all-ones value in clusters of every path: held by all, by some, by one"""
    rng = np.random.default_rng(9)
    sketches, labels = [], []
    for c, (members, per) in enumerate(((3, 40), (6, 200), (9, 300))):  # 120, 1 200 and 2 700 records
        fam = family(rng, members, per // 2, per // 4, per // 4, (c + 1) << 21)
        for i, s in enumerate(fam):
            extra = ([0] if i % 2 == 0 else []) + ([ONES32] if i != 1 else [])
            sketches.append(_sk(np.concatenate([s, np.asarray(extra, dtype=np.uint64)])))
            labels.append(c)
    sketches += [_sk([0]), _sk([ONES32]), _sk([0, ONES32]), _sk([0, 17, ONES32])]  # singletons, and a pair
    labels += [3, 4, 5, 5]
    return sketches, labels


def mixed_labels():
    """families under arbitrary label numbers, with unclustered genomes and empty sketches among them, shuffled"""
    rng = np.random.default_rng(21)
    fams = [family(rng, 5, 30, 20, 4, 1 << 21), family(rng, 12, 100, 80, 10, 2 << 21), family(rng, 20, 90, 60, 6, 3 << 21),
            family(rng, 1, 25, 0, 0, 4 << 21), family(rng, 2, 0, 0, 9, 5 << 21)]
    sketches, cluster = [], []
    for c, fam in enumerate(fams):
        sketches += fam
        cluster += [c] * len(fam)
    sketches += [_sk([]), _sk([]), _sk([])]      # empty sketches: in family 1, in a cluster of their own, unclustered
    cluster += [1, 5, -1]
    sketches += family(rng, 3, 10, 5, 2, 6 << 21)  # unclustered genomes with hashes
    cluster += [-1, -2, -7]
    order = rng.permutation(len(sketches))
    sketches = [sketches[i] for i in order]
    cluster = [cluster[i] for i in order]
    n = len(sketches)
    names = {c: int(v) for c, v in zip(range(6), rng.choice(n, size=6, replace=False))}  # any number below n
    return sketches, [names[c] if c >= 0 else c for c in cluster]


def several_arena(clusters=6):
    """`clusters` arena clusters of 8 x about 300 records each (8 192 slots a table) and two small ones between them"""
    rng = np.random.default_rng(33)
    sketches, labels = [], []
    for c in range(clusters):
        fam = family(rng, 8, 150, 240, 30, (c + 1) << 21)
        assert api.PAN_BLOCK_RECORDS < sum(len(s) for s in fam) <= 4096
        sketches += fam
        labels += [2 * c] * 8
        if c in (1, 3):
            sketches += family(rng, 2, 10, 0, 3, (c + 20) << 21)
            labels += [2 * c + 1] * 2
    return sketches, labels


def thresholds(m):
    """one cluster of m: hash f is held by the members 0 .. f - 1, f = 1 .. m"""
    return [_sk(range(i + 1, m + 1)) for i in range(m)], [0] * m


def small_identity_sets():
    """what the restatement's own identities are checked on without a GPU"""
    return {"edges": path_edges(), "wide": wide(), "markers": markers(), "labels": mixed_labels(), "arena": several_arena(3),
            "m7": thresholds(7), "m20": thresholds(20)}


# ---- sets sized from the device: a workgroup's second turn, the sweep across tables, counts past the sweep's bins ----------------
# The clusters of these sets stand in input order, so cluster c is the c-th of its path's list and, with a grid of G workgroups,
# workgroup c % G meets it in turn c // G.  All clusters of a set draw from one small pool: successive clusters of a workgroup
# hold the same keys, so a slot that was not cleared changes a count.
SMALL_POOL, SMALL_BIG_EVERY, SMALL_BIG_MEMBERS, SMALL_BIG_RECORDS, SMALL_TALL_MEMBERS, SMALL_TALL_HOLDERS = 24, 50, 20, 300, 600, 150
BLOCK_POOL, BLOCK_TALL_MEMBERS, BLOCK_TALL_HOLDERS = 700, 1100, 100


def _pool(seed, size):
    """`size` distinct values below 2^31, ascending, 0 among them"""
    vals = np.random.default_rng(seed).choice(1 << 31, size=size - 1, replace=False).astype(np.uint64)
    return np.unique(np.concatenate([vals, np.zeros(1, dtype=np.uint64)]))


def many_small_layout(num_cu):
    """where the special clusters of many_small stand: `tall` (of SMALL_TALL_MEMBERS members) once in a workgroup's second turn,
    between two small clusters of the same workgroup, and once in the first turn; `big` (of SMALL_BIG_RECORDS records) about every
    SMALL_BIG_EVERY-th of the others"""
    grid = api.PAN_WAVE_WGS_PER_CU * num_cu
    n = 2 * api.PAN_GLOBAL_WGS_PER_CU * num_cu + 531
    p, q = grid // 3 + 7, grid // 6 + 3
    assert q + grid < p + grid < p + 2 * grid < n and p != q
    small = {p, p + 2 * grid, q + grid}  # the clusters the two tall ones' workgroups meet before and after them
    tall = (p + grid, q)
    big = [c for c in range(SMALL_BIG_EVERY // 2, n, SMALL_BIG_EVERY) if c not in small and c not in tall]
    return {"clusters": n, "grid": grid, "tall": tall, "big": big, "around": sorted(small)}


def many_small(num_cu):
    """2 * PAN_GLOBAL_WGS_PER_CU * num_cu + 531 clusters over a pool of SMALL_POOL values, all on the wave path by their records:
    small ones of 2 to 5 members with 0 to 5 hashes each -- one member of every cluster holds the pool's first value, and the
    all-ones value is in every fifth (cluster + member) -- big ones of 20 members and 300 records (1 024 slots, four tiles, where
    every cluster is in the arena), and two of 600 members of whom 150 hold 3 hashes: 450 records, and more members than the
    wave path's LDS histogram has entries."""
    lay = many_small_layout(num_cu)
    rng = np.random.default_rng(61)
    pool = _pool(60, SMALL_POOL)
    big = set(lay["big"])
    sketches, labels = [], []
    for c in range(lay["clusters"]):
        first = len(sketches)
        if c in lay["tall"]:
            for j in range(SMALL_TALL_MEMBERS):
                k = j // 4
                sketches.append(_sk([pool[0], pool[1 + k % 5], pool[6 + k % 7]] if j % 4 == 0 else []))
        elif c in big:
            for j in range(SMALL_BIG_MEMBERS):
                per = SMALL_BIG_RECORDS // SMALL_BIG_MEMBERS
                ones = [ONES32] if j % 3 == 0 else []
                sketches.append(_sk(rng.choice(pool, size=per - len(ones), replace=False).tolist() + ones))
                assert len(sketches[-1]) == per
        else:
            members = int(rng.integers(2, 6))
            for i in range(members):
                held = rng.choice(pool, size=int(rng.integers(0, 4)), replace=False).tolist()
                held += [int(pool[0])] if i == c % members else []
                held += [ONES32] if (c + i) % 5 == 0 else []
                sketches.append(_sk(held))
        labels += [first] * (len(sketches) - first)
    return sketches, labels


def many_block_layout(num_cu):
    """many_block's two clusters of BLOCK_TALL_MEMBERS members: one in a workgroup's second turn behind an ordinary cluster, one in
    the first turn in front of one"""
    grid = api.PAN_BLOCK_WGS_PER_CU * num_cu
    return {"clusters": grid + 37, "grid": grid, "tall": (5 + grid, 11)}


def many_block(num_cu):
    """PAN_BLOCK_WGS_PER_CU * num_cu + 37 clusters over a pool of BLOCK_POOL values, all on the workgroup path: 2 to 4 members that
    together hold 513 to 2 048 records (clusters 1 and 2 exactly those), and two clusters of 1 100 members of whom 100 hold 15
    hashes: more members than the path's LDS histogram has entries"""
    lay = many_block_layout(num_cu)
    rng = np.random.default_rng(71)
    pool = _pool(70, BLOCK_POOL)
    lo, hi = api.PAN_WAVE_RECORDS + 1, api.PAN_BLOCK_RECORDS
    sketches, labels = [], []
    for c in range(lay["clusters"]):
        first = len(sketches)
        if c in lay["tall"]:
            for j in range(BLOCK_TALL_MEMBERS):
                at = 1 + 14 * ((j // 11) % 49)
                sketches.append(_sk([pool[0]] + pool[at:at + 14].tolist() if j % 11 == 0 else []))
        else:
            records = lo if c == 1 else hi if c == 2 else int(rng.integers(1100, hi + 1)) if c % 7 == 0 else int(rng.integers(lo, 1100))
            members = max(int(rng.integers(2, 5)), -(-records // 600))
            for i in range(members):
                per = records // members + (1 if i < records % members else 0)
                sketches.append(_sk(rng.choice(pool, size=per, replace=False)))
                assert len(sketches[-1]) == per
        labels += [first] * (len(sketches) - first)
    return sketches, labels


BINS_MEMBERS = 1100
BINS_COUNTS = (1, 2, 1025, 1025, 1025, 1026, 1026, 1026, 1027, 1099, 1099, BINS_MEMBERS)  # PAN_SWEEP_BINS + 1 is the last count with a bin
BINS_RUN, BINS_HOMES = 5, 40  # the 64-slot run of the table the twelve hashes live in, and how far into it their probes start


def past_the_bins(width):
    """one arena cluster of 1 100 members and twelve hashes, hash k held by the members 0 .. BINS_COUNTS[k] - 1: the counts on
    either side of the sweep's last bin, equal and different ones past it, in one wave of one tile.  The twelve values start
    their probes in the first BINS_HOMES slots of one 64-aligned run of the table (api.pan_slot), so wherever linear probing puts
    them, they stay in that run."""
    lg = api.pan_table_log2(sum(BINS_COUNTS))
    assert lg is not None and BINS_HOMES + len(BINS_COUNTS) <= 64
    vals = np.arange(1, 2_000_000, dtype=np.uint64)
    keys = vals if width == 4 else widen(vals)
    with np.errstate(over="ignore"):
        slots = (keys * np.uint64(api.PAN_MULT)) >> np.uint64(64 - lg)
    held = vals[((slots >> np.uint64(6)) == np.uint64(BINS_RUN)) & ((slots & np.uint64(63)) < np.uint64(BINS_HOMES))][:len(BINS_COUNTS)]
    assert len(held) == len(BINS_COUNTS)
    for v in held.tolist():
        key = v if width == 4 else int(widen([v])[0])
        assert api.pan_slot(key, lg) >> 6 == BINS_RUN and api.pan_slot(key, lg) & 63 < BINS_HOMES
    return [_sk(v for v, f in zip(held.tolist(), BINS_COUNTS) if i < f) for i in range(BINS_MEMBERS)], [0] * BINS_MEMBERS
