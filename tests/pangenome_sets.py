"""The sketch sets of tests/test_gpu_pangenome.py and tests/test_cpu_pangenome.py: every set is (sketches, labels), the sketches
ascending arrays of distinct 32-bit values held as uint64.  materialise() turns them into the hashes of a width: themselves at
width 4, spread over all 64 bits at width 8, with the largest 32-bit value becoming the largest 64-bit one."""
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
