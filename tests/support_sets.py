"""The sketch sets of the cluster-support tests (tests/test_cpu_support.py, tests/test_gpu_support.py).  Every hash is below 2^32, so
one set serves both widths."""
import functools

import numpy as np

KMER, THRESHOLD = 21, 0.05  # the bound is J = 1 / (2 e^1.05 - 1), about 0.212: 78 of 200 shared is inside (0.242), 64 of 200 outside (0.190)
SIZE = 200


def zigzag(n):
    """the vertex at position p of a path of n: p / 2 for even p, n - 1 - p / 2 for odd p"""
    return [p // 2 if p % 2 == 0 else n - 1 - p // 2 for p in range(n)]


class _Pool:
    """hashes below 2^32 handed out once each"""

    def __init__(self, rng, total):
        self.h = rng.choice(1 << 32, size=total, replace=False).astype(np.uint64)
        self.at = 0

    def take(self, k):
        out = self.h[self.at:self.at + k]
        assert len(out) == k
        self.at += k
        return out


def _tight(pool, rng, m, shared, own=10):
    """m sketches of SIZE hashes over one base: shared[i] (an array, or None) is part of member i as it stands, the rest of the
    member is the base's first hashes with `own` of them replaced by hashes of its own"""
    base = pool.take(SIZE)
    out = []
    for i in range(m):
        fixed = np.zeros(0, dtype=np.uint64) if shared[i] is None else shared[i]
        part = base[:SIZE - len(fixed)].copy()
        part[rng.choice(len(part), size=own, replace=False)] = pool.take(own)
        out.append(np.sort(np.concatenate([fixed, part])))
    return out


@functools.lru_cache(maxsize=None)
def constructed(seed=3):
    """(sketches, groups): the groups are the clusters as built, before the genomes are scattered --
       a cluster of two tight triples joined by one pair that shares 78 of 200 hashes;
       two tight clusters of four whose nearest pair shares 64 of 200;
       a tight cluster of five that stands apart;
       a cluster of 2 + 5 over such a bridge of 78, one member of which shares 64 of 200 with a neighbouring cluster of three;
       a sketch that shares nothing; an empty sketch.
    A bridge's hashes belong to its two sketches alone, so it is the only pair between its two sides."""
    rng = np.random.default_rng(seed)
    pool = _Pool(rng, 40 * SIZE)
    none3, none5 = [None] * 3, [None] * 5
    sketches, groups = [], []

    def add(group):
        groups.append(list(range(len(sketches), len(sketches) + len(group))))
        sketches.extend(group)
    b = pool.take(78)
    add(_tight(pool, rng, 3, [b, None, None]) + _tight(pool, rng, 3, [b, None, None]))
    x = pool.take(64)
    add(_tight(pool, rng, 4, [x] + none3))
    add(_tight(pool, rng, 4, [x] + none3))
    add(_tight(pool, rng, 5, none5))
    b2, x2 = pool.take(78), pool.take(64)
    add(_tight(pool, rng, 2, [b2, None]) + _tight(pool, rng, 5, [b2, None, None, None, x2]))
    add(_tight(pool, rng, 3, [x2, None, None]))
    add([np.sort(pool.take(SIZE))])
    add([np.zeros(0, dtype=np.uint64)])
    order = rng.permutation(len(sketches)).tolist()
    place = {old: new for new, old in enumerate(order)}
    return [sketches[o] for o in order], [sorted(place[g] for g in grp) for grp in groups]


@functools.lru_cache(maxsize=None)
def chain(shift, n=130, seed=9):
    """n sketches of SIZE hashes, consecutive ones shifted by `shift` along one ascending run of hashes, placed at the zigzag
    indices: the sketch at position p shares SIZE - shift hashes with its two neighbours on the path and none with anyone else"""
    rng = np.random.default_rng(seed)
    run = np.sort(rng.choice(1 << 32, size=(n - 1) * shift + SIZE, replace=False).astype(np.uint64))
    out = [None] * n
    for p, v in enumerate(zigzag(n)):
        out[v] = run[p * shift:p * shift + SIZE].copy()
    return out


def _family(rng, m, pool=300, core=5, lo=60, hi=120):
    """m sketches over one pool: a core every member holds and a draw of lo .. hi of the pool's other hashes"""
    every = rng.choice(1 << 32, size=core + pool, replace=False).astype(np.uint64)
    return [np.sort(np.concatenate([every[:core], rng.choice(every[core:], size=int(rng.integers(lo, hi + 1)), replace=False)])) for _ in range(m)]


@functools.lru_cache(maxsize=None)
def paths():
    """(sketches, comp): clusters of 1, 2, 64 and 65 members, each a family of its own, and a cluster of three sketches of about
    1 500 hashes -- past the pair routine's LDS stage -- their genomes interleaved"""
    rng = np.random.default_rng(41)
    sketches, comp = [], []
    for lab, m in enumerate((1, 2, 64, 65)):
        sketches += _family(rng, m)
        comp += [lab] * m
    sketches += _family(rng, 3, pool=1600, core=900, lo=550, hi=650)
    comp += [4] * 3
    order = rng.permutation(len(sketches)).tolist()
    return [sketches[o] for o in order], [comp[o] for o in order]


@functools.lru_cache(maxsize=None)
def dense(n=300, seed=12):
    """(sketches, comp): n sketches that all hold hash 1, so the candidates are the whole triangle and a small edge budget cuts the
    rows into several chunks; seven families by g % 7, each sketch 40 to 70 of its family's 80 hashes and three of its own, and
    every family cut into two clusters, so crossing edges abound"""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n):
        fam = np.arange(80, dtype=np.uint64) * 13 + 100_000 * (g % 7 + 1)
        own = np.arange(3, dtype=np.uint64) + 10_000_000 + 10 * g
        out.append(np.unique(np.concatenate([[1], rng.choice(fam, size=int(rng.integers(40, 71)), replace=False), own]).astype(np.uint64)))
    return out, [g % 14 for g in range(n)]
