"""The sketch sets of the jackknife-support tests (tests/test_cpu_nj_support.py, tests/test_gpu_nj_support.py).  Every hash is
below 2^32, so one set serves both widths and one restatement both."""
import functools

import numpy as np


def family(rng, m, subs, pool=200, core=10, lo=30, hi=190):
    """m sketches in `subs` subfamilies (member i in subfamily i % subs): a core of `core` hashes every member holds, a pool of
    `pool` hashes per subfamily, and every member a draw of lo .. hi of its pool's -- 40 to 200 hashes a sketch as the defaults go.
    Ascending uint64 arrays."""
    every = rng.choice(1 << 32, size=core + subs * pool, replace=False).astype(np.uint64)
    out = []
    for i in range(m):
        s = i % subs
        mine = every[core + s * pool:core + (s + 1) * pool]
        take = rng.choice(mine, size=int(rng.integers(lo, hi + 1)), replace=False)
        out.append(np.sort(np.concatenate([every[:core], take])))
    return out


# Two subfamilies of four over two pools of 200 hashes and a shared core of 12: members 0 .. 3 draw 150 to 190 hashes of pool A,
# members 4 .. 7 of pool B.  Between the subfamilies only the core is common, inside one about three quarters of a sketch, so the
# branch between them is in every replicate and the order inside a subfamily is decided by a handful of hashes.
CONSTRUCTED = dict(seed=5, pool=200, core=12, lo=150, hi=190)


@functools.lru_cache(maxsize=None)
def constructed():
    p = CONSTRUCTED
    rng = np.random.default_rng(p["seed"])
    every = rng.choice(1 << 32, size=p["core"] + 2 * p["pool"], replace=False).astype(np.uint64)
    out = []
    for i in range(8):
        s = i // 4
        mine = every[p["core"] + s * p["pool"]:p["core"] + (s + 1) * p["pool"]]
        take = rng.choice(mine, size=int(rng.integers(p["lo"], p["hi"] + 1)), replace=False)
        out.append(np.sort(np.concatenate([every[:p["core"]], take])))
    return out


@functools.lru_cache(maxsize=None)
def component_set():
    """(sketches, comp): components of 1, 2, 3, 4, 5, 64 and 65 members, their genomes interleaved, each a family of its own with
    subfamilies of about eight"""
    rng = np.random.default_rng(77)
    sizes = (1, 2, 3, 4, 5, 64, 65)
    sketches, comp = [], []
    for lab, m in enumerate(sizes):
        sketches += family(rng, m, max(1, m // 8))
        comp += [lab] * m
    order = rng.permutation(len(sketches)).tolist()
    return [sketches[o] for o in order], [comp[o] for o in order]


@functools.lru_cache(maxsize=None)
def six():
    """one component of six in two subfamilies"""
    return family(np.random.default_rng(78), 6, 2)
