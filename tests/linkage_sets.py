"""The key matrices and sketch sets of the complete-linkage tests (tests/test_cpu_linkage.py, tests/test_gpu_linkage.py)."""
import numpy as np

# 1, 2, 3; 63, 64: the wave path and its last size; 65: the workgroup path's first; 257: past one turn of 256 lanes; 300
SIZES = (1, 2, 3, 63, 64, 65, 257, 300)


def _sym(m, fn):
    k = np.zeros((m, m, 2), dtype=np.uint32)
    for i in range(m):
        for j in range(i):
            k[i, j] = k[j, i] = fn(j, i)  # fn(lo, hi)
    return k


def all_equal(m):
    """every key 1 / 2: the tie rule decides every step"""
    return _sym(m, lambda i, j: (1, 2))


def equal_kappa(m):
    """kappa 1 / 2 everywhere, written 1 / 2, 2 / 4 and 3 / 6: the reported denom is the smallest between the two clusters --
    2 / 4 for the first merge (0, 1), 1 / 2 from then on, since cluster 0 has a pair written 1 / 2 with every other point"""
    return _sym(m, lambda i, j: ((1, 2), (2, 4), (3, 6))[(i + j) % 3])


def star(m):
    """kappa(i, j) falls with max(i, j): the merges are (0, 1), (0, 2), ... and every live row's best partner is cluster 0, the
    cluster being merged, at every step (ties go to the smallest index) -- every row looks again every step"""
    return _sym(m, lambda i, j: (2 * m - j, 2 * m))


def chain(m):
    """kappa falls with |i - j|: neighbours tie at the top, the dendrogram pairs them up level by level"""
    return _sym(m, lambda i, j: (2 * m - (j - i), 3 * m))


def zeros(m):
    """kappa 0 everywhere, under several denominators and 0 / 0: no merge"""
    return _sym(m, lambda i, j: (0, (i + j) % 4))


def near_2_31(m, seed=5):
    """counts just below 2^31 over denominators just below 2^32: quotients that differ only in the low bits of the 64-bit products"""
    rng = np.random.default_rng(seed)
    c = rng.integers((1 << 31) - 4 * m, 1 << 31, size=(m, m))
    d = rng.integers((1 << 32) - 8 * m, 1 << 32, size=(m, m))
    return _sym(m, lambda i, j: (int(c[i, j]), int(d[i, j])))


def random_ties(m, seed=1):
    """small counts: many equal kappa under different denominators, some zeros"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 9, size=(m, m))
    c = rng.integers(0, 9, size=(m, m)) % (d + 1)
    return _sym(m, lambda i, j: (int(c[i, j]), int(d[i, j])))


def tie_free(m, seed=2):
    """distinct kappa: common i / denom 10^6 + 1 over a shuffled run of distinct counts (what scipy's linkage can be compared on)"""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(np.arange(1, m * m + 1))[: m * (m - 1) // 2] * 3 + 1000
    it = iter(vals.tolist())
    return _sym(m, lambda i, j: (next(it), 4 * m * m + 2000))


CASES = {"all_equal": all_equal, "equal_kappa": equal_kappa, "star": star, "chain": chain, "zeros": zeros, "near_2_31": near_2_31,
         "random_ties": random_ties, "tie_free": tie_free}


def median_bound(keys):
    """a stop bound inside the matrix: the median kappa above 0 as (num, den), which ends the run mid-way"""
    m = keys.shape[0]
    ks = sorted({(int(keys[i, j, 0]), int(keys[i, j, 1])) for i in range(m) for j in range(i) if keys[i, j, 0] and keys[i, j, 1]},
                key=lambda k: k[0] / k[1])
    return ks[len(ks) // 2] if ks else (1, 2)


# ---- sketch sets for rtc_linkage_complete ----------------------------------------------------------------------------------
COMPONENT_SIZES = (64, 130, 65, 5, 2, 1, 1)  # in order of their smallest member: genomes 0, 1, 2, ... open them


def component_set(seed=3):
    """(sketches, comp): components of 64, 130, 65, 5, 2, 1 and 1 sketches under scattered genome indices; every component draws
    its sketches from a pool of its own (20 to 60 of 100 hashes each, so the pairs of a component share from nothing to most);
    one member of the 5 is empty; the labels are arbitrary numbers, none of them the smallest member."""
    rng = np.random.default_rng(seed)
    n = sum(COMPONENT_SIZES)
    nc = len(COMPONENT_SIZES)
    rest = rng.permutation(np.arange(nc, n)).tolist()
    comp = [0] * n
    labels = [900 - 7 * c for c in range(nc)]
    members = []
    for c, m in enumerate(COMPONENT_SIZES):
        mem = [c] + [rest.pop() for _ in range(m - 1)]
        members.append(sorted(mem))
        for g in mem:
            comp[g] = labels[c]
    sketches = [None] * n
    for c, mem in enumerate(members):
        pool = np.arange(100, dtype=np.uint64) * 1009 + 1_000_003 * (c + 1)
        for g in mem:
            take = int(rng.integers(20, 61))
            sketches[g] = np.sort(rng.choice(pool, size=take, replace=False))
    sketches[members[3][2]] = np.zeros(0, dtype=np.uint64)
    return sketches, comp


def block_bytes(m):
    return 8 * m * m


def band_bytes(m):
    """the smallest band of a component's fill: 64 rows (or all of them) of u32 counts"""
    return 4 * m * min(m, 64)
