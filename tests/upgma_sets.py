"""The sum matrices of the average-linkage tests (tests/test_cpu_upgma.py, tests/test_gpu_upgma.py).  Every set is
(name, S as a list of lists of Python integers, sizes or None)."""
import numpy as np

Q1 = 1 << 20

# 2, 3; 63, 64: the wave path and its last size; 65: the workgroup path's first; 257: past one turn of 256 lanes
SIZES = (2, 3, 63, 64, 65, 257)


def _sym(m, fn):
    S = [[0] * m for _ in range(m)]
    for i in range(m):
        for j in range(i):
            S[i][j] = S[j][i] = int(fn(j, i))  # fn(lo, hi)
    return S


def random_ties(m, seed=1):
    """q from nine values between 0 and Q1: equal means at every step, and after the first merges equal means under different
    sizes"""
    rng = np.random.default_rng(seed + m)
    v = rng.integers(0, 9, size=(m, m)) * (Q1 // 8)
    return _sym(m, lambda i, j: v[i, j])


def tie_free(m, seed):
    """distinct q in [1, Q1): what scipy's linkage can be compared on"""
    rng = np.random.default_rng(seed)
    vals = iter((rng.permutation(Q1 - 1)[: m * (m - 1) // 2] + 1).tolist())
    return _sym(m, lambda i, j: next(vals))


def all_q1(m):
    """every pair at distance 1: the tie rule decides every step, which makes the merges (0, 1), (0, 2), ... and the sums k Q1 (so
    they stay below 2^32 even at m = 300; weighted_ties is where sums pass 32 bits)"""
    return _sym(m, lambda i, j: Q1)


def two_valued(m, fam=7, q=5000):
    """families of `fam` consecutive-by-stride indices at one small q, Q1 across families: what real data looks like"""
    nf = (m + fam - 1) // fam
    return _sym(m, lambda i, j: q if i % nf == j % nf else Q1)


def chain(m):
    """q falls with i + j: the least pair is always the two highest live indices (a, b), and every row below them held b as its
    best partner -- every merge changes the best partner of every other row"""
    return _sym(m, lambda i, j: Q1 // 2 - 100 * (i + j))


def tie_after_merge():
    """The tie a row cache has to get right.  (2, 3) merge first, at 10.  Row 0 is at 500 from 2, from 3 and from 4, so the new
    D(0, 2 + 3) = 1000 / 2 equals D(0, 4) exactly and the tie rule wants (0, 2) next, not (0, 4); row 1 is at 500 from 5 only, so
    (0, 2) must also come before (1, 5).  (With an exact cache row 0's partner before the merge is 2, the lowest of its equals --
    a new D(a, c) is a weighted mean of two values that are both at least the row's best, so it can equal that best only when
    both do, and then the row already holds a or something lower: the hazard is a row that looks at a, b and a higher index at
    one value and has to come out of its rescan with a.)"""
    m = 6
    S = _sym(m, lambda i, j: 900)
    def put(i, j, v):
        S[i][j] = S[j][i] = v
    put(2, 3, 10)
    for y in (2, 3, 4):
        put(0, y, 500)
    put(1, 5, 500)
    return S


def wide():
    """m = 6, sizes 3 000 each: S(0, 1) = 2^58 + x and S(2, 3) = x under the same n_a n_b = 9 000 000 = 2^6 * 140 625, so the two
    cross products differ by 140 625 * 2^64: equal in their low 64 bits, different above.  (2, 3) is the true first merge; a
    64-bit comparison sees a tie and takes (0, 1).  Sums of real distances stop at Q1 n_a n_b < 2^44, where the low 64 bits of two
    different cross products cannot agree (that needs a difference of 2^58 between sums); rtc_upgma_dev takes any sums while
    everything it forms stays below 2^62, which is the case here.  The other pairs are in range, and their cross products -- up
    to 9.4e12 * 3.6e7 -- pass 64 bits too."""
    m = 6
    x = 5_000_000_000_000
    S = _sym(m, lambda i, j: 6_000_000_000_000 + 200_000_000_000 * (i + 2 * j))
    S[0][1] = S[1][0] = (1 << 58) + x
    S[2][3] = S[3][2] = x
    return S, [3000] * m


def weighted_ties(m, seed=6):
    """clusters of 1 000 to 3 000 members each, S = q w_i w_j with q from five values: sums far past 32 bits from the start, and
    equal means under different sizes at every step"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1000, 3001, size=m).tolist()
    v = rng.integers(1, 6, size=(m, m)) * (Q1 // 8)
    return _sym(m, lambda i, j: int(v[i, j]) * w[i] * w[j]), w


def dev_sets():
    """every set rtc_upgma_dev is checked on"""
    out = [("random_ties_%d" % m, random_ties(m), None) for m in SIZES]
    out += [("all_q1_65", all_q1(65), None), ("all_q1_300", all_q1(300), None)]
    out += [("two_valued_66", two_valued(66), None), ("two_valued_130", two_valued(130), None)]
    out += [("chain_70", chain(70), None)]
    out += [("tie_after_merge", tie_after_merge(), None)]
    Sw, ww = wide()
    out += [("wide", Sw, ww)]
    Sb, wb = weighted_ties(66)
    out += [("weighted_ties_66", Sb, wb)]
    rng = np.random.default_rng(9)
    out += [("weighted_67", random_ties(67, seed=4), rng.integers(1, 50, size=67).tolist())]
    return out
