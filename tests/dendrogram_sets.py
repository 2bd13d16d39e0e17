"""The inputs of tests/test_gpu_dendrogram_turns.py and tests/test_cpu_dendrogram_sets.py: matrices whose winning pair sits where
only a later turn of a dendrogram kernel's loop finds it -- a row past the first 1 024 of the workgroup linkage kernel, a scan
workgroup past the first 256 minima of the grid paths' reduce, a row that a scan workgroup reaches only on its second pass.
Random matrices mostly win in row 0; these win at the far end of the active list."""
import functools

import numpy as np

# the sizes of the tests, and the loop that turns there
REDUCE_M = 1030     # r >= 1026: more than 256 scan minima (n_minima = min((r + 2) / 4, 1024)), the reduce's second turn
CHAIN_M = 1300      # 275 steps of top_chain at r >= 1026
CAP_UPGMA_M = 4104  # r > 4097: more rows than 4 * 1 024, a scan workgroup's second row; seven steps of top_chain
CAP_NJ_M = 4102     # the same for neighbour joining; five joins of top_group
GROUP = 6
# Complete linkage: (linkage_sets case, m, seed or None, bounded too).  1 030 is past 1 024, the second turn of lk_wg_kernel's
# steps 1 and 2; 1 300 is past 1 280, that turn's slots 1 and up.  Step 1 sees a pair (a, b) from row a, so only a merge with
# a >= 1024 needs its second turn.  Among six rows that is rare: at 1 030 the seeds are the first found whose dendrogram has one
# (tie_free: 1026 and 1028 are each other's nearest; random_ties: (1025, 1027) at kappa 1); at 1 300 the sets' own seeds have
# 26, 129 and 39, and random_ties one with a = 1280, slot 1.  star merges into 0 throughout: it is there for its rescans, every
# live row at every step, and for step 2.
LINKAGE_CASES = (("tie_free", 1030, 104, False), ("random_ties", 1030, 2, True), ("tie_free", 1300, None, False),
                 ("random_ties", 1300, None, True), ("near_2_31", 1300, None, False), ("star", 1300, None, False))


def linkage_keys(name, m, seed):
    from tests import linkage_sets as S
    return S.CASES[name](m) if seed is None else S.CASES[name](m, seed=seed)


def top_chain(m):
    """S[i][j] = 8 (m - min(i, j)) as uint64, sizes all 1.  Every pair of row k has mean exactly 8 (m - k) at every step -- a merge
    (a, b) adds two cells of equal mean -- so the one least pair is always the last row of the active list: see
    top_chain_records."""
    lo = np.minimum.outer(np.arange(m), np.arange(m))
    S = (8 * (m - lo)).astype(np.uint64)
    np.fill_diagonal(S, 0)
    return S


def top_chain_records(m):
    """the whole dendrogram of top_chain(m): step t joins m - 2 - t and the cluster of t + 1 points that m - 1 - t has become, over
    (t + 1) pairs of 8 (t + 2) each"""
    return [(m - 2 - t, m - 1 - t, 1, t + 1, (t + 1) * 8 * (t + 2)) for t in range(m - 1)]


@functools.lru_cache(maxsize=None)
def top_group(m, g=GROUP, seed=3):
    """A symmetric matrix of eighths in [0.5, 1]; the last g points see every other point k at far[k] + 0.25 (far drawn the same
    way) and each other at (1 + |x - y|) / 64.  The group is tight and far from everything, so the first g - 1 joins are inside it
    -- at list positions m - g and up.  Every entry is a multiple of 1 / 64 below 2: the initial R (sums below 2^14 on a grid of
    2^-6) and everything the first joins form is exact in any order of evaluation."""
    assert m > 2 * g
    rng = np.random.default_rng(seed)
    up = np.triu(rng.integers(4, 9, size=(m, m)) / 8.0, 1)
    D = up + up.T
    far = rng.integers(4, 9, size=m) / 8.0
    lo = m - g
    D[lo:, :lo] = far[None, :lo] + 0.25
    D[:lo, lo:] = D[lo:, :lo].T
    x = np.arange(g)
    D[lo:, lo:] = (1 + np.abs(x[:, None] - x[None, :])) / 64.0
    np.fill_diagonal(D, 0.0)
    assert np.array_equal(D, D.T)
    return np.ascontiguousarray(D)


def on_grid_64(D):
    """every entry times 64 is an integer below 128: what makes top_group's sums exact"""
    s = np.asarray(D) * 64.0
    return bool(np.all(s == np.floor(s)) and np.all(s >= 0) and np.all(s < 128))
