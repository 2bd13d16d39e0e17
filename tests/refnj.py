"""Neighbour joining restated (include/rtclust.h holds the definition): Saitou-Nei with Studier-Keppler's Q over a symmetric
matrix of doubles, every operation one IEEE-754 double operation in the written order.  numpy's elementwise expressions do
exactly the scalar operations, one after the other and without fusing them, so the vectorised steps are bit-identical to the
scalar text; the one ordered sum -- the initial R -- is a Python loop."""
import numpy as np

NONE = 0xFFFFFFFF


def nj(dist, steps=None, exact_sums=False):
    """[(a, b, c, len_a, len_b, len_c)] in step order; c is NONE but in the last record of m >= 3.  steps: stop after that many
    joins (the records are the first `steps` of the whole run's).  exact_sums: the caller vouches that every sum of a row's
    entries is exact in any order (entries on a coarse binary grid), so the initial R may be numpy's row sums."""
    D = np.array(dist, dtype=np.float64, copy=True)
    m = int(D.shape[0])
    assert D.ndim == 2 and D.shape[1] == m
    if m <= 1:
        return []
    if m == 2:
        d = D[0, 1]
        la = np.float64(0.5) * d
        return [(0, 1, NONE, float(la), float(d - la), 0.0)]
    R = np.zeros(m, dtype=np.float64)
    if exact_sums:
        off = D.copy()
        np.fill_diagonal(off, 0.0)
        R[:] = off.sum(axis=1)
    else:
        for i in range(m):
            s = np.float64(0.0)
            row = D[i]
            for j in range(m):
                if j != i:
                    s = s + row[j]
            R[i] = s
    act = np.arange(m)
    r = m
    out = []
    half = np.float64(0.5)
    while r > 3:
        if steps is not None and len(out) >= steps:
            return out
        sub = D[np.ix_(act, act)]
        ra = R[act]
        Q = (np.float64(r - 2) * sub - ra[:, None]) - ra[None, :]  # Q[p, q], p < q: ((r - 2) D[i][j] - R[i]) - R[j]
        Q[np.tril_indices(r)] = np.inf
        p, q = divmod(int(np.argmin(Q)), r)  # the first of equal values in row-major order: smallest i, then smallest j
        i, j = int(act[p]), int(act[q])
        dij = D[i, j]
        delta = (R[i] - R[j]) / np.float64(2 * (r - 2))
        len_i = half * dij + delta
        len_j = dij - len_i
        ks = np.delete(act, [p, q])
        dik, djk = D[i, ks].copy(), D[j, ks].copy()
        duk = half * ((dik + djk) - dij)
        R[ks] = ((R[ks] - dik) - djk) + duk
        D[i, ks] = duk
        D[ks, i] = duk
        R[i] = half * ((R[i] + R[j]) - np.float64(r) * dij)
        out.append((i, j, NONE, float(len_i), float(len_j), 0.0))
        act = np.delete(act, q)
        r -= 1
    if steps is not None and len(out) >= steps:
        return out
    i, j, k = (int(v) for v in act)
    out.append((i, j, k, float(half * ((D[i, j] + D[i, k]) - D[j, k])), float(half * ((D[i, j] + D[j, k]) - D[i, k])),
                float(half * ((D[i, k] + D[j, k]) - D[i, j]))))
    return out


def bits(records):
    """the records with their lengths as 64-bit patterns: equality is equality on bits (-0.0 is not 0.0)"""
    return [(int(a), int(b), int(c)) + tuple(int(np.float64(x).view(np.uint64)) for x in (la, lb, lc)) for a, b, c, la, lb, lc in records]


def splits(records, m):
    """the tree of the records as a sorted list of (split, length): a split is the leaf set on the side of a branch away from
    leaf 0, as a bit mask.  Two leaves: their one branch, len_a + len_b."""
    if m == 2:
        (_, _, _, la, lb, _), = records
        return [(2, la + lb)]
    full = (1 << m) - 1
    under = {x: 1 << x for x in range(m)}
    out = []
    for a, b, c, la, lb, lc in records:
        ends = [(a, la), (b, lb)] + ([(c, lc)] if c != NONE else [])
        for x, ln in ends:
            out.append((full ^ under[x] if under[x] & 1 else under[x], ln))
        for x, _ in ends[1:]:
            under[a] |= under.pop(x)
    return sorted(out)
