"""The sketch set of tests/test_gpu_graph_mash.py and its restated graph, built once per sketch size and shared by both widths
(the u64 lists are the u32 values plus 2^40: the order, and with it every count, is the same).

193 ascending lists (not a multiple of 64) of at most s hashes.  Every non-empty one ends in one hash above all others, so
every pair of non-empty lists is a candidate, and for two long unrelated lists that hash lies beyond the truncation:
  - a family of 80 close members of 241 hashes with exact copies among them: one node with more than 70 passing
    higher-numbered neighbours, equal ranks among them, unions below s (denom < s);
  - looser families on both sides of the threshold, twelve members of them s hashes long (past the 1 024-element LDS staging
    at s = 1200): their unions are cut at s;
  - whole / part: 200 and 99 hashes, the short one a subset -- an edge here, where the KSSD graph's size-ratio rule would skip it;
  - P = {p, top}, R = {top}, Q = {p, q1, q2, top}: P meets R at 1/2 and Q at 2/4; P comes first of the three, so with knn_k = 1
    the cross-multiplied tie decides which one it keeps.  R and P are the lists of 1 and 2 hashes;
  - three unrelated lists of s hashes: their only shared hash is the top one, past the first s of the union;
  - unrelated lists of other sizes, and two empty ones."""
import numpy as np

from tests import refgraph_mash

KMER = 21
THRESHOLD = 0.05  # an edge needs common / denom above ~0.212
TOP = (1 << 31) - 2
KNN = (0, 1, 3, 70)

_CACHE = {}


def _lists(s):
    rng = np.random.default_rng(4100 + s)

    def fresh(m):
        return rng.integers(1000, TOP - 1000, size=m, dtype=np.int64)

    def members(count, size, rate):
        base = fresh(size)
        out = []
        for _ in range(count):
            x = base.copy()
            flip = rng.random(size) < rate
            x[flip] = fresh(int(flip.sum()))
            out.append(x)
        return out
    big = members(74, 240, 0.04)
    big += [big[3].copy(), big[3].copy(), big[10].copy(), big[10].copy(), big[11].copy(), big[40].copy()]
    out = big + members(12, s - 1, 0.2) + members(18, 200, 0.2) + members(30, 200, 0.45) + members(20, 150, 0.7)
    whole = np.unique(fresh(199))
    out += [whole, whole[:98]]  # with the top hash: 200 and 99 hashes
    out += [fresh(s - 1) for _ in range(3)]
    out += [fresh(int(rng.integers(100, 250))) for _ in range(193 - 2 - 3 - len(out))]
    out = [np.unique(np.append(x, TOP)) for x in out]
    p = fresh(3)
    trio = [np.array([p[0], TOP]), np.array([TOP]), np.unique(np.array([p[0], p[1], p[2], TOP]))]  # P, R, Q
    out += [np.zeros(0, dtype=np.int64)] * 2
    order = rng.permutation(193 - 3).tolist()
    out = [out[i] for i in order]
    at = sorted(rng.choice(193, size=3, replace=False).tolist())  # P takes the first of the three places
    for place, x in zip(at, trio):
        out.insert(place, x)
    assert len(out) == 193 and all(len(x) <= s and np.all(np.diff(x) > 0) for x in out)
    return out, tuple(at)


def case(s):
    """(lists, (P, R, Q), counts, {knn_k: edges}) for sketch size s"""
    if s not in _CACHE:
        lists, trio = _lists(s)
        counts = refgraph_mash.counts(lists, s)
        _CACHE[s] = (lists, trio, counts, {k: refgraph_mash.edges(counts, THRESHOLD, KMER, k) for k in KNN})
    return _CACHE[s]


def typed(lists, width):
    if width == 4:
        return [x.astype(np.uint32) for x in lists]
    return [x.astype(np.uint64) + np.uint64(1 << 40) for x in lists]
