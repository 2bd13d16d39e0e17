"""Sketch sets for the eps sweep tests: families at three substitution rates, a chain of sliding windows, loners and
(optionally) empty sketches, in shuffled order.  With k-mer size 21 the pairwise distances -ln(2 j / (1 + j)) / 21 sit near
0.003 (rate 0.03, j ~ 0.89), 0.016 (rate 0.15, j ~ 0.57) and 0.041 (rate 0.35, j ~ 0.27); the chain's windows of 100 hashes
in steps of 25 are 0.014 / 0.033 / 0.066 apart at one / two / three steps.  EPS lies between and beyond these, so the levels
cut the set in different ways; at eps 0.04 and minPts 5 the chain's interior is core (four neighbours) and its ends are
border points."""
import numpy as np

KMER = 21
EPS = [0.002, 0.008, 0.02, 0.04, 0.06, 0.12]
FAMILIES = [(7, 0.03, 260), (6, 0.15, 230), (6, 0.35, 300), (3, 0.03, 200)]  # members, substitution rate, hashes


def family_sets(seed, use64, n_empty=0, shuffle=True):
    rng = np.random.default_rng(seed)
    dt = np.uint64 if use64 else np.uint32

    def fresh(m):
        return rng.integers(1, (1 << 31) - 1, size=m, dtype=np.int64)
    out = []
    for members, rate, size in FAMILIES:
        base = fresh(size)
        for _ in range(members):
            s = base.copy()
            flip = rng.random(size) < rate
            s[flip] = fresh(int(flip.sum()))
            out.append(s)
    chain0 = int(rng.integers(1 << 20, 1 << 30))
    for i in range(8):
        out.append(np.arange(chain0 + 25 * i, chain0 + 25 * i + 100, dtype=np.int64))
    out += [fresh(150), fresh(90)]
    out += [np.zeros(0, dtype=np.int64)] * n_empty
    if shuffle:
        out = [out[i] for i in rng.permutation(len(out))]
    return [np.unique(s).astype(dt) for s in out]


def describe(labels_by_eps, cores_by_eps):
    """(distinct label vectors, some level has noise, some level has a border point) of a sweep's expected result"""
    distinct = len({tuple(int(x) for x in lab) for lab in labels_by_eps})
    noise = any((np.asarray(lab) < 0).any() for lab in labels_by_eps)
    border = any(((np.asarray(lab) >= 0) & ~np.asarray(core, dtype=bool)).any() for lab, core in zip(labels_by_eps, cores_by_eps))
    return distinct, noise, border
