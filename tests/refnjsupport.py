"""Jackknife support of the neighbour-joining trees restated (include/rtclust.h holds the definition, under rtc_nj_support).
Everything here is Python integers and sets but the neighbour joining itself, which is tests/refnj.py's, and the distance of a
key, which is tests/reflinkage.py's.  Splits are compared as frozensets of leaves."""
import numpy as np

from tests import reflinkage as RL
from tests import refnj as R

M64 = (1 << 64) - 1
NONE = R.NONE


def mix(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def word(h, seed, w):
    return mix(int(h) ^ mix((int(seed) + int(w)) & M64))


def kept(h, seed, r):
    """does replicate r keep hash h"""
    return (word(h, seed, r // 64) >> (r % 64)) & 1 == 1


def replicate_sets(sketches, seed, r):
    """the sketches of replicate r as sets"""
    keep = {}
    out = []
    for s in sketches:
        cur = set()
        for h in s:
            h = int(h)
            if h not in keep:
                keep[h] = kept(h, seed, r)
            if keep[h]:
                cur.add(h)
        out.append(cur)
    return out


def distances(sets, kmer_size):
    """D[a][b] over a list of hash sets: the distance of the key (common, |a| + |b| - common), 1 for common == 0 or denom == 0"""
    m = len(sets)
    D = np.zeros((m, m), dtype=np.float64)
    for i in range(m):
        for j in range(i):
            common = len(sets[i] & sets[j])
            denom = len(sets[i]) + len(sets[j]) - common
            D[i, j] = D[j, i] = 1.0 if common == 0 or denom == 0 else RL.distance(common, denom, kmer_size)
    return D


def record_splits(records, m):
    """one entry per record: None where it names no split, else the split as the frozenset of local leaves on the side that does
    not hold leaf 0 (the component's smallest member: members ascend).  m <= 3: all None."""
    if m < 4:
        return [None] * len(records)
    everyone = frozenset(range(m))
    under = {x: frozenset([x]) for x in range(m)}
    out = []
    for a, b, c, *_ in records:
        if c != NONE:
            out.append(None)
            continue
        s = under[a] | under.pop(b)
        under[a] = s
        out.append(everyone - s if 0 in s else s)
    return out


def support_of(sketches, kmer_size, replicates, seed):
    """(records of the main tree with local indices, support per record) for one component, sketches in member order"""
    m = len(sketches)
    main = R.nj(distances([set(int(h) for h in s) for s in sketches], kmer_size))
    main_splits = record_splits(main, m)
    support = [0] * len(main)
    if m >= 4:
        for r in range(replicates):
            rep = R.nj(distances(replicate_sets(sketches, seed, r), kmer_size))
            have = set(s for s in record_splits(rep, m) if s is not None)
            for e, s in enumerate(main_splits):
                if s is not None and s in have:
                    support[e] += 1
    return main, support


def clusters(sketches, comp, kmer_size, replicates, seed):
    """rtc_nj_support: (records with genome indices, first, support) over the components of the labelling, in order of their
    smallest member"""
    groups = {}
    for g, lab in enumerate(comp):
        groups.setdefault(int(lab), []).append(g)
    records, first, support = [], [0], []
    for members in sorted(groups.values()):
        if len(members) >= 2:
            main, sup = support_of([sketches[g] for g in members], kmer_size, replicates, seed)
            records += [(members[a], members[b], members[c] if c != NONE else c, la, lb, lc) for a, b, c, la, lb, lc in main]
            support += sup
        first.append(len(records))
    return records, first, support


def label(count, replicates):
    """the percentage a support file prints: half up, in integers"""
    return (200 * count + replicates) // (2 * replicates)
