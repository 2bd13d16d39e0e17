"""Jackknife support of the clusters restated (include/rtclust.h holds the definition, under rtc_cluster_support).  Everything here
is Python integers, sets and a union-find; the mask is tests/refnjsupport.py's, the distance of a key tests/reflinkage.py's, and it
is evaluated per pair and replicate, never through a table."""
import math

from tests import reflinkage as RL
from tests import refnjsupport as RS


def radio(threshold, kmer_size):
    """the size-ratio bound of the MST's candidates: floor(2 e^(threshold (k - 1)) - 1), saturated"""
    r = 2.0 * math.exp(threshold * (kmer_size - 1)) - 1.0
    return int(r) if r < 2147483647.0 else 2147483647


def candidates(sketches, threshold, kmer_size):
    """the pairs (i, j), j < i, that share a hash and pass the size-ratio rule on the full sketches"""
    rad = radio(threshold, kmer_size)
    owners = {}
    for g, s in enumerate(sketches):
        for h in s:
            owners.setdefault(int(h), []).append(g)
    pairs = set()
    for gs in owners.values():
        for x in range(len(gs)):
            for y in range(x):
                pairs.add((gs[x], gs[y]))
    out = []
    for i, j in sorted(pairs):
        a, b = len(sketches[i]), len(sketches[j])
        if max(a, b) <= rad * min(a, b):
            out.append((i, j))
    return out


def is_edge(common, denom, kmer_size, threshold):
    return common > 0 and RL.distance(common, denom, kmer_size) <= threshold


class _Words:
    """the mask words of every hash of a set, one word index at a time"""

    def __init__(self, sketches, seed):
        self.hashes = sorted({int(h) for s in sketches for h in s})
        self.seed = seed
        self.words = {}

    def kept(self, r):
        w = r // 64
        if w not in self.words:
            self.words[w] = {h: RS.word(h, self.seed, w) for h in self.hashes}
        bit = r % 64
        return {h for h, x in self.words[w].items() if (x >> bit) & 1}


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _union(parent, a, b):
    ra, rb = _find(parent, a), _find(parent, b)
    if ra != rb:
        parent[max(ra, rb)] = min(ra, rb)  # the root is the smallest member


def cluster_order(comp):
    """(cluster of every genome, members of every cluster): clusters numbered by their smallest member, members ascending"""
    number, members = {}, []
    cl = []
    for g, lab in enumerate(comp):
        lab = int(lab)
        if lab not in number:
            number[lab] = len(members)
            members.append([])
        cl.append(number[lab])
        members[number[lab]].append(g)
    return cl, members


def replicate(sets, cand, cl, members, kmer_size, threshold):
    """one replicate over the given hash sets: ([(whole, pure, pieces) per cluster], [piece - 1 per genome])"""
    n = len(sets)
    parent = list(range(n))
    touched = set()
    for i, j in cand:
        common = len(sets[i] & sets[j])
        denom = len(sets[i]) + len(sets[j]) - common
        if not is_edge(common, denom, kmer_size, threshold):
            continue
        if cl[i] == cl[j]:
            _union(parent, i, j)
        else:
            touched.add(cl[i])
            touched.add(cl[j])
    P = [_find(parent, g) for g in range(n)]
    piece = {}
    for p in P:
        piece[p] = piece.get(p, 0) + 1
    per_cluster = []
    for c, mem in enumerate(members):
        whole = all(P[g] == mem[0] for g in mem)
        pieces = sum(1 for g in mem if P[g] == g)
        per_cluster.append((whole, c not in touched, pieces))
    return per_cluster, [piece[P[g]] - 1 for g in range(n)]


def outcomes(sketches, comp, kmer_size, threshold, replicates, seed, keep_all=False):
    """the replicates 0 .. replicates - 1, each as replicate() returns it; keep_all: every hash kept in every replicate"""
    full = [set(int(h) for h in s) for s in sketches]
    cand = candidates(sketches, threshold, kmer_size)
    cl, members = cluster_order(comp)
    words = _Words(sketches, seed)
    out = []
    for r in range(replicates):
        if keep_all:
            sets = full
        else:
            kept = words.kept(r)
            sets = [s & kept for s in full]
        out.append(replicate(sets, cand, cl, members, kmer_size, threshold))
    return out, members


def tally(outs, members, replicates):
    """rtc_cluster_support's output from the first `replicates` outcomes: ([(size, recovered, split, merged, mixed, max_pieces)],
    [together])"""
    rec = [[len(m), 0, 0, 0, 0, 0] for m in members]
    together = [0] * sum(len(m) for m in members)
    for per_cluster, minus in outs[:replicates]:
        for c, (whole, pure, pieces) in enumerate(per_cluster):
            rec[c][1 + (0 if whole and pure else 1 if pure else 2 if whole else 3)] += 1
            rec[c][5] = max(rec[c][5], pieces)
        for g, x in enumerate(minus):
            together[g] += x
    return [tuple(r) for r in rec], together


def support(sketches, comp, kmer_size, threshold, replicates, seed, keep_all=False):
    outs, members = outcomes(sketches, comp, kmer_size, threshold, replicates, seed, keep_all)
    return tally(outs, members, replicates)


def mst_partition(sketches, kmer_size, threshold):
    """the labels of single linkage at the threshold over the candidates: the MST's own partition, every genome labelled by the
    smallest member of its cluster"""
    full = [set(int(h) for h in s) for s in sketches]
    parent = list(range(len(sketches)))
    for i, j in candidates(sketches, threshold, kmer_size):
        common = len(full[i] & full[j])
        if is_edge(common, len(full[i]) + len(full[j]) - common, kmer_size, threshold):
            _union(parent, i, j)
    return [_find(parent, g) for g in range(len(sketches))]


def need(d, kmer_size, threshold):
    """the keep table's entry by direct evaluation: the least c in 1 .. d whose distance is at most the threshold, d + 1 if none"""
    for c in range(1, d + 1):
        if RL.distance(c, d, kmer_size) <= threshold:
            return c
    return d + 1


def label(count, replicates):
    """the percentage the support file prints: half up, in integers"""
    return (200 * count + replicates) // (2 * replicates)
