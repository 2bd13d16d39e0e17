"""The density hierarchy of clust-dbscan --hierarchy (rtc_dbscan_hierarchy, rtc_hierarchy_cut, rtc_hierarchy_flat) restated in
plain Python, beside tests/refdbscan.py (the reference's predicate, which decides the kept pairs) and tests/refkdist.py (the
core triples).  Candidates by brute force, j as fractions.Fraction, Kruskal under the total order (larger m first, then smaller
p, then smaller q), the cut with the predicate in double, the condensed tree and its selection by excess of mass as
include/rtclust.h defines them."""
import math
from fractions import Fraction

from tests import refdbscan as R
from tests import refkdist as KD

NONE = KD.NONE
MIN_DIST = 1e-12


def kept_pairs(sketches, eps_max, kmer_size, use64, max_posting=0):
    """{(p, q): common} with p < q: the pairs the reference's neighbour test accepts at eps_max, in both orientations"""
    nb = R.neighbour_lists(sketches, eps_max, kmer_size, use64, max_posting)
    cand = KD.candidates(sketches, use64, max_posting)
    sets = [set(x) for x in nb]
    out = {}
    for p, lst in enumerate(nb):
        for q in lst:
            assert p in sets[q], ("the relation is not symmetric", p, q)
            if p < q:
                out[(p, q)] = cand[p][q]
    return out


def jac(t):
    return KD.jaccard(t[0], t[1], t[2])


def hierarchy(sketches, eps_max, min_pts, kmer_size, use64, max_posting=0):
    """(forest, core): forest a list of (p, q, common, size_p, size_q) in the total order, core as refkdist.kdist gives it"""
    core = KD.kdist(sketches, min_pts, use64, max_posting)
    sizes = [len(s) for s in sketches]
    edges = []
    for (p, q), c in kept_pairs(sketches, eps_max, kmer_size, use64, max_posting).items():
        if core[p][3] == NONE or core[q][3] == NONE:
            continue
        lim = (c, sizes[p], sizes[q])
        for t in (core[p][:3], core[q][:3]):  # the pair's own triple unless a core level is strictly below it
            if jac(t) < jac(lim):
                lim = tuple(t)
        edges.append((-jac(lim), p, q, lim))
    edges.sort(key=lambda e: e[:3])
    parent = list(range(len(sketches)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    forest = []
    for _, p, q, lim in edges:
        a, b = find(p), find(q)
        if a != b:
            parent[a] = b
            forest.append((p, q) + lim)
    return forest, core


def pred(a, b, common, t):
    """findNeighborsKSSDWithIndex's test for reference size a and candidate size b, as tests/refdbscan.py restates it"""
    if a == 0 or b == 0:
        return False
    if b < math.floor(t * float(a)) or b > math.ceil(float(a) / t):
        return False
    return not (float(common) * (1.0 + t) + 1e-12 < t * float(a) + t * float(b))


def passes(common, a, b, t):
    return (a == 0 and b == 0) or (pred(a, b, common, t) and pred(b, a, common, t))


def cut(n, forest, core, eps, kmer_size):
    """(labels, core flags): DBSCAN* at eps, clusters numbered by smallest core index, non-core points -1"""
    t = R.jaccard_min(eps, kmer_size)
    is_core = [c[3] != NONE and passes(c[0], c[1], c[2], t) for c in core]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for p, q, c, a, b in forest:
        if is_core[p] and is_core[q] and passes(c, a, b, t):
            ra, rb = find(p), find(q)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    ids, labels = {}, []
    for v in range(n):
        if not is_core[v]:
            labels.append(-1)
            continue
        labels.append(ids.setdefault(find(v), len(ids)))
    return labels, is_core


def min_margin(forest, core, eps_list, kmer_size):
    """the smallest |j - t(eps)| over the forest's and the core triples and the eps values: the cut's exact order and its
    double predicate agree while this stays far above rounding"""
    js = {jac(e[2:]) for e in forest} | {jac(c) for c in core if c[3] != NONE}
    return min((abs(float(j) - R.jaccard_min(eps, kmer_size)) for j in js for eps in eps_list), default=1.0)


def distance(common, a, b, kmer_size):
    return KD.distance(common, a, b, kmer_size)


def flat(n, forest, core, kmer_size, min_cluster_size):
    """(labels, stabilities by label, the smallest relative gap between a cluster's stability and its children's sum)"""
    # the dendrogram, forest order: node = ('leaf', v) or index of the merge
    comp = {v: [v] for v in range(n) if core[v][3] != NONE}   # root point -> members
    where = {v: v for v in comp}                              # point -> root point
    top = {v: ("leaf", v) for v in comp}
    merges = []
    for p, q, c, a, b in forest:
        rp, rq = where[p], where[q]
        assert rp != rq
        lam = 1.0 / max(distance(c, a, b, kmer_size), MIN_DIST)
        merges.append((top[rp], top[rq], lam))
        for v in comp[rq]:
            where[v] = rp
        comp[rp] += comp.pop(rq)
        top[rp] = ("merge", len(merges) - 1)

    def members(node):
        out, stack = [], [node]
        while stack:
            kind, x = stack.pop()
            if kind == "leaf":
                out.append(x)
            else:
                stack += [merges[x][0], merges[x][1]]
        return out

    clusters = []  # dicts: parent, children, birth, terms {merge index: value}, points (fallen out of it)

    def new(parent, birth):
        clusters.append({"parent": parent, "children": None, "birth": birth, "terms": {}, "points": []})
        return len(clusters) - 1
    tops = [root for root in sorted(comp) if len(comp[root]) >= min_cluster_size]
    work = [(top[root], new(None, 0.0)) for root in tops]
    while work:
        node, c = work.pop()
        while True:
            if node[0] == "leaf":  # cannot happen for min_cluster_size >= 2: a live node holds that many points
                clusters[c]["points"].append(node[1])
                break
            left, right, lam = merges[node[1]]
            ml, mr = members(left), members(right)
            big_l, big_r = len(ml) >= min_cluster_size, len(mr) >= min_cluster_size
            if big_l and big_r:
                clusters[c]["terms"][node[1]] = float(len(ml) + len(mr)) * (lam - clusters[c]["birth"])
                cl, cr = new(c, lam), new(c, lam)
                clusters[c]["children"] = (cl, cr)
                work += [(left, cl), (right, cr)]
                break
            leaving = (0 if big_l else len(ml)) + (0 if big_r else len(mr))
            clusters[c]["terms"][node[1]] = float(leaving) * (lam - clusters[c]["birth"])
            if not big_l:
                clusters[c]["points"] += ml
            if not big_r:
                clusters[c]["points"] += mr
            if not big_l and not big_r:
                break
            node = left if big_l else right
    for cl in clusters:
        s = 0.0
        for e in sorted(cl["terms"]):  # forest order
            s += cl["terms"][e]
        cl["stab"] = s
    gap = math.inf

    def best(c):
        nonlocal gap
        cl = clusters[c]
        if cl["children"] is None:
            cl["selected"] = True
            return cl["stab"]
        below = best(cl["children"][0]) + best(cl["children"][1])
        gap = min(gap, abs(cl["stab"] - below) / max(abs(cl["stab"]), abs(below), 1e-300))
        root = cl["parent"] is None and len(tops) == 1
        cl["selected"] = (not root) and cl["stab"] > below
        return cl["stab"] if cl["selected"] else below
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    for c, cl in enumerate(clusters):
        if cl["parent"] is None:
            best(c)
    labels = [-1] * n
    shown = {}
    for c, cl in enumerate(clusters):  # parents come before their children
        up = shown.get(cl["parent"])
        shown[c] = up if up is not None else (c if cl["selected"] else None)
    owner = {}
    for c, cl in enumerate(clusters):
        for v in cl["points"]:
            owner[v] = shown[c]
    number, stabs = {}, []
    for v in range(n):
        c = owner.get(v)
        if c is None:
            continue
        if c not in number:
            number[c] = len(number)
            stabs.append(clusters[c]["stab"])
        labels[v] = number[c]
    return labels, stabs, gap


def nested_sets(seed, use64):
    """Sketch sets with a hierarchy worth selecting from: two super-families whose sub-families (three and two, five members
    each at substitution rate 0.03) derive from one root at rate 0.2, and two loners, in shuffled order.  The sub-families
    merge well below eps 0.12, so the condensed tree has true splits and excess of mass has something to compare."""
    import numpy as np
    rng = np.random.default_rng(1000 + seed)
    dt = np.uint64 if use64 else np.uint32

    def fresh(m):
        return rng.integers(1, (1 << 31) - 1, size=m, dtype=np.int64)

    def mutate(b, rate):
        s = b.copy()
        flip = rng.random(len(b)) < rate
        s[flip] = fresh(int(flip.sum()))
        return s
    out = []
    for size, subs in ((300, 3), (260, 2)):
        root = fresh(size)
        for _ in range(subs):
            sub = mutate(root, 0.2)
            out += [mutate(sub, 0.03) for _ in range(5)]
    out += [fresh(200), fresh(120)]
    out = [out[i] for i in rng.permutation(len(out))]
    return [np.unique(s).astype(dt) for s in out]
