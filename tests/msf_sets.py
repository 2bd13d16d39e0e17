"""Graphs for the Boruvka forest kernels (rtc_mst.hip, rtc_sort.hip), handed to them as edge lists without a single sketch:
tests/test_cpu_msf_sets.py proves on the reference (tests/refmsf.py) that each holds what it is for, tests/test_gpu_msf_edges.py
runs them on the GPU.  Every case is (n, edges int32 [m, 3] of (i, j, common) with i > j, lens uint32 [n], wmode), built from a
seed; every pair occurs once, common <= min(len_i, len_j), and in mode 2 | s << 2 common <= s as well.  The list is shuffled
unless the case is about its order.  A case name ending in _var is the same graph with sizes that vary (the weight / edge-id
passes), without it all sizes are equal (the fused key).

One turn of the edge kernels is num_cu * 8 workgroups of 256 lanes (grid_for): 524 288 list entries with 256 compute units."""
import os

import numpy as np

SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))

_CACHE = {}


def turn(num_cu):
    return num_cu * 8 * 256


def _pack(n, i, j, c, lens, wmode, rng=None):
    i, j, c = (np.asarray(a, dtype=np.int64) for a in (i, j, c))
    e = np.stack([np.maximum(i, j), np.minimum(i, j), c], axis=1).astype(np.int32).reshape(-1, 3)
    if rng is not None and len(e):
        e = e[rng.permutation(len(e))]
    return n, np.ascontiguousarray(e), np.ascontiguousarray(np.asarray(lens, dtype=np.uint32)), wmode


def _distinct_pairs(rng, n, m):
    """about m distinct pairs a > b of [0, n)"""
    a = rng.integers(0, n, size=m + m // 8 + 8)
    b = rng.integers(0, n, size=len(a))
    keep = a != b
    hi, lo = np.maximum(a, b)[keep], np.minimum(a, b)[keep]
    u = np.unique(hi * np.int64(n) + lo)
    u = u[rng.permutation(len(u))][:m]
    return u // n, u % n


# ---- chain: one successor chain for relabel to walk -------------------------------------------------------------------------
CHAIN = 20_000


def chain(var=False):
    """A path whose similarity rises strictly along the index: in round one vertex v hooks onto v + 1, the last two pick each
    other and the smaller one, CHAIN - 2, stays the root.  CHAIN - 1 hooks in one tree, the walk from vertex 0 has CHAIN - 2
    links.  Two rounds."""
    rng = np.random.default_rng(2101)
    v = np.arange(CHAIN - 1)
    lens = np.full(CHAIN, 2 * CHAIN, dtype=np.uint32)
    if var:
        lens[0] += 1  # edge (1, 0) stays the least similar one
    return _pack(CHAIN, v + 1, v, v + 1, lens, 0, rng)


# ---- ruler: components double per round -------------------------------------------------------------------------------------
RULER = 4097
RULER_SMALL = (3, 5, 9, 17)  # the round that finds nothing is round 1, 2, 3, 4: each position of the groups 2 + 3 + 3 + ...


def ruler(n=RULER, var=False):
    """A path whose edge v (between v - 1 and v) carries 100 - ctz(v) common hashes of 100."""
    rng = np.random.default_rng(2102)
    v = np.arange(1, n)
    ctz = np.array([(int(x) & -int(x)).bit_length() - 1 for x in v])
    lens = np.full(n, 100, dtype=np.uint32)
    if var:
        lens[0] = 101
    return _pack(n, v, v - 1, 100 - ctz, lens, 0, rng)


# ---- star: 64 lanes name one component, and 64 different ones ------------------------------------------------------------------
STAR = 5000
STAR_HUB = 2500


def star(distinct, var=False):
    """Hub STAR_HUB in the middle of the ids, so that it is the j of half its edges and the i of the rest.  Equal weights: the
    hub's choice is pure id order, (STAR_HUB, 0).  With sizes that vary the weight is common / min (mode 1) and every leaf
    is at least as long as the hub, so the weights stay equal."""
    rng = np.random.default_rng(2103 + distinct)
    leaves = np.array([v for v in range(STAR) if v != STAR_HUB])
    common = rng.permutation(STAR - 1) + 1 if distinct else np.full(STAR - 1, 7)
    lens = np.full(STAR, STAR, dtype=np.uint32)
    if var:
        lens = (STAR + rng.integers(0, 50, size=STAR)).astype(np.uint32)
        lens[STAR_HUB] = STAR
    return _pack(STAR, leaves, np.full(STAR - 1, STAR_HUB), common, lens, 1 if var else 0, rng)


# ---- pooling: waves whose on-lanes name exactly four, five or six, and many components -------------------------------------------
POOL_CLIQUE = 8
POOL_RUNS = (16,) * 12 + (13,) * 24 + (7,) * 27  # 192 + 312 + 189 bridge edges; the runs of 16 start on a multiple of 64


def pooling(shuffled=False, var=False):
    """len(POOL_RUNS) + 1 cliques of 8 with equal weights inside, so that in round one every member hooks onto the clique's
    first vertex (pure id order) and a clique is one component from round two on.  Clique r + 1 is joined to clique r by
    POOL_RUNS[r] bridges of lower, random weights, consecutive in the list: 64 consecutive entries name 4 components with the
    runs of 16, 5 or 6 with the runs of 13, 10 or 11 with the runs of 7 -- on the i side and on the j side alike."""
    rng = np.random.default_rng(2104)
    cliques = len(POOL_RUNS) + 1
    n = cliques * POOL_CLIQUE
    i, j, c = [], [], []
    for q in range(cliques):
        for a in range(POOL_CLIQUE):
            for b in range(a):
                i.append(q * POOL_CLIQUE + a); j.append(q * POOL_CLIQUE + b); c.append(90)
    first_bridge = len(i)
    assert first_bridge % 64 == 0  # 64 cliques of 28 edges: the bridges begin with a wave
    for r, run in enumerate(POOL_RUNS):
        cells = rng.permutation(POOL_CLIQUE * POOL_CLIQUE)[:run]
        for cell in cells:
            i.append((r + 1) * POOL_CLIQUE + int(cell) // POOL_CLIQUE); j.append(r * POOL_CLIQUE + int(cell) % POOL_CLIQUE)
            c.append(int(rng.integers(1, 12)))
    lens = np.full(n, 100, dtype=np.uint32)
    if var:
        lens = (100 + (np.arange(n) // POOL_CLIQUE) % 3).astype(np.uint32)  # one size per clique: the weights inside stay equal
    case = _pack(n, i, j, c, lens, 0, rng if shuffled else None)
    return case, first_bridge


# ---- complete graphs --------------------------------------------------------------------------------------------------------
def complete_size(num_cu, turns):
    """1 100 and 1 500 vertices with 256 compute units: 604 450 edges are past one turn, 1 124 250 past two"""
    k = int(np.ceil((1100, 1500)[turns - 1] * np.sqrt(num_cu / 256.0)))
    while k * (k - 1) // 2 <= turns * turn(num_cu):
        k += 1
    return k


def complete(k, counts, var=False, seed=2105):
    """K_k.  counts == 1: every count and every size equal, the forest is (i, 0) for all i.  Else that many distinct counts;
    with sizes that vary, common / min (mode 1) over sizes 1 000 and 1 001 by the parity of the id."""
    rng = np.random.default_rng(seed + k)
    i, j = np.tril_indices(k, -1)
    common = np.full(len(i), 40) if counts == 1 else 40 + rng.integers(0, counts, size=len(i))
    lens = np.full(k, 1000, dtype=np.uint32)
    if var:
        lens = (1000 + np.arange(k) % 2).astype(np.uint32)
    return _pack(k, i, j, common, lens, 1 if var else 0, rng)


# ---- equal doubles from different counts ------------------------------------------------------------------------------------
RATIO_SIZES = (4, 6, 8, 10, 12, 16, 20, 24, 40, 60, 100, 200)
RATIO_TARGETS = ((1, 1), (1, 2), (1, 3), (2, 3), (1, 4), (3, 4), (1, 5))
RATIO_S = {"below": 3, "inside": 50, "above": 1000}  # mode 2: s against unions of 4 .. 400


def ratios(wmode, seed=2106):
    """600 vertices with sizes from RATIO_SIZES, 3 000 edges; wherever a count exists that makes common / denom one of
    RATIO_TARGETS the edge takes one, so that 2/4, 3/6 and 50/100 meet many times"""
    from fractions import Fraction
    rng = np.random.default_rng(seed + wmode % 64)
    n = 600
    lens = rng.choice(RATIO_SIZES, size=n)
    i, j = _distinct_pairs(rng, n, 3000)
    targets = {Fraction(p, q) for p, q in RATIO_TARGETS}
    table = {}

    def good(la, lb):
        if (la, lb) not in table:
            top = min(la, lb)
            if (wmode & 3) == 2:
                top = min(top, wmode >> 2)
            out = []
            for c in range(1, top + 1):
                d = min(la, lb) if (wmode & 3) == 1 else la + lb - c
                if (wmode & 3) == 2:
                    d = min(d, wmode >> 2)
                if Fraction(c, d) in targets:
                    out.append(c)
            table[(la, lb)] = (out, top)
        return table[(la, lb)]
    common = []
    for a, b in zip(i.tolist(), j.tolist()):
        out, top = good(int(lens[a]), int(lens[b]))
        common.append(int(rng.choice(out)) if out else int(rng.integers(0, top + 1)))
    return _pack(n, i, j, common, lens, wmode, rng)


# ---- zero and empty ---------------------------------------------------------------------------------------------------------
def empty(n=7):
    return _pack(n, [], [], [], np.arange(n) + 3, 0)


def pair(with_edge):
    return _pack(2, [1] if with_edge else [], [0] if with_edge else [], [3] if with_edge else [], [9, 5], 0)


def zeros(wmode, seed=2107):
    """300 vertices in three blocks of 100 without an edge between them; in every block the first three vertices have no
    edge at all, the next two have size 0 and are joined to each other and to the block by edges of denom 0 / common 0, and a
    quarter of the other edges has common 0 (J = 0: the largest key, equal for all of them)"""
    rng = np.random.default_rng(seed + wmode)
    n = 300
    lens = rng.integers(1, 30, size=n)
    i, j, c = [], [], []
    for base in (0, 100, 200):
        lens[base + 3] = lens[base + 4] = 0
        i += [base + 4, base + 20, base + 50]; j += [base + 3, base + 3, base + 4]; c += [0, 0, 0]
        a, b = _distinct_pairs(rng, 95, 240)
        for x, y in zip((a + base + 5).tolist(), (b + base + 5).tolist()):
            i.append(x); j.append(y)
            c.append(0 if rng.integers(0, 4) == 0 else int(rng.integers(0, min(lens[x], lens[y]) + 1)))
    return _pack(n, i, j, c, lens, wmode, rng)


def hook_order():
    """Three vertices, (2, 0) the most similar pair and (1, 0) the other edge: 0 and 2 pick each other, 1 hooks onto 0.  The
    smaller root, 0, records (2, 0) ahead of vertex 1's (1, 0); were the larger root kept, 2 would record it behind."""
    return _pack(3, [2, 1], [0, 0], [9, 4], [10, 10, 10], 0)


# ---- key layouts at the 63-bit line ---------------------------------------------------------------------------------------------
LAYOUT_EQUAL = (1 << 30) + 5
LAYOUT_EDGES = 300_000


def key_bits(n, longest):
    """(b, w): index bits and count bits as rtc_boruvka_key_bits and rtc_msf_device count them"""
    b = 1
    while b < 32 and (1 << b) < n:
        b += 1
    w = 1
    while w < 32 and (1 << w) <= longest:
        w += 1
    return b, w


def layout(n, var):
    """LAYOUT_EDGES random edges over n = 65 536 or 65 537 vertices whose sizes are all 2^30 + 5, or vary inside
    [2^30, 2^31); the last vertex has edges; a third of the counts is within 3 of 0, a third within 3 of the smaller size, the
    rest comes from 1 000 values"""
    rng = np.random.default_rng(2108 + n % 7 + 10 * var)
    lens = rng.integers(1 << 30, 1 << 31, size=n) if var else np.full(n, LAYOUT_EQUAL)
    i, j = _distinct_pairs(rng, n, LAYOUT_EDGES)
    i[:40], j[:40] = n - 1, np.arange(40) * 1500  # (distinct from each other; a repeat of a random pair is removed below)
    u = np.unique(i * np.int64(n) + j)
    i, j = u // n, u % n
    top = np.minimum(lens[i], lens[j])
    kind = rng.integers(0, 3, size=len(i))
    near = rng.integers(0, 4, size=len(i))
    values = rng.integers(4, 1 << 30, size=1000)
    common = np.where(kind == 0, near, np.where(kind == 1, top - near, values[rng.integers(0, 1000, size=len(i))]))
    return _pack(n, i, j, common, lens, 0, rng)


# ---- vertices past one turn ---------------------------------------------------------------------------------------------------
def forest_size(num_cu):
    return max(600_000 * num_cu // 256, turn(num_cu) + 70_000)


def random_forest(num_cu):
    """Vertex v attaches to a random earlier one, 1 % stay roots: the list is a forest, so the result is the list in (key, i, j)
    order.  Sizes 50 .. 150, counts 1 .. the smaller size."""
    n = forest_size(num_cu)
    rng = np.random.default_rng(2109)
    v = np.arange(1, n)
    v = v[rng.random(n - 1) >= 0.01]
    to = (rng.random(len(v)) * v).astype(np.int64)
    lens = rng.integers(50, 151, size=n)
    common = 1 + (rng.random(len(v)) * np.minimum(lens[v], lens[to])).astype(np.int64)
    return _pack(n, v, to, common, lens, 0, rng)


# ---- random sparse graphs -----------------------------------------------------------------------------------------------------
def sparse(seed):
    rng = np.random.default_rng(2200 + seed)
    n = int(rng.integers(2, 5001))
    degree = float(rng.uniform(1, 8))
    m = min(int(n * degree / 2), n * (n - 1) // 2)
    fixed = bool(rng.integers(0, 2))
    smax = int(rng.choice([6, 40, 3000]))
    lens = np.full(n, smax) if fixed else rng.integers(0 if smax == 6 else 1, smax + 1, size=n)
    mode = int(rng.integers(0, 3))
    wmode = mode if mode < 2 else 2 | int(rng.integers(1, 2 * smax)) << 2
    i, j = _distinct_pairs(rng, n, m) if n > 2 else (np.array([1]), np.array([0]))
    top = np.minimum(lens[i], lens[j])
    if mode == 2:
        top = np.minimum(top, wmode >> 2)
    common = (rng.random(len(i)) * (top + 1)).astype(np.int64)
    if len(i) > 8:  # exact copies of weights: the counts and sizes of another edge's ends
        lens[i[:4]], lens[j[:4]] = lens[i[4:8]], lens[j[4:8]]
        top = np.minimum(lens[i], lens[j])
        if mode == 2:
            top = np.minimum(top, wmode >> 2)
        common = np.minimum(common, top)
        if fixed:
            common[:4] = common[4:8]
    return _pack(n, i, j, common, lens, wmode, rng)


# ---- the list of cases --------------------------------------------------------------------------------------------------------
def builders(num_cu):
    k1, k2 = complete_size(num_cu, 1), complete_size(num_cu, 2)
    b = {
        "chain": lambda: chain(), "chain_var": lambda: chain(True),
        "ruler": lambda: ruler(), "ruler_var": lambda: ruler(var=True),
        "star_equal": lambda: star(False), "star_equal_var": lambda: star(False, True),
        "star_distinct": lambda: star(True), "star_distinct_var": lambda: star(True, True),
        "pooling": lambda: pooling()[0], "pooling_var": lambda: pooling(var=True)[0],
        "pooling_shuffled": lambda: pooling(True)[0], "pooling_shuffled_var": lambda: pooling(True, True)[0],
        "k300_equal": lambda: complete(300, 1),
        "k_one_turn": lambda: complete(k1, 10), "k_one_turn_var": lambda: complete(k1, 10, True),
        "k_two_turns_var": lambda: complete(k2, 10, True),
        "ratios_mode0": lambda: ratios(0), "ratios_mode1": lambda: ratios(1),
        "empty": lambda: empty(), "pair_without": lambda: pair(False), "pair_with": lambda: pair(True),
        "zeros_mode0": lambda: zeros(0), "zeros_mode1": lambda: zeros(1), "hook_order": hook_order,
        "layout_65536": lambda: layout(65536, False), "layout_65537": lambda: layout(65537, False),
        "layout_65536_var": lambda: layout(65536, True), "layout_65537_var": lambda: layout(65537, True),
        "forest": lambda: random_forest(num_cu),
    }
    b.update({"ruler_%d" % n: (lambda n=n: ruler(n)) for n in RULER_SMALL})
    b.update({"ratios_s_%s" % k: (lambda s=s: ratios(2 | s << 2)) for k, s in RATIO_S.items()})
    b.update({"sparse_%d" % s: (lambda s=s: sparse(s)) for s in range(1, SOAK_SEEDS + 1)})
    return b


def names(num_cu=256):
    return sorted(builders(num_cu))


LARGEST = ("k_two_turns_var", "forest")  # left out where every round is a host round trip
IS_FOREST = ("forest",)                  # the list is a forest: no Kruskal needed


def case(name, num_cu=256):
    key = (name, num_cu)
    if key not in _CACHE:
        _CACHE[key] = builders(num_cu)[name]()
    return _CACHE[key]


def reordered(edges, name):
    """the same list in another order (the reverse of a list whose order is the case, another shuffle otherwise)"""
    if name in ("pooling", "pooling_var") or len(edges) < 3:
        return np.ascontiguousarray(edges[::-1])
    return np.ascontiguousarray(edges[np.random.default_rng(len(edges)).permutation(len(edges))])
