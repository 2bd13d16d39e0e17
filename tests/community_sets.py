"""Inputs the rtc_louvain / rtc_leiden edge tests share (tests/test_cpu_community_sets.py proves on the restatements that they
hold their cases, tests/test_gpu_community_edges.py runs them on the GPU): more rows than a launch has workgroups, rows at the
lengths where the row kernel changes path, probe chains that wrap round the end of a table, chains that run into the caps,
self loops with duplicate and reversed records, and total weight just under 2^46.  Every set is (n, edges), edges a list of
(u, v, q); boundary_stars returns a dict of such sets."""
import numpy as np

ONE = 1 << 20
GOLDEN = 2654435761  # the row kernel's hash: the home slot of community d is (d * GOLDEN mod 2^32) >> (32 - log2 slots)

_CACHE = {}


def clique(vs, q):
    vs = list(vs)
    return [(a, b, q) for i, a in enumerate(vs) for b in vs[i + 1:]]


def home_slot(d, log2_slots):
    return ((d * GOLDEN) & 0xffffffff) >> (32 - log2_slots)


def many_short_rows(num_cu):
    """32 num_cu + 200 vertices, every one with a row of 3 to 7 entries: cliques of 3 to 6 members with random weights in
    [ONE/2, ONE), clique 2k joined to clique 2k + 1 by one light edge and to nothing else.  (Joined in a ring or a chain the
    aggregated graph is a path, on which the synchronous rule oscillates up to both caps.)  The wave path's launch has
    32 num_cu workgroups, so 200 of them take a second row."""
    key = ("short", num_cu)
    if key not in _CACHE:
        rng = np.random.default_rng(1301)
        n = 32 * num_cu + 200
        edges, first, at = [], [], 0
        while at < n:
            size = int(rng.integers(3, 7))
            left = n - at - size
            if left < 0:
                size = n - at
            elif left in (1, 2):
                size = size + left if size + left <= 6 else size - (3 - left)
            first.append(at)
            for a in range(at, at + size):
                for b in range(a + 1, at + size):
                    edges.append((a, b, int(rng.integers(ONE // 2, ONE))))
            at += size
        for a, b in zip(first[0::2], first[1::2]):
            edges.append((a + 1, b, int(rng.integers(ONE // 64, ONE // 16))))
        _CACHE[key] = (n, edges)
    return _CACHE[key]


LONG_BLOCK = 135
LONG_WEIGHTS = (ONE // 2, 5 * ONE // 8, 3 * ONE // 4, 7 * ONE // 8)
LONG_LINKS = (ONE // 64, ONE // 32, ONE // 16, ONE // 8)


def many_long_rows(num_cu):
    """ceil((3 num_cu + 40) / 135) complete blocks of 135 vertices, so every row has 134 entries or more and the block path's
    launch of 3 num_cu workgroups has rows left for a second turn.  The weights inside a block come from four values and the
    200 light links of a block to other blocks from four more, so that equal scores are common.  The first vertex of every
    block but block 0 is linked to the first vertex of the block before by ONE/8: in round 0 of a refinement it has no
    candidate below it in its own block, so under modularity only the coarse filter keeps it from proposing across."""
    key = ("long", num_cu)
    if key not in _CACHE:
        rng = np.random.default_rng(1302)
        blocks = -(-(3 * num_cu + 40) // LONG_BLOCK)
        n = blocks * LONG_BLOCK
        edges = []
        for b in range(blocks):
            lo = b * LONG_BLOCK
            for x in range(lo, lo + LONG_BLOCK):
                for y in range(x + 1, lo + LONG_BLOCK):
                    edges.append((x, y, LONG_WEIGHTS[int(rng.integers(0, 4))]))
        seen = set()
        for b in range(1, blocks):
            seen.add(((b - 1) * LONG_BLOCK, b * LONG_BLOCK))
            edges.append((b * LONG_BLOCK, (b - 1) * LONG_BLOCK, ONE // 8))
        for b in range(blocks):
            made = 0
            while made < 200:
                x = b * LONG_BLOCK + int(rng.integers(0, LONG_BLOCK))
                y = int(rng.integers(0, n))
                if y // LONG_BLOCK == b or (min(x, y), max(x, y)) in seen:
                    continue
                seen.add((min(x, y), max(x, y)))
                edges.append((x, y, LONG_LINKS[int(rng.integers(0, 4))]))
                made += 1
        _CACHE[key] = (n, edges)
    return _CACHE[key]


def heavy_star(units=1000):
    """A centre numbered 2 100 tied to 2 100 leaves by about `units` units each, and the leaf pairs (i, i + 1), even i < 600, by
    three units: the centre's row lies on the global path.  units = 1000: under CPM at resolution 0.25 the centre is a lone
    eligible proposer, and M2 is about 2^42.  units = 1: the same at resolution 1/4096."""
    star = [(2100, i, units * ONE + (i * 7919) % 13) for i in range(2100)]
    return 2101, star + [(i, i + 1, 3 * ONE) for i in range(0, 600, 2)]


BOUNDARY_LENGTHS = (128, 129, 2048, 2049)
BOUNDARY_PAIRS = 100  # tied up to leaf 600, as star_2100 is, Leiden's modularity does not settle on the two long stars: see cycling_star


def boundary_star(length, self_loop):
    """A star whose centre, the highest number, has a row of exactly `length` entries: `length` leaves, or one leaf fewer and a
    self loop at the centre (the row length counts the self entry).  Weights as in Louvain's star_300, leaf pairs as in
    star_2100."""
    leaves = length - 1 if self_loop else length
    edges = [(leaves, i, 1 + (i * 7919) % 13) for i in range(leaves)]
    edges += [(i, i + 1, 3) for i in range(0, min(BOUNDARY_PAIRS, leaves - 1), 2)]
    if self_loop:
        edges.append((leaves, leaves, 5))
    return leaves + 1, edges


def boundary_stars():
    return {"star_%d%s" % (length, "_self" if loop else ""): boundary_star(length, loop) for length in BOUNDARY_LENGTHS for loop in (False, True)}


COLLIDING = {8: (40, 60), 12: (16, 984), 13: (8, 2500)}  # log2 slots: (colliding neighbours, other neighbours)
COLLIDING_BALLAST = {8: 1, 12: 5, 13: 10}  # edges of 100 000 between vertices of their own: they set M2, see colliding_star


def colliding_ids(log2_slots, n=65536):
    """the ids below n - 1 whose home slot in a table of 1 << log2_slots slots is the last one"""
    d = np.arange(n - 1, dtype=np.uint64)
    home = ((d * np.uint64(GOLDEN)) & np.uint64(0xffffffff)) >> np.uint64(32 - log2_slots)
    return np.nonzero(home == np.uint64((1 << log2_slots) - 1))[0].tolist()


def colliding_star(log2_slots):
    """65 536 vertices, most of them isolated; the centre, 65 535, is tied to ids whose home slot is the table's last (so their
    probe chain wraps round to slot 0) and to enough other ids that its row takes the table of 1 << log2_slots slots: 8 the
    wave's, 12 the workgroup's, 13 the smallest global one.  The colliding ids carry the two heaviest weights in alternation,
    so the centre's best community in round 0 is one of them and is decided among equals by the smaller id.  On a bare star
    everything ends in one community whichever leaf the centre chose.  So every colliding id also heads a heavy triangle of its
    own, and a few heavy edges between otherwise isolated vertices bring M2 to where the centre's score for a triangle's head,
    51 M2 - k_centre k_head, is still the best one while the triangles it did not choose stay apart: the labels differ with the
    choice.  No weight reaches a quarter of a unit: CPM at 0.25 moves nothing."""
    key = ("colliding", log2_slots)
    if key not in _CACHE:
        n = 65536
        n_hit, n_other = COLLIDING[log2_slots]
        every = colliding_ids(log2_slots, n)
        hit = every[-n_hit:]
        rng = np.random.default_rng(1303 + log2_slots)
        taken = set(every)
        free = [int(y) for y in rng.permutation(n - 1).tolist() if y not in taken]
        others, free = free[:n_other], free[n_other:]
        edges = [(n - 1, y, 50 + (i & 1)) for i, y in enumerate(hit)]
        edges += [(n - 1, y, 1 + (y * 7919) % 13) for y in others]
        for i, y in enumerate(hit):  # a triangle of its own for every colliding id: the centre's choice stays visible in the labels
            a, b = free[2 * i], free[2 * i + 1]
            edges += [(y, a, 1000), (y, b, 1000), (a, b, 1000)]
        for j in range(n_hit, n_hit + COLLIDING_BALLAST[log2_slots]):
            edges.append((free[2 * j], free[2 * j + 1], 100_000))
        _CACHE[key] = (n, edges)
    return _CACHE[key]


def cycling_star():
    """Louvain's star_300 with the leaf pairs (i, i + 1), even i < 100, tied by 3: under modularity at resolution 1 the iterations
    of Leiden alternate between two partitions and end at the cap of 100."""
    return 301, [(300, i, 1 + (i * 7919) % 13) for i in range(300)] + [(i, i + 1, 3) for i in range(0, 100, 2)]


def nontarget_star():
    """A star of 1 000 leaves with the leaf pairs (i, i + 1), even i < 600, tied by 3.  Under modularity at resolution 1 the
    second level has a row of 301 entries whose lone vertex proposes while a neighbouring refined community is no target."""
    return 1001, [(1000, i, 1 + (i * 7919) % 13) for i in range(1000)] + [(i, i + 1, 3) for i in range(0, 600, 2)]


def chain(n):
    """a path of equal weights: the synchronous rule oscillates on it"""
    return n, [(i, i + 1, ONE) for i in range(n - 1)]


def loops_and_duplicates():
    """two weight layers on a 4-clique, self loops, a pair given in both orders and a triangle: Louvain's first such case"""
    return 9, clique(range(4), 10) + clique(range(4), 7) + [(4, 4, 50), (4, 5, 9), (5, 4, 9), (5, 6, 30), (6, 7, 30), (7, 5, 30), (3, 4, 1), (8, 8, 4),
                                                          (0, 0, 3)]


def loops_and_duplicates_large():
    """60 vertices in 5 planted blocks by residue; every vertex has a self loop, and a fifth of the records are a repeat of an
    earlier record or an earlier record turned round (u > v).  Vertices 60 to 65 are tests/leiden_sets.py's pendant with self
    loops: a 5-clique of unit weights and vertex 65 hanging on vertex 60 by half a unit, with a self loop of one unit (two in
    the row).  Under CPM at 0.25 all six join community 60 in round 0 and vertex 65 then fails the eligibility test, which they would pass if the self entry counted."""
    if "loops" not in _CACHE:
        rng = np.random.default_rng(1304)
        n = 60
        edges = [(x, x, int(rng.integers(ONE // 8, ONE // 2))) for x in range(n)]
        for x in range(n):
            for y in range(x + 1, n):
                p = 0.8 if x % 5 == y % 5 else 0.06
                if rng.random() < p:
                    edges.append((x, y, int(rng.integers(ONE // 4, ONE))))
        edges += clique(range(60, 65), ONE) + [(65, 60, ONE // 2)] + [(x, x, ONE) for x in range(60, 66)]
        base = len(edges)
        for i in rng.choice(base, size=base // 4, replace=False).tolist():  # a quarter more: a fifth of the total
            u, v, q = edges[i]
            edges.append((v, u, int(rng.integers(ONE // 8, ONE // 2))) if rng.random() < 0.5 else (u, v, q))
        order = rng.permutation(len(edges)).tolist()
        _CACHE["loops"] = (n + 6, [edges[i] for i in order])
    return _CACHE["loops"]


def near_limit():
    """Two 6-cliques and a bridge with M2 = 2^46 - 2^19, within 2^20 of the largest total the calls take.  A record holds at
    most 2^32 - 1, so every pair is given as some 270 records."""
    if "limit" not in _CACHE:
        total = (1 << 45) - (1 << 18)  # the sum of all q: M2 / 2
        pairs = clique(range(6), 0) + clique(range(6, 12), 0)
        bridge = total >> 9
        share, rest = divmod(total - bridge, len(pairs))
        edges = []
        for i, (u, v, _) in enumerate(pairs + [(5, 6, 0)]):
            w = bridge if (u, v) == (5, 6) else share + (1 if i < rest else 0)
            while w > 0:
                q = min(w, 0xffffffff)
                edges.append((u, v, q) if len(edges) % 3 else (v, u, q))
                w -= q
        assert 2 * sum(q for _, _, q in edges) == (1 << 46) - (1 << 19)
        _CACHE["limit"] = (12, edges)
    return _CACHE["limit"]
