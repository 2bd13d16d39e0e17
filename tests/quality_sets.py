"""Inputs the rtc_silhouette tests share (tests/test_cpu_quality.py proves on the restatement that they hold their cases,
tests/test_gpu_quality.py runs them on the GPU).  Every set is (n, edges, labels): edges a list of (u, v, q), labels an int array,
negative for an unclustered vertex."""
import numpy as np

from tests.community_sets import colliding_ids

ONE = 1 << 20
NONE = 0xFFFFFFFF
# mirrors of rabbittclust_amd/csrc/rtc_quality.h (tests/test_cpu_quality.py holds them against api's and the header's)
WAVE_ROW, WAVE_SLOTS, BLOCK_ROW, BLOCK_SLOTS, GLOBAL_LOG2_MIN = 128, 256, 1024, 2048, 6
WAVE, WORKGROUP, GLOBAL = 1, 2, 4
WGS_PER_CU = {WAVE: 32, WORKGROUP: 4, GLOBAL: 8}  # SIL_WAVE_ / SIL_BLOCK_ / SIL_GLOBAL_WGS_PER_CU: a path's grid, a row a workgroup and turn

_CACHE = {}


def table_log2(length, all_global=False):
    """log2 of the slots of the table a row of `length` entries gets"""
    if not all_global and length <= WAVE_ROW:
        return 8
    if not all_global and length <= BLOCK_ROW:
        return 11
    lg = GLOBAL_LOG2_MIN
    while (1 << lg) < 2 * length:
        lg += 1
    return lg


def path_of(length, all_global=False):
    return GLOBAL if all_global or length > BLOCK_ROW else WAVE if length <= WAVE_ROW else WORKGROUP


def random_graph(seed, n, p_edge=0.3, n_clusters=4, p_noise=0.1, lonely_cluster=False):
    """n vertices in up to n_clusters clusters with scattered ids, some unclustered; every pair listed with probability p_edge at a
    random q, a tenth of them at 0 or ONE.  lonely_cluster: the members of one cluster lose all their records."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(n, size=min(n_clusters, n), replace=False)
    labels = ids[rng.integers(0, len(ids), size=n)].astype(np.int64)
    labels[rng.random(n) < p_noise] = -1
    lonely = int(ids[0]) if lonely_cluster else None
    edges = []
    for u in range(n):
        for v in range(u):
            if rng.random() >= p_edge or (lonely is not None and lonely in (labels[u], labels[v])):
                continue
            r = rng.random()
            edges.append((u, v, 0 if r < 0.05 else ONE if r < 0.1 else int(rng.integers(1, ONE))))
    return n, edges, labels


BOUNDARY_LENGTHS = (WAVE_ROW, WAVE_ROW + 1, BLOCK_ROW, BLOCK_ROW + 1)


def boundary_star(length):
    """A centre, the highest number, with a row of exactly `length` entries.  The leaves lie in five clusters (ids 3, 7, 11, 19 and
    the centre's own, 2) of different sizes, a few leaves are unclustered, q falls into eight values so that sums tie now and
    then, and every fifth pair of neighbouring leaves is listed too: those rows are short."""
    if ("star", length) not in _CACHE:
        n = length + 1
        ids = (2, 3, 7, 11, 19)
        labels = np.array([ids[(i * 7 + i // 5) % 5] for i in range(n)], dtype=np.int64)
        labels[n - 1] = 2
        labels[5:n - 1:37] = -1
        edges = [(n - 1, i, ((i * 7919) % 8 + 1) * (ONE // 16)) for i in range(length)]
        edges += [(i, i + 1, ONE // 3) for i in range(0, length - 1, 5)]
        _CACHE[("star", length)] = (n, edges, labels)
    return _CACHE[("star", length)]


COLLIDING_ROWS = {8: 100, 11: 1000, 12: 2000}  # log2 slots of the table: the centre's row, the same table with and without RTC_SIL_GLOBAL


def colliding_star(log2_slots):
    """65 536 vertices, most of them unclustered and without a record.  The centre, 65 535, has a row of COLLIDING_ROWS[log2_slots]
    entries, which gives it the table of 1 << log2_slots slots on its own path and on the global one alike.  Its first neighbours
    lie one each in the clusters whose home slot is the table's last (tests/community_sets.py: colliding_ids), so their probe
    chain wraps round to slot 0; they carry the two least q in alternation, so the best other cluster is one of them and is
    decided among equal means by the smaller id.  The other neighbours lie in clusters drawn from the remaining ids, several to
    a cluster, at larger q.  The centre's own cluster is another colliding id."""
    if ("colliding", log2_slots) not in _CACHE:
        n = 65536
        length = COLLIDING_ROWS[log2_slots]
        every = colliding_ids(log2_slots, n)
        hit = every[-min(len(every) - 1, 24):]
        own = every[0]
        rng = np.random.default_rng(2300 + log2_slots)
        taken = set(every)
        free_ids = [int(y) for y in rng.permutation(n - 1).tolist() if y not in taken]
        other_clusters = free_ids[:max(8, length // 6)]
        labels = np.full(n, -1, dtype=np.int64)
        labels[n - 1] = own
        vertices = [int(v) for v in rng.permutation(n - 1)[:length].tolist()]
        edges = []
        for i, v in enumerate(vertices):
            if i < len(hit):
                labels[v] = hit[i]
                q = ONE // 8 + (i & 1)
            elif i < len(hit) + 3:
                labels[v] = own
                q = ONE // 2 + i
            else:
                labels[v] = other_clusters[int(rng.integers(0, len(other_clusters)))]
                q = ONE // 4 + int(rng.integers(0, ONE // 2))
            edges.append((n - 1, v, q) if i % 3 else (v, n - 1, q))
        _CACHE[("colliding", log2_slots)] = (n, edges, labels)
    return _CACHE[("colliding", log2_slots)]


def arithmetic():
    """Clusters 0 = {0, 1, 2}, 1 = {3, 4}, 2 = {5, 6, 7, 8}, 9 = {9} and vertex 10 unclustered.
    Vertex 0 lists all of cluster 1 and all of cluster 2 at ONE / 2: equal means under different sizes, the smaller id wins, and
    the complement term of both is 0.  Vertex 1 lists vertex 3 at ONE and nothing else outside: the best mean is exactly ONE, so
    b_cluster is none while near_cluster is 1.  (1, 2) is listed at 0.  Vertex 2's neighbours all lie in its own cluster.  Vertex
    9 is a singleton with a record; vertex 10 has records, which are ignored."""
    labels = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 9, -1], dtype=np.int64)
    edges = [(0, y, ONE // 2) for y in (3, 4, 5, 6, 7, 8)] + [(0, 1, ONE // 4), (2, 0, 3 * ONE // 4), (1, 2, 0), (3, 1, ONE), (9, 5, ONE // 8),
                                                                (10, 0, 5), (10, 9, 7), (4, 10, 0)]
    return 11, edges, labels


BIG_A, BIG_B = 256, 2  # the two foreign clusters have 2^22 + 256 (id 2) and 2^22 + 2 (id 3) members


def _listed(total_deficit):
    """q of the listed neighbours of one cluster whose deficits ONE - q sum to total_deficit: all but the last at ONE / 4 or 0 in
    alternation, the last takes the rest"""
    qs, left, i = [], total_deficit, 0
    while left > ONE:
        q = ONE // 4 if i % 2 and left > 2 * ONE else 0
        qs.append(q)
        left -= ONE - q
        i += 1
    qs.append(ONE - left)
    return qs


def past_64_bits():
    """Cluster 0 = {0, 1}; cluster 2 holds the N1 = 2^22 + 256 vertices from 2 on, cluster 3 the N2 = 2^22 + 2 after them, nearly all
    without a record: only the label array and the output are large.
    N2 divides 2^64 + 2 and N1 divides 2^64 - 256.  Vertex 0 lists a few hundred members of each at distances chosen so that
    S1 = (2^64 + 2) / N2 and S2 = (2^64 - 256) / N1: the cross products are S1 N2 = 2^64 + 2 and S2 N1 = 2^64 - 256.  S2 N1 is the
    smaller, so cluster 3 is the nearer: the right answer is the LARGER id.  The two products straddle 2^64: their high words
    differ, and their low 64 bits are 2 and 2^64 - 256, in the reverse order -- a product kept to 64 bits picks cluster 2.  Both
    round to the double 2^64 -- compared as doubles they tie, and the tie goes to the smaller id, cluster 2 again.  Vertex 1
    lists one member of each at ONE / 2."""
    if "big" not in _CACHE:
        n1, n2 = (1 << 22) + BIG_A, (1 << 22) + BIG_B
        assert ((1 << 64) + 2) % n2 == 0 and ((1 << 64) - 256) % n1 == 0
        s1, s2 = ((1 << 64) + 2) // n2, ((1 << 64) - 256) // n1
        n = 2 + n1 + n2
        labels = np.empty(n, dtype=np.int64)
        labels[:2] = 0
        labels[2:2 + n1] = 2
        labels[2 + n1:] = 3
        edges = []
        for first, size, total in ((2, n1, s1), (2 + n1, n2, s2)):
            for i, q in enumerate(_listed(size * ONE - total)):  # S = size ONE - the deficits
                y = first + 7 * i
                edges.append((0, y, q) if i % 2 else (y, 0, q))
        edges += [(1, 2, ONE // 2), (2 + n1, 1, ONE // 2)]
        _CACHE["big"] = (n, edges, labels)
    return _CACHE["big"]


def big_products(n, edges, labels, x):
    """(S1 N2, S2 N1) of vertex x of past_64_bits against clusters 2 and 3"""
    size = {2: int((labels == 2).sum()), 3: int((labels == 3).sum())}
    s = {}
    for d in (2, 3):
        qs = [q for u, v, q in edges if (u == x and labels[v] == d) or (v == x and labels[u] == d)]
        s[d] = sum(qs) + (size[d] - len(qs)) * ONE
    return s[2] * size[3], s[3] * size[2]


def one_cluster(n=40):
    """every vertex in cluster 5: b_den is 0 everywhere"""
    rng = np.random.default_rng(77)
    edges = [(u, v, int(rng.integers(0, ONE + 1))) for u in range(n) for v in range(u) if rng.random() < 0.4]
    return n, edges, np.full(n, 5, dtype=np.int64)


def singletons(n=30):
    """every vertex alone in the cluster of its own number, some pairs listed"""
    rng = np.random.default_rng(78)
    edges = [(u, v, int(rng.integers(0, ONE + 1))) for u in range(n) for v in range(u) if rng.random() < 0.3]
    return n, edges, np.arange(n, dtype=np.int64)


def _circulant(n, reach, seed):
    """Vertex x is listed with x + 1 .. x + reach (mod n), the orientation alternating: every row has 2 reach entries.  q takes
    eight values, so sums and means tie; the labels are nine scattered ids, and every 41st vertex is unclustered.  The rows of a
    path stand in vertex order, so with a grid of G workgroups, workgroup b meets the b-th, (b + G)-th, ... clustered vertex:
    rows over the same nine clusters, one after the other in the same table."""
    assert n > 2 * reach
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(n, size=9, replace=False))
    labels = ids[rng.integers(0, 9, size=n)].astype(np.int64)
    labels[40::41] = -1
    q = ((rng.integers(0, 8, size=(n, reach)) + 1) * (ONE // 16)).tolist()
    edges = []
    for x in range(n):
        for k in range(1, reach + 1):
            y = (x + k) % n
            edges.append((x, y, q[x][k - 1]) if (x + k) % 2 else (y, x, q[x][k - 1]))
    return n, edges, labels


def many_short_rows(num_cu):
    """32 num_cu + 501 vertices with rows of 6 entries: more rows than the wave path's grid, and than the global path's under
    RTC_SIL_GLOBAL=1"""
    if ("short", num_cu) not in _CACHE:
        _CACHE[("short", num_cu)] = _circulant(WGS_PER_CU[WAVE] * num_cu + 501, 3, 2400)
    return _CACHE[("short", num_cu)]


def many_long_rows(num_cu):
    """4 num_cu + 77 vertices with rows of 130 entries, just past WAVE_ROW: more rows than the workgroup path's grid"""
    if ("long", num_cu) not in _CACHE:
        _CACHE[("long", num_cu)] = _circulant(WGS_PER_CU[WORKGROUP] * num_cu + 77, (WAVE_ROW + 2) // 2, 2401)
    return _CACHE[("long", num_cu)]


# ---- sketches for rtc_cluster_quality ----------------------------------------------------------------------------------------
def family_sketches(seed, width, n_families=9, per_family=6, pool=400):
    """n_families * per_family + 6 sketches: every family draws 120 to 300 hashes a member from a pool of its own, and a tenth of
    each sketch from a pool all families share, so members of different families share a little or nothing; then one empty
    sketch, one of 12 hashes inside the first member of family 0 (the size-ratio rule of the MST's filter would drop that pair),
    and four strangers.  Scattered by a permutation.  Returns ascending arrays of distinct hashes of the width's type."""
    rng = np.random.default_rng(seed)
    dt = np.uint64 if width == 8 else np.uint32
    top = (1 << 62) if width == 8 else (1 << 31)
    shared = rng.choice(top, size=pool, replace=False)
    out = []
    for f in range(n_families):
        own = rng.choice(top, size=pool, replace=False)
        for _ in range(per_family):
            take = int(rng.integers(120, 301))
            out.append(np.concatenate([rng.choice(own, size=take, replace=False), rng.choice(shared, size=take // 10, replace=False)]))
    out.append(np.zeros(0, dtype=np.int64))
    out.append(rng.choice(out[0], size=12, replace=False))
    for _ in range(4):
        out.append(rng.choice(top, size=int(rng.integers(100, 200)), replace=False))
    order = rng.permutation(len(out)).tolist()
    return [np.unique(np.asarray(out[o]).astype(dt)) for o in order], order.index(n_families * per_family + 1), order.index(0)


def dense_sketches(n=300, seed=9):
    """n u32 sketches that all share hash 1, so the candidate list is the whole triangle and a small edge budget cuts the rows into
    several chunks: seven families by g % 7, each sketch 30 to 70 of its family's 80 hashes and three of its own.  Returns
    (sketches, labels): the family as the label, every eleventh sketch unclustered."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n):
        pool = np.arange(80, dtype=np.uint32) * 13 + 100_000 * (g % 7 + 1)
        own = np.arange(3, dtype=np.uint32) + 10_000_000 + 10 * g
        out.append(np.unique(np.concatenate([[1], rng.choice(pool, size=int(rng.integers(30, 71)), replace=False), own]).astype(np.uint32)))
    labels = np.array([g % 7 for g in range(n)], dtype=np.int32)
    labels[::11] = -1
    return out, labels
