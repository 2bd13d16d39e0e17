"""Sketch sets for the k-NN DBSCAN tests (tests/test_cpu_dbscan_knn.py proves on the restatement that they hold their cases,
tests/test_gpu_dbscan_knn.py runs them on the GPU): rows, k, tied groups and first-shared indices past one wave of 64 lanes.

star_set: every star is a hub and its leaves.  The hub's ascending hash list is a private prefix followed by disjoint chunks,
and every leaf is exactly one chunk, so a leaf's only passer is its hub (never a core point at minPts 3), the hub is a core
point as soon as it keeps two leaves, and a leaf is in the hub's cluster if and only if the hub kept it: the labels show every
hub row's kept set.  A leaf scores width / |hub| against its hub and arrives in the order of its chunk in the hub's list.  By
chunk order a star holds its "early better" leaves (width W + 2), its "worse" ones (W - 2), its "tied" ones (W) and its "late
better" ones (W + 2, the star's highest ids, so they arrive when the heap is full and pop tied entries).  The ids of the
other leaves are shuffled against the chunk order and the hub's id sits in their middle."""
import numpy as np

from tests import refdbscan as R

KMER = 21
EPS = 0.3  # jaccard_min 0.00092: below every leaf's score (about 24 / 3 700 against the largest hub) and its binary32 value
MIN_PTS = 3
W = 24
GAP = 3
KS = (16, 63, 64, 65, 100, 128, 129)
# (private prefix, tied, early better, late better, worse); hub rows of 100, 111, 70, 147, 64 and 16 passers.  The third star
# has 64 leaves at or above the tied score and 6 below it: Q == k at k = 64 with P > k.
STARS = ((0, 100, 0, 0, 0), (63, 100, 6, 5, 0), (64, 59, 3, 2, 6), (65, 129, 10, 8, 0), (130, 64, 0, 0, 0), (0, 12, 2, 2, 0))
# the row-chunk variant: every sketch also holds one hash above all others, so that every pair is a candidate; the leaves are
# wide enough that one common hash fails the predicate at CHUNK_EPS (1 / 161 < t = 0.0075 < 81 / 8 968)
CHUNK_STARS = ((63, 70, 4, 3, 0), (65, 100, 6, 5, 0))
CHUNK_W = 80
CHUNK_EPS = 0.2
CHUNK_SHARED = 0xfffffff0
DECOY_MAX_POSTING = 2


def star_set(seed, stars=STARS, w=W, bridge_w=0, shared=None, decoy=False):
    """(sketches, info).  info: hubs (ids), leaves (per star the (id, kind) in chunk order, kind one of early / worse / tied /
    late), bridges (ids), decoys (ids).  bridge_w: one bridge sketch between consecutive stars, a chunk of that width from each
    of the two hubs, placed last in either hub's list, with ids above every star.  shared: a hash every sketch holds.  decoy:
    one more sketch that holds the first half of every third tied chunk (and hashes of its own), so that max_posting =
    DECOY_MAX_POSTING prunes those hashes and the common counts of those leaves fall."""
    rng = np.random.default_rng(seed)
    sketches, hubs, leaves, bridge_chunks, decoy_hashes = [], [], [], [], []
    for s, (prefix, tied, early, late, worse) in enumerate(stars):
        cursor = 1000 + 2_000_000 * s + int(rng.integers(0, 1000))
        hub = [np.arange(cursor, cursor + prefix)]
        cursor += prefix + GAP
        chunks = []
        for kind, count, width in (("early", early, w + 2), ("worse", worse, w - 2), ("tied", tied, w), ("late", late, w + 2)):
            for j in range(count):
                chunks.append((kind, np.arange(cursor, cursor + width)))
                if decoy and kind == "tied" and j % 3 == 0:
                    decoy_hashes.append(chunks[-1][1][:width // 2])
                cursor += width + GAP
        ends = []
        for _ in range(((s > 0) + (s + 1 < len(stars))) if bridge_w else 0):
            ends.append(np.arange(cursor, cursor + bridge_w))
            cursor += bridge_w + GAP
        bridge_chunks.append(ends)
        hub = np.concatenate(hub + [c for _, c in chunks] + ends)
        body = [i for i, (kind, _) in enumerate(chunks) if kind != "late"]
        body = [body[i] for i in rng.permutation(len(body))]
        order = body[:len(body) // 2] + [-1] + body[len(body) // 2:] + [i for i, (kind, _) in enumerate(chunks) if kind == "late"]
        first = len(sketches)
        ids = {}
        for pos, i in enumerate(order):
            if i < 0:
                hubs.append(first + pos)
                sketches.append(hub)
            else:
                ids[i] = first + pos
                sketches.append(chunks[i][1])
        leaves.append([(ids[i], kind) for i, (kind, _) in enumerate(chunks)])
    bridges = []
    for s in range(len(stars) - 1 if bridge_w else 0):
        bridges.append(len(sketches))
        sketches.append(np.concatenate([bridge_chunks[s][-1], bridge_chunks[s + 1][0]]))
    decoys = []
    if decoy:
        decoys.append(len(sketches))
        sketches.append(np.concatenate(decoy_hashes + [np.arange(500_000_000, 500_000_030)]))
    if shared is not None:
        sketches = [np.concatenate([x, [shared]]) for x in sketches]
    out = [np.unique(x).astype(np.uint32) for x in sketches]
    assert all(len(a) == len(b) for a, b in zip(out, sketches))
    return out, {"hubs": hubs, "leaves": leaves, "bridges": bridges, "decoys": decoys}


def bridged_star_set(seed, low=False):
    """star_set with a bridge between consecutive stars: two neighbours, so a core point at minPts 3, and the only way a
    cluster number gets from one hub to the next.  The default bridge (chunks of W + 4) scores above every leaf, so both hubs
    keep it for every k >= 2, and it heads either hub's row sorted by score.  low: chunks of W - 4, which score below every
    leaf; a hub keeps it only where k does not cut its row, and then it is the last record of the sorted row, past position
    64."""
    return star_set(seed, bridge_w=W - 4 if low else W + 4)


def chunk_star_set(seed):
    return star_set(seed, stars=CHUNK_STARS, w=CHUNK_W, shared=CHUNK_SHARED)


def row_shape(arrivals, k):
    """Of one row's passers in arrival order: (P, G, Q, h, |E|) -- passers, those above s*, those at or above it, the passers
    above s* that arrive after the k-th at or above it, the tied ones within the first k at or above it.  G = Q = P and h = |E|
    = 0 for a row of at most k passers."""
    P = len(arrivals)
    if P <= k:
        return P, P, P, 0, 0
    s_star = sorted((s for _, s in arrivals), reverse=True)[k - 1]
    at_or_above = [s for _, s in arrivals if s >= s_star]
    G = sum(s > s_star for s in at_or_above)
    return P, G, len(at_or_above), sum(s > s_star for s in at_or_above[k:]), sum(s == s_star for s in at_or_above[:k])


def first_shared_index(sketches, p, c, max_posting=0):
    """The smallest index in p's list (pruned when max_posting > 0) of a hash that c holds: the arrival key of c in row p"""
    hp = sketches[p]
    if max_posting > 0:
        kept = R.kept_hashes(sketches, max_posting)
        hp = np.asarray([h for h in hp.tolist() if h in kept], dtype=np.uint32)
    return int(np.flatnonzero(np.isin(hp, sketches[c]))[0])


# (|a|, |b|, common): float32(common / union) < common / union, so some jaccard_min lies between the two
FLOAT_PAIRS = ((117, 126, 14), (175, 201, 170), (261, 93, 17), (51, 81, 10))


def float_boundary_pairs():
    return FLOAT_PAIRS


def float_boundary_eps(a, b, c, kmer_size=KMER):
    """An eps whose t = jaccard_min(eps) has float32(c / u) < t <= c / u, u = a + b - c: the pair passes the predicate in
    doubles and its binary32 score fails (double)score >= t."""
    u = a + b - c
    exact, single = c / u, float(np.float32(c) / np.float32(u))
    assert single < exact
    lo, hi = 0.0, 4.0  # t falls with eps
    for _ in range(200):
        mid = (lo + hi) / 2
        t = R.jaccard_min(mid, kmer_size)
        if t > exact:
            lo = mid
        elif t <= single:
            hi = mid
        else:
            return mid
    raise AssertionError("no eps between the binary32 and the binary64 score of %r" % ((a, b, c),))


def float_boundary_sketches(a, b, c):
    x = np.arange(1000, 1000 + a)
    return [x.astype(np.uint32), np.concatenate([x[:c], np.arange(1_000_000, 1_000_000 + b - c)]).astype(np.uint32)]


SATURATED_EPS = 0.005  # jaccard_min 0.82, below every score of the set, capped or not


def saturated_choice_set():
    """x: 70 000 hashes; y: 68 000 of them and 2 000 of its own; z: the last 66 000 of x.  With exact counts x scores 68 000 /
    72 000 = 0.9444 against y and 66 000 / 70 000 = 0.9429 against z; with counts capped at 65 535 it scores 65 535 / 74 465 =
    0.880 against y and 65 535 / 70 465 = 0.930 against z.  At k = 1 and minPts 2 the capped lists are x -> z, y -> z (64 000
    common, 0.889, against 0.880 for x), z -> x: labels 0, 1, 0.  The exact ones are x -> y, y -> x, z -> x: labels 0, 0, 1."""
    x = np.arange(0, 70_000)
    y = np.concatenate([x[:68_000], np.arange(700_000, 702_000)])
    z = x[4_000:]
    return [s.astype(np.uint32) for s in (x, y, z)]
