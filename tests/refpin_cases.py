"""The inputs of the reference pin (tests/golden/ref_dbscan.npz, ref_postprocess.npz): seeded generators of sketch sets and
forests, and the grids of parameters the reference's own KssdDBSCAN / build_dedup_candidates_per_cluster /
select_k_reps_per_cluster_tree were run on.  tests/golden/make_golden.py records the reference's results for these cases;
tests/test_cpu_refpin.py and tests/test_gpu_refpin.py rebuild the inputs here and compare.  The generators only make inputs;
gen_kssd_family takes its genomes and sketches from the CPU oracle and the package's family descriptors, and the fixture
pins every input set by SHA-256."""
import hashlib
import json
import math

import numpy as np

from tests import sweep_sets

KMER = 22
INT_MAX = 2 ** 31 - 1


def jaccard_min(eps, k):
    x = math.exp(-eps * k)
    return x / (2.0 - x)


def _block(base, m):
    return np.arange(base, base + m, dtype=np.uint64)


# ---- sketch sets ----
def gen_family(seed, use64, n_empty):
    return sweep_sets.family_sets(seed, use64, n_empty=n_empty)


def gen_hand(use64):
    """tests/test_gpu_dbscan.py's hand-built set: two chains of sliding windows, point 6 a border point of both clusters at
    minPts 4, point 0 labelled noise first and absorbed later, 13 and 15 empty, 14 alone"""
    def win(i, base):
        return _block(base + 25 * i, 100)
    sk = [win(i, 0) for i in range(6)] + [np.concatenate([_block(175, 50), _block(100_000, 50)])]
    sk += [win(i, 100_000) for i in range(6)] + [_block(0, 0), _block(50_000, 80), _block(0, 0)]
    return [s.astype(np.uint64 if use64 else np.uint32) for s in sk]


SAT_A, SAT_C = 70_000, 68_000


def gen_saturation(use64):
    """two sketches of 70 000 hashes sharing 68 000: past the 65 535 a u16 counter holds"""
    x = _block(0, SAT_A)
    y = np.concatenate([x[:SAT_C], _block(10 * SAT_A, SAT_A - SAT_C)])
    return [v.astype(np.uint64 if use64 else np.uint32) for v in (x, y)]


def saturation_eps():
    """(eps where 68 000 common passes and 65 535 fails, a smaller eps where both fail, a larger one where both pass)"""
    a, c = SAT_A, SAT_C

    def ok(common, e):
        t = jaccard_min(float(e), KMER)
        return not (common * (1.0 + t) + 1e-12 < t * a + t * a)
    grid = [float(e) for e in np.linspace(0.0005, 0.05, 400)]
    flip = next(e for e in grid if ok(c, e) and not ok(65535, e))
    below = max(e for e in grid if not ok(c, e))
    above = next(e for e in grid if ok(65535, e))
    return flip, below, above


def saturation_edge_eps():
    """the eps whose accept boundary for two sketches of SAT_A hashes lies at 65 535.5 common hashes: a count that stops at
    65 535 fails, one that reaches 65 536 would pass"""
    ts = 65535.5 / (2 * SAT_A - 65535.5)
    eps = -math.log(2.0 * ts / (1.0 + ts)) / KMER
    t = jaccard_min(eps, KMER)
    assert 65535 * (1.0 + t) + 1e-12 < t * SAT_A + t * SAT_A and not (65536 * (1.0 + t) + 1e-12 < t * SAT_A + t * SAT_A)
    return eps


HUB_POINTS = 10_400  # the hub touches this many points: past the reference's parallel evaluation threshold of 10 000
HUB_EPS = 0.35


def gen_hub():
    """One hub sketch holding HUB_POINTS + 1099 hashes, and HUB_POINTS small sketches that each hold a hub hash of their own:
    the hub's posting scan touches all of them, every other point touches few.  Every 40th small sketch holds four hub
    hashes and is the hub's neighbour at HUB_EPS (t = 2.3e-4: 4 (1 + t) >= t (11 499 + 9) = 2.6), the others are not (1 + t).
    The small sketches come in families of three sharing five hashes, every 7th family is a single point."""
    m = HUB_POINTS
    hub = np.arange(1, m + 1100, dtype=np.uint64)
    out = [hub]
    for i in range(m):
        fam = i // 3
        own = [1 + i] + ([1 + m + (i % 997) + 3 * j for j in range(3)] if i % 40 == 0 else [])
        body = _block(10_000_000 + 100 * fam, 5) if fam % 7 else _block(20_000_000 + 100 * i, 5)
        out.append(np.unique(np.concatenate([np.array(own, dtype=np.uint64), body])))
    return [s.astype(np.uint32) for s in out]


def near_tie_eps(a, b, c, k):
    """eps values on both sides of the 1e-12 tolerance for sizes a, b sharing c: tests/test_gpu_dbscan.py's own search"""
    from tests.test_gpu_dbscan import _near_tie
    return _near_tie(a, b, c, k)


NEAR_TIES = [(1000, 1000, 700), (1000, 900, 612), (333, 517, 250)]


def gen_near_tie(a, b, c, use64):
    x = _block(0, a)
    y = np.concatenate([x[:c], _block(10 * (a + b), b - c)])
    return [v.astype(np.uint64 if use64 else np.uint32) for v in (x, y)]


def gen_sizes(sizes, use64):
    """nested sketches arange(s): any two share the smaller one whole"""
    return [np.arange(s, dtype=np.uint64 if use64 else np.uint32) for s in sizes]


def gen_row_chunks():
    """tests/test_gpu_dbscan.py's row-chunk set: 600 sketches that all share one hash, so the candidate list is the whole
    triangle and a small edge budget cuts it into row chunks"""
    n = 600
    rng = np.random.default_rng(3)
    sets = []
    for g in range(n):
        body = _block(100_000 * (g % 7), 60)[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, _block(10_000_000 + 1000 * g, 5)])))
    return [np.asarray(x, dtype=np.uint32) for x in sets]


def gen_lists(sets, use64):
    return [np.array(sorted(x), dtype=np.uint64 if use64 else np.uint32) for x in sets]


def gen_kssd_family(seed, n_fam, per, L, k, drlevel):
    """the KSSD sketches of synthetic genome families as tests/test_gpu_dbscan.py's _family_sketches makes them on the GPU,
    here from the CPU oracle (the sketch kernel is held to it elsewhere)"""
    from oracle import pyoracle as O
    from rabbittclust_amd import api
    desc = api.synth_family_descs(n_fam, per, global_seed=seed)
    return [O.kssd_sketch(O.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), L), k, drlevel) for d in desc]


def random_set(seed):
    """a seeded random sketch set for the live sweep: 1-80 points in families (a base of 0-400 hashes, members with
    substitutions at the family's rate and a random share of the base kept), with single points and empty sketches mixed in,
    in shuffled order; and the parameters to run it with: (sketches, use64, eps, minPts, kmer size, max_posting, threads)"""
    rng = np.random.default_rng(50_000 + seed)
    use64 = seed % 2 == 1
    n = int(rng.integers(1, 81))
    out = []
    while len(out) < n:
        members = int(rng.integers(1, 9))
        size = int(rng.integers(0, 401))
        rate = float(rng.choice([0.02, 0.1, 0.3, 0.6]))
        base = rng.integers(1, (1 << 31) - 1, size=size, dtype=np.int64)
        for _ in range(members):
            s = base.copy()
            flip = rng.random(size) < rate
            s[flip] = rng.integers(1, (1 << 31) - 1, size=int(flip.sum()), dtype=np.int64)
            out.append(s[rng.random(size) < rng.uniform(0.5, 1.0)] if rng.random() < 0.5 else s)
    out = [out[i] for i in rng.permutation(len(out))[:n]]
    sk = [np.unique(s).astype(np.uint64 if use64 else np.uint32) for s in out]
    eps = float(rng.choice([0.005, 0.02, 0.05, 0.1, 0.2]))
    return (sk, use64, eps, int(rng.choice([1, 2, 3, 4, 6])), int(rng.choice([17, 21, 22])),
            0 if use64 else int(rng.choice([0, 0, 2, 5, 50])), int(rng.choice([1, 4])))


GENERATORS = dict(family=gen_family, hand=gen_hand, saturation=gen_saturation, hub=gen_hub, near_tie=gen_near_tie,
                  sizes=gen_sizes, lists=gen_lists, row_chunks=gen_row_chunks, kssd_family=gen_kssd_family)
_cache = {}


def sketches_of(gen, args):
    key = json.dumps([gen, args], sort_keys=True)
    if key not in _cache:
        _cache[key] = GENERATORS[gen](**args)
    return _cache[key]


def input_sha(sketches):
    h = hashlib.sha256()
    for s in sketches:
        h.update(np.array([len(s), s.dtype.itemsize], dtype="<u8").tobytes())
        h.update(np.ascontiguousarray(s).tobytes())
    return h.hexdigest()


def use64_of(sketches):
    return sketches[0].dtype.itemsize == 8


# the sketch sets of tests/test_gpu_dbscan.py that come from the sketch kernel: (seed, n_fam, per, L, k, drlevel)
KSSD_FAMILIES = [dict(seed=s, n_fam=6, per=5, L=400_000, k=21, drlevel=3) for s in (1, 2, 3)]
KSSD_FAMILY_U64 = dict(seed=11, n_fam=4, per=4, L=300_000, k=25, drlevel=3)
KSSD_FAMILY_POSTING = dict(seed=5, n_fam=5, per=4, L=300_000, k=21, drlevel=3)
ROW_CHUNKS = ("row_chunks", {}, 0.1, 4, KMER, 0)
# the genomes of tests/test_gpu_dbscan.py's command line test, sketched at -k 17; CLI_RUNS: (eps, minPts, -l layout)
KSSD_FAMILY_CLI = dict(seed=9, n_fam=4, per=4, L=1_000_000, k=17, drlevel=3)
CLI_RUNS = [(0.03, 2, True), (0.05, 3, False)]
FAMILY_EPS = (0.01, 0.02, 0.03, 0.05, 0.1)
FAMILY_MINPTS = (1, 2, 5, 50)
# One step inside / outside the u32 size bound at eps 0.9, k 22 (t = 1.26e-9, any common hash makes a neighbour):
# ceil(2 / t) <= INT_MAX < ceil(3 / t).  Point 0 shares a hash with each of the others, which share none: at minPts 3 point 0
# is the only core point and all three form one cluster.  Where the bound of a sketch of 3 hashes overflows to a negative int,
# points 0 and 1 find no neighbour at all and point 2 only one: three noise points.
INSIDE_SETS, OUTSIDE_SETS = [[0, 1], [1, 2], [0]], [[0, 1, 2], [2, 3, 4], [0]]
OVERFLOW_SIZES = [3000, 3000, 10, 10]


def dbscan_cases():
    """[(generator, arguments, eps, minPts, kmer size, max_posting)]: the grid of tests/golden/ref_dbscan.npz"""
    out = []
    for seed in (1, 2, 3):
        for use64 in (False, True):
            args = dict(seed=seed, use64=use64, n_empty=2)
            for eps in sweep_sets.EPS:
                for min_pts in (0, 1, 2, 3, 5, 100):  # 100 > n = 34
                    for mp in ((0,) if use64 else (0, 1, 5, 1000)):  # 1000 >= n: prunes nothing
                        out.append(("family", args, eps, min_pts, sweep_sets.KMER, mp))
    for use64 in (False, True):
        for eps in (0.01, 0.04, 0.2):
            for min_pts in (1, 2, 3, 4, 5):
                out.append(("hand", dict(use64=use64), eps, min_pts, KMER, 0))
        for eps in saturation_eps() + (saturation_edge_eps(),):
            out.append(("saturation", dict(use64=use64), eps, 2, KMER, 0))
        for a, b, c in NEAR_TIES:
            for eps in near_tie_eps(a, b, c, KMER):
                out.append(("near_tie", dict(a=a, b=b, c=c, use64=use64), eps, 2, KMER, 0))
    for min_pts in (2, 3, 4):
        out.append(("hub", {}, HUB_EPS, min_pts, KMER, 0))
    for args in KSSD_FAMILIES:
        for eps in FAMILY_EPS:
            for min_pts in FAMILY_MINPTS:
                out.append(("kssd_family", args, eps, min_pts, 22, 0))
    for eps in (0.01, 0.03, 0.08):
        for min_pts in (1, 2, 5):
            out.append(("kssd_family", KSSD_FAMILY_U64, eps, min_pts, 26, 0))
    for mp in (1, 2, 3, 4, 8, 1000):
        out.append(("kssd_family", KSSD_FAMILY_POSTING, 0.05, 2, 22, mp))
    out.append(ROW_CHUNKS)
    for eps, min_pts, _ in CLI_RUNS:
        out.append(("kssd_family", KSSD_FAMILY_CLI, eps, min_pts, 17, 0))
    # the u32 size bound ceil(size / t) at INT_MAX: inside it, one step outside, and the example far outside; and u64
    for use64 in (False, True):
        for eps in (0.6, 0.7, 0.9):
            for min_pts in (2, 3):
                out.append(("lists", dict(sets=INSIDE_SETS, use64=use64), eps, min_pts, KMER, 0))
                out.append(("lists", dict(sets=OUTSIDE_SETS, use64=use64), eps, min_pts, KMER, 0))
                out.append(("sizes", dict(sizes=OVERFLOW_SIZES, use64=use64), eps, min_pts, KMER, 0))
    return out


def case_key(case):
    return json.dumps(list(case), sort_keys=True)


def u32_bound_exceeded(sketches, eps, k):
    """the kernels' refusal (rtc_dbscan_common.h): a u32 set whose largest ceil(size / t) is past INT_MAX"""
    t = jaccard_min(eps, k)
    return (not use64_of(sketches)) and math.ceil(max(len(s) for s in sketches) / t) > INT_MAX


def genomes_of(n, by_file):
    """the names the printed file carries; one total length past 2^31 in the -l layout"""
    if by_file:
        return [("dir/g%05d.fna" % i, 3_000_000_000 if i == 1 else 1000 + 37 * i, "seq%d" % i, "" if i % 5 == 0 else "synthetic member %d" % i)
                for i in range(n)]
    return [("seq%d" % i, 1000 + 37 * i, "" if i % 5 == 0 else "synthetic member %d" % i) for i in range(n)]


def cli_genomes(by_file):
    """what clust-dbscan's output names for KSSD_FAMILY_CLI's genomes written as g000.fna ... (one record each) and listed by
    relative path, or as the records r0 ... of one file"""
    a = KSSD_FAMILY_CLI
    n = a["n_fam"] * a["per"]
    if by_file:
        return [("g%03d.fna" % g, a["L"], "g%d" % g, "synthetic family %d" % (g // a["per"])) for g in range(n)]
    return [("r%d" % g, a["L"], "member %d" % g) for g in range(n)]


def print_layout(index):
    return index % 2 == 0


# ---- forests for the post-processing ----
def forest_case(seed):
    """a seeded forest: (n, edges [(a, b, w)], lens, dedup distances, k values).  Shapes: chains, stars, caterpillars, random
    trees; weights tied (few values, 0 included) or distinct; lengths equal, few-valued or distinct; some trees are joined by
    edges above every dedup distance, some nodes stay alone."""
    rng = np.random.default_rng(1000 + seed)
    n_trees = int(rng.integers(1, 6))
    sizes = [int(rng.integers(1, 40)) for _ in range(n_trees)]
    n = sum(sizes) + int(rng.integers(0, 3))
    ids = rng.permutation(n)
    tied = seed % 2 == 0
    edges, at, heads = [], 0, []
    for t, s in enumerate(sizes):
        nodes = ids[at:at + s]
        shape = ("chain", "star", "caterpillar", "random")[(seed + t) % 4]
        for i in range(1, s):
            if shape == "chain":
                p = i - 1
            elif shape == "star":
                p = 0
            elif shape == "caterpillar":  # a spine of the even positions, a leg on each
                p = i - 2 if i % 2 == 0 and i >= 2 else i - 1
            else:
                p = int(rng.integers(0, i))
            w = float(rng.choice([0.0, 0.005, 0.005, 0.01, 0.015])) if tied else float(rng.random() * 0.02)
            edges.append((int(nodes[i]), int(nodes[p]), w))
        heads.append(int(nodes[0]))
        at += s
    for i in range(1, len(heads)):
        if rng.random() < 0.5:
            edges.append((heads[i], heads[int(rng.integers(0, i))], 0.03 + 0.01 * float(rng.random())))
    order = rng.permutation(len(edges))
    edges = [edges[i] for i in order]
    kind = seed % 3
    lens = ([5000] * n if kind == 0 else rng.choice([1000, 1000, 2000], size=n).tolist() if kind == 1
            else rng.integers(1000, 10 ** 6, size=n).tolist())
    on = edges[len(edges) // 2][2] if edges else 0.01
    dedup = [0.0, 0.005, 0.01, 0.015, 1.0, float(np.nextafter(on, -1.0)), on, float(np.nextafter(on, 2.0))]
    return n, edges, [int(x) for x in lens], dedup, (0, 1, 2, 3, 1000)


def components(n, edges):
    """the forest's connected components, each in breadth-first order from its smallest node (the cluster lists the
    post-processing takes as input)"""
    adj = [[] for _ in range(n)]
    for a, b, _ in edges:
        adj[a].append(b)
        adj[b].append(a)
    seen, out = [False] * n, []
    for i in range(n):
        if seen[i]:
            continue
        seen[i] = True
        comp, head = [i], 0
        while head < len(comp):
            for v in adj[comp[head]]:
                if not seen[v]:
                    seen[v] = True
                    comp.append(v)
            head += 1
        out.append(comp)
    return out


FOREST_SEEDS = range(60)
