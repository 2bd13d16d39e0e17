"""Inputs of the rtc_mcl tests (tests/test_cpu_mcl.py proves on the restatement that they hold their cases,
tests/test_gpu_mcl.py and tests/test_gpu_mcl_turns.py run them on the GPU).  Every set is (n, records, S): records a list of (u, v, q), q in units of 2^-20,
S the selection size the set is meant for."""
import numpy as np

UNIT = 1 << 20

_CACHE = {}


def clique(vs, q):
    vs = list(vs)
    return [(a, b, q) for i, a in enumerate(vs) for b in vs[i + 1:]]


def empty():
    return 5, [], 1024


def one_edge():
    return 2, [(0, 1, UNIT)], 1024


def path9(decreasing=False):
    return 9, [(i, i + 1, UNIT - (i * 40000 if decreasing else 0)) for i in range(8)], 1024


def chain_s1():
    """A path of 6 at S = 1: a column keeps its one largest entry, among equals the lowest row, so column j starts as row j - 1
    alone and after t iterations holds row max(j - 2^t, 0).  Stopped early, the upper columns name a row that is no attractor:
    the cluster rule's second case."""
    return 6, [(i, i + 1, UNIT) for i in range(5)], 1


def ring40():
    return 40, [(i, (i + 1) % 40, UNIT) for i in range(40)], 1024


def two_cliques():
    """two 6-cliques of weight 0.9 and a bridge of 0.3"""
    return 12, clique(range(6), 943718) + clique(range(6, 12), 943718) + [(5, 6, 314573)], 1024


def tied_clique(S):
    """30 vertices, every pair at the same weight: which rows a column keeps is decided by the index alone"""
    return 30, clique(range(30), UNIT // 2), S


def hub_star(S=8):
    """a centre, vertex 0, with 20 leaves -- more than S -- whose weights come from 7 values, so the start matrix is cut
    among equals; leaf pairs (i, i + 1), odd i < 12, tied by a light edge"""
    return 21, [(0, i, UNIT // 2 + (i * 7919) % 7) for i in range(1, 21)] + [(i, i + 1, UNIT // 8) for i in range(1, 12, 2)], S


def duplicates():
    """two layers on a 4-clique, self records, a pair in both orientations and a triangle"""
    return 9, (clique(range(4), 10 * UNIT // 16) + clique(range(4), 7 * UNIT // 16) +
               [(4, 4, 50), (4, 5, 9 * UNIT // 16), (5, 4, 9 * UNIT // 16), (5, 6, UNIT // 2), (6, 7, UNIT // 2), (7, 5, UNIT // 2),
                (3, 4, UNIT // 16), (8, 8, 4), (0, 0, 3)]), 1024


# name: (families, members, S, the generator's seed).  The seeds are those at which the restatement reaches an exact fixed point
# after the iteration counts of FAMILY_ITERATIONS (inflation 1.5, 2, 2.5) with every family whole.
FAMILY_SETS = {"families_12x15": (12, 15, 1024, 1403), "families_12x15_s8": (12, 15, 8, 1401), "families_6x40_s16": (6, 40, 16, 10949),
               "families_3x150_s64": (3, 150, 64, 1478)}
FAMILY_ITERATIONS = {"families_12x15": (24, 15, 12), "families_12x15_s8": (20, 13, 11), "families_6x40_s16": (20, 15, 11),
                     "families_3x150_s64": (26, 16, 12)}


def families(name):
    """n_fam families of `per` vertices numbered family after family: an edge inside a family with probability 0.8 and a weight
    in [0.90, 0.98], an edge across with probability 0.01 and a weight in [0.75, 0.80]"""
    if name not in _CACHE:
        n_fam, per, S, seed = FAMILY_SETS[name]
        rng = np.random.default_rng(seed)
        n = n_fam * per
        rec = []
        for x in range(n):
            for y in range(x + 1, n):
                if x // per == y // per:
                    if rng.random() < 0.8:
                        rec.append((x, y, int(round(float(rng.uniform(0.90, 0.98)) * UNIT))))
                elif rng.random() < 0.01:
                    rec.append((x, y, int(round(float(rng.uniform(0.75, 0.80)) * UNIT))))
        _CACHE[name] = (n, rec, S)
    return _CACHE[name]


def family_of(name):
    n_fam, per, _, _ = FAMILY_SETS[name]
    return [(x // per) * per for x in range(n_fam * per)]


def _arms(extra):
    """(a, b) with 3 a + 4 b == extra"""
    for b in range(3):
        if extra >= 4 * b and (extra - 4 * b) % 3 == 0:
            return (extra - 4 * b) // 3, b
    raise ValueError(extra)


def boundary(B):
    """Three components, one per W in (B - 1, B, B + 1).  A component is a clique of c members, a probe vertex tied to all of
    them, a leaves on the probe and b more leaves on it that carry a leaf of their own.  In the start matrix a member's
    column has c + 1 entries, a leaf's 2, a leaf with a leaf 3 and the probe's c + a + b + 1, so the probe's column gathers
    W = c (c + 2) + 3 a + 4 b + 1 products in the first iteration.  The weights differ so that no two columns are alike."""
    if ("boundary", B) not in _CACHE:
        c = 2
        while (c + 1) * (c + 3) + 1 + 6 <= B - 1:
            c += 1
        rec, probes, at = [], [], 0
        for W in (B - 1, B, B + 1):
            a, b = _arms(W - c * (c + 2) - 1)
            members = list(range(at, at + c))
            probe = at + c
            at = probe + 1
            for i, x in enumerate(members):
                for y in members[i + 1:]:
                    rec.append((x, y, UNIT - 1000 * ((x + 3 * y) % 17)))
                rec.append((probe, x, UNIT // 2 + 100 * i))
            for t in range(a + b):
                rec.append((at, probe, UNIT // 4 + 50 * t))
                if t >= a:
                    rec.append((at, at + 1, UNIT // 8))
                    at += 1
                at += 1
            probes.append(probe)
        _CACHE[("boundary", B)] = (at, rec, 4096), probes
    return _CACHE[("boundary", B)]


def summed(total):
    """one pair whose records, in both orientations, sum to `total`"""
    return 3, [(0, 1, total - 5), (1, 0, 4), (0, 1, 1), (1, 2, UNIT)], 1024


def hand_sets():
    return {"empty": empty(), "one_edge": one_edge(), "path9_equal": path9(), "path9_decreasing": path9(True), "ring40": ring40(), "chain_s1": chain_s1(),
            "two_cliques": two_cliques(), "tied_clique_s8": tied_clique(8), "tied_clique_s64": tied_clique(64), "hub_star_s8": hub_star(),
            "duplicates": duplicates(), "summed_2_32_less_1": summed((1 << 32) - 1)}


def all_sets(boundaries):
    out = hand_sets()
    for name in FAMILY_SETS:
        out[name] = families(name)
    for B in boundaries:
        out["boundary_%d" % B] = boundary(B)[0]
    return out


def constants():
    """every `constexpr uint32_t NAME = value;` of the kernel's header"""
    if "constants" not in _CACHE:
        import os
        import re
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        text = open(os.path.join(root, "rabbittclust_amd", "csrc", "rtc_mcl.h")).read()
        _CACHE["constants"] = {name: int(value) for name, value in re.findall(r"constexpr uint32_t (\w+) = (\d+)u?;", text)}
    return _CACHE["constants"]


def boundaries():
    """(MCL_WAVE_WORK, MCL_BLOCK_WORK) as the kernel's header has them"""
    return constants()["MCL_WAVE_WORK"], constants()["MCL_BLOCK_WORK"]


def grids(num_cu, n):
    """the workgroups of the start launch and of the wave, workgroup and global column launches on a device of num_cu CUs: a
    list of more columns than that gives some workgroup a second turn of its loop"""
    c = constants()
    return tuple(min(n, num_cu * c[name]) for name in ("MCL_START_WGS_PER_CU", "MCL_WAVE_WGS_PER_CU", "MCL_BLOCK_WGS_PER_CU", "MCL_GLOBAL_WGS_PER_CU"))


def every_set():
    return all_sets(boundaries())


HIGH_INFLATION_SETS = ("two_cliques", "tied_clique_s8", "families_12x15_s8", "hub_star_s8")  # run at inflation 3 to 8 as well


# ---- the sets that take a workgroup past its first column (tests/test_gpu_mcl_turns.py), kept out of every_set() ----
CUS = 256  # the compute units of an MI355X: the sets are sized for its grids, and the GPU test asks the device it runs on
TURNS_N = 10240


def home(i, log2_slots):
    """row i's home slot in a table of 2^log2_slots slots: MclTable's hash"""
    return ((i * constants()["MCL_GOLDEN"]) & 0xffffffff) >> (32 - log2_slots)


def probe_fill(rows, log2_slots):
    """{slot: row} after the rows claimed their slots by linear probing (the set of taken slots does not depend on the order)"""
    slots, mask = {}, (1 << log2_slots) - 1
    for i in rows:
        s = home(i, log2_slots)
        while s in slots:
            s = (s + 1) & mask
        slots[s] = i
    return slots


def wrap_ids(n=TURNS_N):
    """(12 ids below n whose home is one of the last 4 of MCL_WAVE_SLOTS = 512 slots -- and so one of the last 8 of 1024 --,
    18 ids whose home is one of the last 8 of MCL_BLOCK_SLOTS = 4096 slots): as cliques, a column of the first gathers 144
    products in 12 rows on the wave path, a column of the second 324 in 18 rows on the workgroup path, and the probe chains
    run off the last slot to slot 0"""
    c = constants()
    wave_log2, block_log2 = c["MCL_WAVE_SLOTS"].bit_length() - 1, c["MCL_BLOCK_SLOTS"].bit_length() - 1
    block = [i for i in range(n) if home(i, block_log2) >= c["MCL_BLOCK_SLOTS"] - 8][:18]
    wave = [i for i in range(n) if home(i, wave_log2) >= c["MCL_WAVE_SLOTS"] - 4 and i not in block][:12]
    return wave, block


def turns_10k(S, n=TURNS_N):
    """n vertices: the two wrap cliques on the ids of wrap_ids(), and on the other ids, in a fixed random order, 50 cliques
    of 20 (weights in [0.9, 1): W = 400, the workgroup path), a hub with 160 leaves and one with 60 (from the second iteration
    every column of theirs gathers 161^2 and 61^2 products: the global path at 32768 and at 8192 slots), paths of 5 with
    weights in [0.5, 1) (the wave path) and the last few vertices without an edge."""
    if ("turns_10k", S, n) not in _CACHE:
        rng = np.random.default_rng(20261)
        wave, block = wrap_ids(n)
        rest = sorted(set(range(n)) - set(wave) - set(block))
        rest = [rest[i] for i in rng.permutation(len(rest)).tolist()]
        q = lambda lo, hi: int(round(float(rng.uniform(lo, hi)) * UNIT))
        rec = []
        for vs in (wave, block):
            rec += [(a, b, q(0.9, 1.0)) for a, b, _ in clique(vs, 0)]
        at = 0
        for _ in range(50):
            rec += [(a, b, q(0.9, 1.0)) for a, b, _ in clique(rest[at:at + 20], 0)]
            at += 20
        for leaves in (160, 60):
            rec += [(rest[at], x, q(0.5, 1.0)) for x in rest[at + 1:at + 1 + leaves]]
            at += leaves + 1
        for _ in range((len(rest) - at) // 5):
            rec += [(rest[at + i], rest[at + i + 1], q(0.5, 1.0)) for i in range(4)]
            at += 5
        _CACHE[("turns_10k", S, n)] = (n, rec, S)
    return _CACHE[("turns_10k", S, n)]


HUB_300 = 150


def hub_300(S):
    """a centre, vertex HUB_300, with 300 leaves whose weights come from 7 values: its column has 301 keys, more than the 256
    lanes of mcl_start_kernel take in one turn, cut among equals at S = 64 and whole at S = 1024"""
    return 301, [(HUB_300, i, UNIT // 2 + (i * 7919) % 7) for i in range(301) if i != HUB_300], S


def turn_sets():
    return {"turns_10k": turns_10k(1024), "turns_10k_s8": turns_10k(8), "hub_300_s64": hub_300(64), "hub_300_s1024": hub_300(1024)}


def _trajectory(name, h, sets, upto):
    key = ("trajectory", name, h)
    from tests import refmcl
    n, rec, S = (sets or every_set())[name]
    if key not in _CACHE:
        _CACHE[key] = {"mats": [refmcl.start(n, rec, S)], "converged": 0, "cuts": [sum(len(a) + 1 > S for a in refmcl.adjacency(n, rec))]}
    t = _CACHE[key]
    while len(t["mats"]) <= min(upto, 100) and not t["converged"]:
        N, cut = refmcl.iterate_counting(t["mats"][-1], h, S)
        t["mats"].append(N)
        t["cuts"].append(cut)
        t["converged"] = int(t["mats"][-1] == t["mats"][-2])
    return t


def trajectory(name, h, sets=None, upto=100):
    """The restatement's matrices of a set at inflation h / 2: [start, after iteration 1, ...] up to the fixed point (or 100
    iterations, or `upto` of them if that is fewer), and whether it converged.  Computed once, and lengthened when a later
    call asks for more; nobody changes a matrix."""
    t = _trajectory(name, h, sets, upto)
    return t["mats"], t["converged"]


def expected(name, h, T, sets=None):
    """what rtc_mcl returns for the set at max_iter = T: (labels, iterations, converged, entries)"""
    from tests import refmcl
    mats, converged = trajectory(name, h, sets, upto=T)
    its = min(T, len(mats) - 1)
    M = mats[its]
    return refmcl.clusters(M), its, int(bool(converged) and its == len(mats) - 1), refmcl.entries(M)


def cuts(name, h, T, sets=None):
    """the columns that select cut in a call at max_iter = T: those of the start matrix with more than S entries and those of
    every iteration with more than S rows alive after the inflation"""
    t = _trajectory(name, h, sets, T)
    return sum(t["cuts"][:min(T, len(t["mats"]) - 1) + 1])


def work(M):
    """W of every column: the products its expansion gathers"""
    return [sum(len(M[k]) for k in col) for col in M]


def path_counts(M):
    """the columns that the iteration from matrix M sends to the (wave, workgroup, global) path"""
    wave, block = boundaries()
    W = work(M)
    return sum(w <= wave for w in W), sum(wave < w <= block for w in W), sum(w > block for w in W)


def table_log2(W, n, S):
    """log2 of the slots a column of work W takes of its global table: mcl_column_kernel's rule under rtc_mcl's gtab_log2"""
    low = constants()["MCL_GLOBAL_LOG2_MIN"]
    stride = min(S, n)
    gtab = low
    while gtab < 31 and (1 << gtab) < 2 * min(stride * stride, n):
        gtab += 1
    log2 = low
    while log2 < gtab and (1 << log2) < 2 * min(W, n):
        log2 += 1
    return log2


def shuffled(records, seed=7):
    rng = np.random.default_rng(seed)
    out = [records[i] for i in rng.permutation(len(records)).tolist()]
    return [(v, u, q) if i % 3 == 0 else (u, v, q) for i, (u, v, q) in enumerate(out)]
