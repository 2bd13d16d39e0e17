"""The inputs the rtc_graph_snn tests share: name -> (n, records), records (u, v).  expected(name) is tests/refsnn.py's answer,
computed once."""
import functools
import os
import random
import re

from tests import refsnn as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants():
    """every constexpr uint32_t of rabbittclust_amd/csrc/rtc_snn.h"""
    text = open(os.path.join(ROOT, "rabbittclust_amd", "csrc", "rtc_snn.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr uint32_t (\w+) = (\d+)u?;", text)}


def boundaries():
    c = constants()
    return c["SNN_WAVE_ROW"], c["SNN_BLOCK_ROW"]


def clique(ids):
    ids = list(ids)
    return [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]


# ---- the cases on paper ----
def single_edge():
    return 2, [(0, 1)]


def path3():
    return 3, [(0, 1), (1, 2)]


def triangle():
    return 3, clique(range(3))


def k5():
    return 5, clique(range(5))


def star70():
    return 71, [(0, leaf) for leaf in range(1, 71)]


def two_k40():
    return 80, clique(range(40)) + clique(range(40, 80)) + [(39, 40)]


# ---- records as a file may hold them ----
def messy():
    """reversed, duplicated, a self loop on a vertex with neighbours and one on a vertex without, and vertex 7 that no record names"""
    return 9, [(0, 1), (1, 0), (0, 1), (2, 1), (0, 2), (2, 2), (3, 2), (2, 3), (4, 3), (5, 5), (6, 8), (8, 6), (3, 0)]


def random_graph(seed):
    """300 vertices, each naming 1 to 40 others"""
    rng = random.Random(seed)
    rec = []
    for x in range(300):
        for y in rng.sample([y for y in range(300) if y != x], rng.randint(1, 40)):
            rec.append((x, y) if rng.random() < 0.5 else (y, x))
    rng.shuffle(rec)
    return 300, rec


def k130():
    return 130, clique(range(130))


def k65_65():
    return 130, [(a, 65 + b) for a in range(65) for b in range(65)]


def hub(row):
    """vertex 0 joined to all vertices of row // 5 disjoint K5 -- every such edge has shared = 4 -- and to row % 5 leaves of its
    own (shared = 0), which bring its row to `row` entries exactly"""
    rec = [(0, x) for x in range(1, row + 1)]
    for c in range(row // 5):
        rec += clique(range(1 + 5 * c, 6 + 5 * c))
    return row + 1, rec


PAPER = {"single_edge": single_edge, "path3": path3, "triangle": triangle, "k5": k5, "star70": star70, "two_k40": two_k40}
# the weight of every edge of the case, or of the named one
PAPER_WEIGHTS = {"single_edge": (1, 1), "path3": (2, 3), "triangle": (1, 1), "k5": (1, 1), "star70": (2, 71)}


def hub_rows():
    wave, block = boundaries()
    return (wave, wave + 1, block, block + 1)


def hub_path(row):
    """the paths a hub set takes: the K5 edges one wave, the hub's edges by its row"""
    wave, block = boundaries()
    return 1 | (1 if row <= wave else 2 if row <= block else 4)


@functools.lru_cache(maxsize=None)
def every_set():
    sets = {name: make() for name, make in PAPER.items()}
    sets["messy"] = messy()
    for seed in (1, 2, 3):
        sets["random_%d" % seed] = random_graph(seed)
    sets["k130"] = k130()
    sets["k65_65"] = k65_65()
    for row in hub_rows():
        sets["hub_%d" % row] = hub(row)
    return sets


@functools.lru_cache(maxsize=None)
def expected(name):
    n, rec = every_set()[name]
    return R.snn(n, rec)


@functools.lru_cache(maxsize=None)
def expected_counters(name):
    """(distinct edges, triangles, probes, records with u != v)"""
    n, rec = every_set()[name]
    return len(R.edges(n, rec)), R.triangles(n, rec), R.probes(n, rec), sum(1 for u, v in rec if u != v)


def expected_paths(name):
    """records on the wave / workgroup / global path"""
    n, rec = every_set()[name]
    wave, block = boundaries()
    rows = R.longer_rows(n, rec)
    return sum(r <= wave for r in rows), sum(wave < r <= block for r in rows), sum(r > block for r in rows)
