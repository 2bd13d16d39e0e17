"""Restatement of the placement rule of rtc_dbscan_assign (include/rtclust.h), brute force: a query against every point of a
clustered set, with the neighbour predicates of tests/refdbscan.py (KSSD, both orientations) and tests/refdbscan_mash.py
(MinHash).  The reference has no such rule; what ties it to the reference is the leave-one-out property that
tests/test_cpu_dbscan_assign.py holds against the compiled KssdDBSCAN.  Also the command line's TSV and the parser of the
model file, both from their documented layout (README)."""
import math
import struct
from fractions import Fraction

import numpy as np

from tests import refdbscan as R
from tests import refdbscan_mash as M

NONE = 0xFFFFFFFF
PLACE_DT = np.dtype([("label", "<i4"), ("label_max", "<i4"), ("n_neighbours", "<u4"), ("n_core", "<u4"), ("nearest", "<u4"),
                     ("common", "<u4"), ("denom", "<u4"), ("flags", "<u4")])


def kssd_pred(a, b, common, t, use64):
    """findNeighborsKSSDWithIndex's test for reference point of size a and candidate of size b (tests/refdbscan.neighbour_lists,
    the evaluation block): the u32 index path skips empty sketches, the u64 brute force has no emptiness test."""
    if not use64 and (a == 0 or b == 0):
        return False
    min_size = math.floor(t * a)
    max_size = math.ceil(float(a) / t)
    if b < min_size or b > max_size:
        return False
    return not (float(common) * (1.0 + t) + 1e-12 < t * float(a) + t * float(b))


def _finish(nbrs, cands, labels, core, would_be_core):
    """the record from N(q) (indices) and the candidates (index, common, denom) that share a hash"""
    core_labels = [int(labels[p]) for p in nbrs if core[p]]
    best = None
    for p, c, d in cands:
        key = Fraction(c, d)
        if best is None or key > best[0]:  # ascending p: equal keys stay with the lower index
            best = (key, p, c, d)
    return (min(core_labels) if core_labels else -1, max(core_labels) if core_labels else -1, len(nbrs), len(core_labels),
            best[1] if best else NONE, best[2] if best else 0, best[3] if best else 0, int(would_be_core))


def place_kssd(model, labels, core, q, eps, min_pts, kmer_size, use64):
    t = R.jaccard_min(eps, kmer_size)
    q = np.asarray(q)
    nbrs, cands = [], []
    for p, s in enumerate(model):
        common = len(np.intersect1d(q, s, assume_unique=True))
        seen = common if use64 else min(common, 65535)  # MarkCnt's u16 count
        fwd, bwd = kssd_pred(len(q), len(s), seen, t, use64), kssd_pred(len(s), len(q), seen, t, use64)
        assert fwd == bwd, ("orientation-dependent pair", p)
        if fwd:
            nbrs.append(p)
        if common:
            cands.append((p, seen, len(q) + len(s) - seen))
    return _finish(nbrs, cands, labels, core, len(nbrs) + 1 >= min_pts)


def place_mash(model, labels, core, q, eps, min_pts, kmer_size, sketch_size):
    q = np.asarray(q)
    nbrs, cands = [], []
    for p, s in enumerate(model):
        if not len(np.intersect1d(q, s, assume_unique=True)):
            continue  # distance 1 > eps
        c, d = M.mash_counts_sets(q, np.asarray(s), sketch_size)
        if M.distance(c, d, kmer_size) <= eps:
            nbrs.append(p)
        cands.append((p, c, d))
    return _finish(nbrs, cands, labels, core, len(nbrs) >= max(min_pts, 0))


def place_all(model, labels, core, queries, eps, min_pts, kmer_size, use64=False, sketch_size=None):
    """PLACE_DT per query: sketch_size None is KSSD, otherwise MinHash with that estimator size"""
    out = np.zeros(len(queries), dtype=PLACE_DT)
    for i, q in enumerate(queries):
        out[i] = (place_kssd(model, labels, core, q, eps, min_pts, kmer_size, use64) if sketch_size is None else
                  place_mash(model, labels, core, q, eps, min_pts, kmer_size, sketch_size))
    return out


def distance(rec, kmer_size, sketch_size=None):
    """what the command line prints for a record's nearest point"""
    if int(rec["nearest"]) == NONE:
        return math.inf
    c, d = int(rec["common"]), int(rec["denom"])
    if sketch_size is not None:
        return M.distance(c, d, kmer_size)
    if c == d:
        return 0.0
    j = float(c) / float(d)
    return -math.log(2.0 * j / (1.0 + j)) / kmer_size


def tsv(names_q, recs, names_db, kmer_size, sketch_size=None):
    """clust-dbscan --db --assign's output"""
    out = ["query\tcluster\tbridges\tneighbours\tcore_neighbours\twould_be_core\tnearest\tdistance\n"]
    for name, r in zip(names_q, recs):
        d = distance(r, kmer_size, sketch_size)
        out.append("%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\n" % (
            name, "novel" if r["label"] < 0 else str(int(r["label"])), int(r["label"] != r["label_max"]), int(r["n_neighbours"]),
            int(r["n_core"]), int(r["flags"]) & 1, "-" if int(r["nearest"]) == NONE else names_db[int(r["nearest"])],
            "inf" if math.isinf(d) else "%.6f" % d))
    return "".join(out)


# ---- the model file, byte by byte as INTEGRATION.md section 6 lists it ----
MAGIC = b"RTCDBSM1"


def parse_model(blob):
    """dict of everything in a clust-dbscan --db file; raises ValueError on a foreign or truncated one"""
    at = [0]

    def take(fmt):
        size = struct.calcsize(fmt)
        if at[0] + size > len(blob):
            raise ValueError("truncated")
        v = struct.unpack_from(fmt, blob, at[0])
        at[0] += size
        return v

    def text():
        (n,) = take("<I")
        if at[0] + n > len(blob):
            raise ValueError("truncated")
        s = blob[at[0]:at[0] + n].decode()
        at[0] += n
        return s
    if blob[:8] != MAGIC:
        raise ValueError("foreign")
    at[0] = 8
    m = {}
    (m["version"], m["kind"], m["width"], m["by_file"], m["kmer_size"], m["half_k"], m["half_subk"], m["drlevel"], m["sketch_size"],
     m["min_pts"], m["max_posting"], m["n_clusters"]) = take("<12i")
    m["min_len"], m["n"] = take("<QQ")
    (m["eps"],) = take("<d")
    n = m["n"]
    m["labels"] = np.array(take("<%di" % n), dtype=np.int32)
    m["core"] = np.array(take("<%dB" % n), dtype=np.uint8)
    genomes = []
    for _ in range(n):
        g = {"file": text(), "name": text(), "comment": text()}
        g["length"], g["total_length"] = take("<QQ")
        genomes.append(g)
    m["genomes"] = genomes
    lens = take("<%dI" % n)
    dt = np.dtype("<u8" if m["width"] == 8 else "<u4")
    sk = []
    for ln in lens:
        size = ln * dt.itemsize
        if at[0] + size > len(blob):
            raise ValueError("truncated")
        sk.append(np.frombuffer(blob, dtype=dt, count=ln, offset=at[0]).copy())
        at[0] += size
    m["sketches"] = sk
    if at[0] != len(blob):
        raise ValueError("trailing bytes")
    return m


# ---- a set whose border and noise points can be taken out without moving a core flag ----
def satellite_set(seed, use64, n_fam=4, members=8, satellites=3, loners=10):
    """Families of `members` sketches that share a core of 150 hashes and hold 50 of their own (Jaccard 0.6 among them);
    `satellites` members per family have a satellite: the member's own 50 hashes, 60 of the family's core and 40 fresh ones --
    Jaccard 0.458 with that member, at most 0.25 with anything else; and loners.  With k-mer size 21 and eps 0.04 (Jaccard 0.275)
    at minPts 5 the members are core points with room to spare, each satellite is a border point with one neighbour and the
    loners are noise: taking one of them out moves no core flag.  Shuffled.  (The family sets of tests/sweep_sets.py do not serve
    here: their border points hold core points up -- at eps 0.04 / minPts 5, 0.02 / 4, 0.06 / 5 and 0.02 / 3 no clustered point
    of them can be taken out without moving a core flag, at 0.04 / 4 two can -- so they cannot give the five clustered points
    the leave-one-out test has to check.)"""
    rng = np.random.default_rng(seed)
    need = n_fam * (150 + members * 50 + satellites * 40) + loners * 120
    pool = rng.permutation(np.unique(rng.integers(1, (1 << 31) - 1, size=2 * need, dtype=np.int64)))
    assert len(pool) >= need
    at = [0]

    def fresh(m):
        at[0] += m
        return pool[at[0] - m:at[0]]
    out = []
    for _ in range(n_fam):
        core = fresh(150)
        own = [fresh(50) for _ in range(members)]
        out += [np.concatenate([core, o]) for o in own]
        out += [np.concatenate([own[i], core[:60], fresh(40)]) for i in range(satellites)]
    out += [fresh(120) for _ in range(loners)]
    out = [out[i] for i in rng.permutation(len(out))]
    return [np.unique(s).astype(np.uint64 if use64 else np.uint32) for s in out]
