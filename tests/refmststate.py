"""Python restatement of the reference's clust-mst --save-rep / --append state (src/mst_state.cpp): the state file's byte
layout (MinHashMstState::save / KssdMstState::save), the initial state (one tree medoid per cluster), the append
(MinHashMstAppendCluster / KssdMstAppendCluster with their filters), the compaction and printMstStateClusterResult.

One rule is ours: among matches at equal distance the lowest representative slot survives, and the others are merged
into it in ascending slot order (the reference takes phmap's and OpenMP's order there)."""
import math
import struct

import refpost as RP

MH_MAGIC, KS_MAGIC = b"MHMSTST01", b"KSMSTST01"


def jaccard_min(threshold, k):
    e = math.exp(-threshold * float(k))
    return e / (2.0 - e)


def radio(threshold, k):  # KssdMstAppendCluster: std::pow(exp_dk, -1.0)
    return math.pow(math.exp(-threshold * float(k)), -1.0)


def min_common_needed(jmin, size_q, size_r, containment):
    if containment:
        return int(jmin * min(size_q, size_r))
    return int(jmin * (size_q + size_r) / (1.0 + jmin))


def ratio_ok(size_q, size_r, rad):
    ratio = float(size_q) / float(size_r)
    return not (ratio > rad or ratio < 1.0 / rad)


def distance(common, size_q, size_r, containment, k):
    """None where the reference skips the pair (denom <= 0)"""
    if containment:
        jac = common / float(min(size_q, size_r))
    else:
        denom = size_q + size_r - common
        if denom <= 0:
            return None
        jac = common / float(denom)
    if jac >= 1.0:
        return 0.0
    if jac <= 0.0:
        return 1.0
    d = -math.log(2.0 * jac / (1.0 + jac)) * (1.0 / float(k))
    return 1.0 if d > 1.0 else d


def keep(common, size_q, size_r, threshold, k, kssd, containment):
    """the reference's filters for one (query, representative) pair with `common` shared hashes: the distance or None"""
    if size_r == 0 or common == 0:
        return None
    if kssd and not ratio_ok(size_q, size_r, radio(threshold, k)):
        return None
    if common < min_common_needed(jaccard_min(threshold, k), size_q, size_r, containment and not kssd):
        return None
    d = distance(common, size_q, size_r, containment and not kssd, k)
    if d is None or not d <= threshold or math.isnan(d) or math.isinf(d):
        return None
    return d


def brute_pairs(sketches, n_reps, threshold, k, kssd, containment):
    """every (query, slot, common, dist) rtc_rep_match emits, by brute force over all pairs"""
    sets = [set(int(h) for h in s) for s in sketches]
    out = []
    for q in range(len(sketches) - n_reps):
        i = n_reps + q
        for j in range(i):
            c = len(sets[i] & sets[j])
            d = keep(c, len(sets[i]), len(sets[j]), threshold, k, kssd, containment)
            if d is not None:
                out.append((q, j, c, d))
    return out


class State:
    def __init__(self, kssd=False):
        self.kssd = kssd
        self.threshold = 0.05
        self.kmer_size = 21
        self.sketch_size, self.contain_compress, self.is_containment = 1000, 0, False
        self.half_k, self.half_subk, self.drlevel, self.use64 = 10, 6, 3, not kssd
        self.N, self.sketch_by_file = 0, True
        self.rep_ids, self.rep_lens, self.rep_names, self.rep_hashes = [], [], [], []
        self.clusters, self.member_names, self.member_lens = [], [], []

    def fields(self):
        return {k: (list(map(list, v)) if k in ("rep_hashes", "clusters") else v) for k, v in vars(self).items()}


def _index(st):
    idx = {}
    for r, hs in enumerate(st.rep_hashes):
        for h in hs:
            idx.setdefault(int(h), []).append(r)
    return sorted(idx.items())


def save(st, index_order=None):
    """the bytes of save(); index_order: a permutation of the index entries (the reference writes phmap's order)"""
    hw = "Q" if st.use64 else "I"
    b = bytearray(KS_MAGIC if st.kssd else MH_MAGIC)
    b += struct.pack("<di", st.threshold, st.kmer_size)
    if st.kssd:
        b += struct.pack("<iii?", st.half_k, st.half_subk, st.drlevel, st.use64)
    else:
        b += struct.pack("<ii?", st.sketch_size, st.contain_compress, st.is_containment)
    b += struct.pack("<?i", st.sketch_by_file, st.N)
    b += struct.pack("<Q", len(st.rep_hashes))
    for r, hs in enumerate(st.rep_hashes):
        nm = st.rep_names[r].encode()
        b += struct.pack("<iQI", st.rep_ids[r], st.rep_lens[r], len(nm)) + nm
        b += struct.pack("<Q", len(hs)) + struct.pack("<%d%s" % (len(hs), hw), *[int(h) for h in hs])
    b += struct.pack("<Q", len(st.clusters))
    for c in st.clusters:
        b += struct.pack("<Q", len(c)) + struct.pack("<%di" % len(c), *c)
    b += struct.pack("<Q", len(st.member_names))
    for nm in st.member_names:
        e = nm.encode()
        b += struct.pack("<I", len(e)) + e
    b += struct.pack("<Q", len(st.member_lens)) + struct.pack("<%dQ" % len(st.member_lens), *st.member_lens)
    idx = _index(st)
    if index_order is not None:
        idx = [idx[i] for i in index_order]
    b += struct.pack("<Q", len(idx))
    for h, lst in idx:
        b += struct.pack("<" + hw, h) + struct.pack("<Q", len(lst)) + struct.pack("<%di" % len(lst), *lst)
    return bytes(b)


def parse(raw):
    """the state in `raw` and its inverted index {hash: [reps]}"""
    pos = 9

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, raw, pos)
        pos += struct.calcsize("<" + fmt)
        return v

    kssd = raw[:9] == KS_MAGIC
    assert kssd or raw[:9] == MH_MAGIC
    st = State(kssd)
    st.threshold, st.kmer_size = take("di")
    if kssd:
        st.half_k, st.half_subk, st.drlevel, st.use64 = take("iii?")
    else:
        st.sketch_size, st.contain_compress, st.is_containment = take("ii?")
        st.use64 = True
    st.sketch_by_file, st.N = take("?i")
    hw = "Q" if st.use64 else "I"
    (R,) = take("Q")
    for _ in range(R):
        rid, ln, nn = take("iQI")
        st.rep_ids.append(rid)
        st.rep_lens.append(ln)
        st.rep_names.append(raw[pos:pos + nn].decode())
        pos += nn
        (m,) = take("Q")
        st.rep_hashes.append(list(take("%d%s" % (m, hw))))
    (C,) = take("Q")
    for _ in range(C):
        (m,) = take("Q")
        st.clusters.append(list(take("%di" % m)))
    (M,) = take("Q")
    for _ in range(M):
        (nn,) = take("I")
        st.member_names.append(raw[pos:pos + nn].decode())
        pos += nn
    (m,) = take("Q")
    st.member_lens = list(take("%dQ" % m))
    (H,) = take("Q")
    idx = {}
    for _ in range(H):
        (h,) = take(hw)
        (m,) = take("Q")
        idx[h] = list(take("%di" % m))
    assert pos == len(raw)
    return st, idx


def initial_state(st, names, lens, clusters, forest, hashes, by_file=True):
    """MinHashInitialMstState / KssdInitialMstState on `st`'s parameters: every cluster's tree medoid"""
    n = len(names)
    st.N, st.sketch_by_file = n, by_file
    st.member_names, st.member_lens = list(names), list(lens)
    rep = RP.tree_medoids(n, forest, float("inf"), lens)
    cands = RP.dedup_candidates(clusters, rep, float("inf"))
    for c, cl in enumerate(clusters):
        if not cl:
            continue
        r = cands[c][0] if cands[c] else cl[0]
        st.rep_ids.append(r)
        st.rep_names.append(names[r])
        st.rep_lens.append(lens[r])
        st.rep_hashes.append([int(h) for h in hashes[r]])
        st.clusters.append(list(cl))
    return st


class _UF:  # UnionFind.h
    def __init__(self, n):
        self.p, self.r = list(range(n)), [0] * n

    def extend(self):
        self.p.append(len(self.p))
        self.r.append(0)

    def find(self, x):
        while self.p[x] != x:
            x = self.p[x]
        return x

    def merge(self, x, y):
        x, y = self.find(x), self.find(y)
        if x == y:
            return
        if self.r[x] > self.r[y]:
            self.p[y] = x
        elif self.r[x] < self.r[y]:
            self.p[x] = y
        else:
            self.p[x] = y
            self.r[y] += 1


def _apply(st, uf, matches, name, ln, hashes):
    nid = st.N
    st.N += 1
    st.member_names.append(name)
    st.member_lens.append(ln)
    if not matches:
        st.rep_ids.append(nid)
        st.rep_names.append(name)
        st.rep_lens.append(ln)
        st.rep_hashes.append([int(h) for h in hashes])
        st.clusters.append([nid])
        uf.extend()
        return len(st.rep_hashes) - 1
    matches = sorted(matches)  # by slot; the lowest slot among equal distances survives
    best = min(range(len(matches)), key=lambda m: (matches[m][1], matches[m][0]))
    surv = matches[best][0]
    for m, (r, _) in enumerate(matches):
        if m == best:
            continue
        o, s = uf.find(r), uf.find(surv)
        if o == s:
            continue
        uf.merge(s, o)
        new_root = uf.find(s)
        loser = o if new_root == s else s
        st.clusters[new_root] += st.clusters[loser]
        st.clusters[loser] = []
    st.clusters[uf.find(surv)].append(nid)
    return None


def _finish(st, uf):
    keep_r = [r for r in range(len(st.rep_hashes)) if st.clusters[r] and uf.find(r) == r]
    live = [list(st.clusters[r]) for r in keep_r]
    for a in ("rep_ids", "rep_names", "rep_lens", "rep_hashes", "clusters"):
        setattr(st, a, [getattr(st, a)[r] for r in keep_r])
    return live


def append(st, names, lens, qhashes):
    """MinHashMstAppendCluster / KssdMstAppendCluster as the reference runs it: probe the index of every representative
    (merged-away ones included), redirect to the roots, and measure each root with its own count"""
    kssd, cont = st.kssd, st.is_containment and not st.kssd
    uf = _UF(len(st.rep_hashes))
    idx = {}
    for r, hs in enumerate(st.rep_hashes):
        for h in hs:
            idx.setdefault(int(h), []).append(r)
    for q, hs in enumerate(qhashes):
        hits = {}
        for h in hs:
            for r in idx.get(int(h), ()):
                hits[r] = hits.get(r, 0) + 1
        roots = {uf.find(r) for r in hits}
        matches = []
        for r in roots:
            if r not in hits:
                continue
            d = keep(hits[r], len(hs), len(st.rep_hashes[r]), st.threshold, st.kmer_size, kssd, cont)
            if d is not None:
                matches.append((r, d))
        r_new = _apply(st, uf, matches, names[q], lens[q], hs)
        if r_new is not None:
            for h in hs:
                idx.setdefault(int(h), []).append(r_new)
    return _finish(st, uf)


def replay(st, names, lens, qhashes, pairs):
    """the same decisions from a list of (query, slot, common, dist) pairs, slot R + i = query i"""
    R0 = len(st.rep_hashes)
    uf = _UF(R0)
    became = [None] * len(names)
    by_q = {}
    for q, s, _, d in pairs:
        by_q.setdefault(q, []).append((s, d))
    for q in range(len(names)):
        matches = []
        for s, d in sorted(by_q.get(q, ())):
            r = s if s < R0 else became[s - R0]
            if r is None or uf.find(r) != r:
                continue
            matches.append((r, d))
        became[q] = _apply(st, uf, matches, names[q], lens[q], qhashes[q])
    return _finish(st, uf)


def cluster_text(live, member_names, member_lens, by_file, threshold):
    """printMstStateClusterResult"""
    out = []
    if threshold >= 0.0:
        out.append("# Clustering threshold: %.6f\n# Total clusters: %d\n#\n" % (threshold, len(live)))
    for i, c in enumerate(live):
        out.append("the cluster %d is: \n" % i)
        for j, g in enumerate(c):
            name, ln = (member_names[g], member_lens[g]) if 0 <= g < len(member_names) else ("N/A", 0)
            out.append(("\t%5d\t%6d\t%12dnt\t%20s\n" if by_file else "\t%6d\t%6d\t%12dnt\t%20s\n") % (j, g, ln, name))
        out.append("\n")
    return "".join(out)
