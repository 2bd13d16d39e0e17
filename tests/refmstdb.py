"""Python restatement of the reference's clust-mst --db read side (src/mst_state.cpp:1150-1415, src/sub_command.cpp:942-1236):
the stats report (MinHashMstPrintStats / KssdMstPrintStats), the top-k search (MinHashMstQueryTopK / KssdMstQueryTopK) and
the query / assign TSVs.

One rule is ours: equal distances rank by the lower representative slot (the reference's std::sort leaves them in phmap's
order).  The search ranks by the exact key common / denom (fractions.Fraction), the distance is libm's from that key."""
import math
from fractions import Fraction


def stats_text(st):
    """the report --stats prints on stdout; the unique hashes are counted over every representative slot"""
    uniq = len(set(int(h) for hs in st.rep_hashes for h in hs))
    o = []
    if st.kssd:
        o.append("========== KSSD MST RepDB stats ==========\n")
        o.append("  Kmer size:        %d\n" % st.kmer_size)
        o.append("  half_k:           %d\n" % st.half_k)
        o.append("  half_subk:        %d\n" % st.half_subk)
        o.append("  drlevel:          %d\n" % st.drlevel)
        o.append("  use64:            %s\n" % ("yes" if st.use64 else "no"))
    else:
        o.append("========== MinHash MST RepDB stats ==========\n")
        o.append("  Kmer size:        %d\n" % st.kmer_size)
        o.append("  Sketch size:      %d\n" % st.sketch_size)
        o.append("  Containment:      %s\n" % ("yes" if st.is_containment else "no"))
        if st.is_containment:
            o.append("  Contain compress: %d\n" % st.contain_compress)
    o.append("  Threshold:        %.6f\n" % st.threshold)
    o.append("  Total reps slots: %d\n" % len(st.rep_hashes))
    o.append("  sketch_by_file:   %s\n" % ("yes" if st.sketch_by_file else "no"))
    o.append("  Total members N:  %d\n" % st.N)
    if st.kssd:
        o.append("  Inverted index:   %d unique hashes (%s-bit)\n" % (uniq, "64" if st.use64 else "32"))
    else:
        o.append("  Inverted index:   %d unique hashes\n" % uniq)
    sizes = [len(c) for c in st.clusters if c]
    edges = [(1, 1), (2, 2), (3, 5), (6, 10), (11, 100), (101, 1000), (1001, 1 << 62)]
    b = [sum(1 for s in sizes if lo <= s <= hi) for lo, hi in edges]
    live, total = len(sizes), sum(sizes)
    o.append("  Live clusters:    %d\n" % live)
    o.append("  Total members:    %d\n" % total)
    o.append("  Cluster size:     min=%d max=%d avg=%.2f\n" % (min(sizes) if sizes else 0, max(sizes) if sizes else 0,
                                                             total / live if live else 0.0))
    o.append("  Size histogram:\n")
    for label, v in zip(("size=1         ", "size=2         ", "size=3-5       ", "size=6-10      ", "size=11-100    ",
                         "size=101-1000  ", "size>1000      "), b):
        o.append("    %s: %d\n" % (label, v))
    o.append("==========================================\n" if st.kssd else "==============================================\n")
    return "".join(o)


def wmode(st):
    if st.kssd:
        return 0
    if st.is_containment:
        return 1
    return 2 | (max(st.sketch_size, 1) << 2)


def mash_counts(a, b, s):
    """Mash's union-truncated merge: (common, denom) among the first s union elements"""
    i = j = c = d = 0
    while d < s and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            c += 1
            i += 1
            j += 1
        d += 1
    if d < s:
        d += min((len(a) - i) + (len(b) - j), s - d)
    return c, d


def counts(q, r, mode):
    """(common, denom) of query sketch q against representative sketch r, both ascending lists"""
    if mode & 3 == 2:
        return mash_counts(list(q), list(r), mode >> 2)
    c = len(set(q) & set(r))
    return c, (min(len(q), len(r)) if mode & 3 == 1 else len(q) + len(r) - c)


def distance(common, denom, mode, k):
    j = common / float(denom) if denom else 0.0
    if j == 1.0:
        d = 0.0
    elif j == 0.0:
        d = 1.0
    elif mode & 3 == 1:
        d = -(1.0 / k) * math.log(j)
    else:
        d = -math.log(2.0 * j / (1.0 + j)) / float(k)
        d = 1.0 if d > 1.0 else d
    return math.inf if math.isnan(d) else d


def topk(reps, queries, mode, k, live=None):
    """per query: [(slot, common, denom)] of its best k candidates (k == 0: all); a candidate is a live slot that shares a hash
    over the full sketches"""
    sets = [set(int(h) for h in r) for r in reps]
    out = []
    for q in queries:
        qs = set(int(h) for h in q)
        cand = []
        for s, r in enumerate(reps):
            if live is not None and not live[s]:
                continue
            if not (qs & sets[s]):
                continue
            c, d = counts([int(h) for h in q], [int(h) for h in r], mode)
            cand.append((-Fraction(c, d), s, c, d))
        cand.sort()
        out.append([(s, c, d) for _, s, c, d in (cand if k == 0 else cand[:k])])
    return out


def live_ids(st):
    ids, n = [], 0
    for c in st.clusters:
        ids.append(n if c else -1)
        n += 1 if c else 0
    return ids


def query_tsv(st, qnames, hits):
    """mst_repdb_query's TSV from topk()'s lists"""
    mode, ids = wmode(st), live_ids(st)
    o = ["#query\trank\trep_name\tdistance\tcluster_id\tcluster_size\n"]
    for i, (nm, hs) in enumerate(zip(qnames, hits)):
        nm = nm or "query_%d" % i
        if not hs:
            o.append("%s\t0\tno_match\t-1\t-1\t0\n" % nm)
        for r, (s, c, d) in enumerate(hs):
            o.append("%s\t%d\t%s\t%.6f\t%d\t%d\n" % (nm, r + 1, st.rep_names[s], distance(c, d, mode, st.kmer_size), ids[s],
                                                    len(st.clusters[s])))
    return "".join(o)


def assign_tsv(st, qnames, hits):
    """mst_repdb_assign's TSV from topk(..., 1)"""
    mode, ids = wmode(st), live_ids(st)
    o = ["#query\tassigned_cluster\trep_name\tdistance\tcluster_size\tstatus\n"]
    for i, (nm, hs) in enumerate(zip(qnames, hits)):
        nm = nm or "query_%d" % i
        d = distance(hs[0][1], hs[0][2], mode, st.kmer_size) if hs else None
        if hs and d <= st.threshold:
            s = hs[0][0]
            o.append("%s\t%d\t%s\t%.6f\t%d\tassigned\n" % (nm, ids[s], st.rep_names[s], d, len(st.clusters[s])))
        else:
            o.append("%s\t-1\tunassigned\t-1\t0\tnovel\n" % nm)
    return "".join(o)
