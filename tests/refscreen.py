"""The definition of rtc_rep_screen (include/rtclust.h) restated over Python sets with an inverted index, and the Python
rendering of clust-mst --db --screen's two reports.  Nothing here looks at how the library computes."""
import math

import numpy as np

Q20 = 1 << 20


def screen(reps, queries, min_common=1, min_cont_q20=0, min_unique=1, max_picks=0, live=None):
    """reps / queries: lists of iterables of distinct hashes.  Returns (hits, sums, info):
    hits[q]  [(slot, common, size, unique, rank)] in the library's order: picks by rank, the rest by common / size, larger
             first, compared by cross-multiplication, equal ratios to the lower slot
    sums[q]  (n_hashes, n_matched, n_explained, n_hits, n_picks)
    info[q]  dict: rounds (picks made), ties (the picks decided between equal counts by the lower slot), expansion (the most
             live representatives one hash of the sample lies in), matches (its match records), widest_pick (the largest
             common of a pick), holders_max (the most eligible candidates that hold one matched hash), last_index_picks (the
             ranks won by the highest eligible slot)"""
    assert min_unique >= 1 and 0 <= min_cont_q20 <= Q20
    sizes = [len(r) for r in reps]
    index = {}
    for s, r in enumerate(reps):
        if live is not None and not live[s]:
            continue
        for h in r:
            index.setdefault(int(h), []).append(s)
    hits, sums, info = [], [], []
    for x in queries:
        xs = [int(h) for h in x]
        shared = {}  # slot -> the hashes of X it holds
        expansion = matches = 0
        for h in xs:
            run = index.get(h, ())
            expansion = max(expansion, len(run))
            matches += len(run)
            for s in run:
                shared.setdefault(s, []).append(h)
        elig = sorted(s for s, hs in shared.items()
                      if len(hs) >= max(1, min_common) and len(hs) * Q20 >= min_cont_q20 * sizes[s])
        pos = {s: i for i, s in enumerate(elig)}
        holders = {}  # matched hash -> the eligible candidates that hold it
        for s in elig:
            for h in shared[s]:
                holders.setdefault(h, []).append(pos[s])
        u = np.array([len(shared[s]) for s in elig], dtype=np.int64)
        alive = set(holders)
        n_matched = len(alive)
        rank = [0] * len(elig)
        unique = [0] * len(elig)
        ties = []
        last_index_picks = []
        widest_pick = 0
        holders_max = max((len(c) for c in holders.values()), default=0)
        t = 0
        limit = min(max_picks, len(elig)) if max_picks else len(elig)
        while t < limit:
            best = int(u.max())
            if best < min_unique:
                break
            tied = np.flatnonzero(u == best)
            w = int(tied[0])  # candidates are in slot order: the lower slot
            t += 1
            if len(tied) > 1:
                ties.append(t)
            rank[w], unique[w] = t, best
            widest_pick = max(widest_pick, len(shared[elig[w]]))
            if w == len(elig) - 1:
                last_index_picks.append(t)
            for h in shared[elig[w]]:
                if h in alive:
                    alive.discard(h)
                    for c in holders[h]:
                        u[c] -= 1
            assert u[w] == 0
        for i in range(len(elig)):
            if not rank[i]:
                unique[i] = int(u[i])
        recs = [(s, len(shared[s]), sizes[s], unique[i], rank[i]) for i, s in enumerate(elig)]
        picks = sorted((r for r in recs if r[4]), key=lambda r: r[4])
        rest = sorted((r for r in recs if not r[4]), key=_ratio_key)
        hits.append(picks + rest)
        sums.append((len(xs), n_matched, n_matched - len(alive), len(recs), len(picks)))
        info.append({"rounds": t, "ties": ties, "expansion": expansion, "matches": matches, "widest_pick": widest_pick,
                     "holders_max": holders_max, "last_index_picks": last_index_picks})
    return hits, sums, info


class _Ratio:
    """common / size, larger first, exact; equal ratios by the lower slot"""

    def __init__(self, r):
        self.slot, self.common, self.size = r[0], r[1], r[2]

    def __lt__(self, o):
        l, r = self.common * o.size, o.common * self.size
        return l > r if l != r else self.slot < o.slot


def _ratio_key(r):
    return _Ratio(r)


def containment_order(recs):
    """a query's hits by containment alone (what the order would be without the rounds)"""
    return sorted(recs, key=_ratio_key)


def flat(hits):
    """[(query, slot, common, size, unique, rank)] as the library lays the hits out"""
    return [(q,) + tuple(r) for q, hs in enumerate(hits) for r in hs]


def identity(common, size, kmer_size):
    if common == size:
        return 1.0
    if common == 0:
        return 0.0
    return math.pow(float(common) / float(size), 1.0 / kmer_size)


def screen_tsv(names, rep_names, cluster_id, cluster_size, hits, sums, kmer_size):
    o = ["#sample\trank\tcluster_id\trep_name\tcluster_size\tshared\trep_hashes\tcontainment\tidentity\tunique\tunique_share\n"]
    for q, (nm, hs) in enumerate(zip(names, hits)):
        nm = nm or "query_%d" % q
        if not hs:
            o.append("%s\t0\t-1\tno_match\t0\t0\t0\t0.000000\t0.000000\t0\t0.000000\n" % nm)
        for s, c, size, uq, rank in hs:
            o.append("%s\t%s\t%d\t%s\t%d\t%d\t%d\t%.6f\t%.6f\t%d\t%.6f\n" % (
                nm, str(rank) if rank else "-", cluster_id[s], rep_names[s], cluster_size[s], c, size, float(c) / float(size),
                identity(c, size, kmer_size), uq, float(uq) / float(sums[q][0])))
    return "".join(o)


def summary_tsv(names, sums):
    o = ["#sample\thashes\tmatched\texplained\thits\tpicks\tunexplained_share\n"]
    for q, (nm, s) in enumerate(zip(names, sums)):
        nm = nm or "query_%d" % q
        share = "%.6f" % (float(s[0] - s[2]) / float(s[0])) if s[0] else "-"
        o.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (nm, s[0], s[1], s[2], s[3], s[4], share))
    return "".join(o)
