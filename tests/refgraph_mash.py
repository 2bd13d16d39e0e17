"""rtc_graph_build_mash's edge rule restated: the graph of clust-leiden --minhash.  The counts and the distance are
tests/refdbscan_mash.py's (the union-truncated merge and MinHash::distance() as the project restates them, Python floats and
math.log); this adds what makes a graph of them:

  - the pairs: every u < v with both lists non-empty, a shared hash, and distance(common, denom) < threshold strictly.  No
    size-ratio rule (that is the KSSD graph's, tests/refgraph.py).  A pair whose only shared hashes lie beyond the truncation
    has common 0, distance 1, and is no edge at any threshold <= 1;
  - k-NN: node u keeps its knn_k best among v > u, ranked by Fraction(common, denom), larger first, equal ratios to the lower v;
  - the strict decision table: cmin[d] = the least common with distance(common, d) < threshold, d + 1 where none is."""
from fractions import Fraction

from tests.refdbscan_mash import distance, mash_counts


def counts(sketches, sketch_size):
    """{(u, v): (common, denom)} for every u < v with both lists non-empty and a shared hash"""
    lists = [[int(h) for h in s] for s in sketches]
    sets = [set(x) for x in lists]
    out = {}
    for u in range(len(lists)):
        if not lists[u]:
            continue
        for v in range(u + 1, len(lists)):
            if lists[v] and not sets[u].isdisjoint(sets[v]):
                out[(u, v)] = mash_counts(lists[u], lists[v], sketch_size)
    return out


def edges(pair_counts, threshold, kmer_size, knn_k=0):
    """[(u, v, common, denom)] in (u, v) order from counts()'s result"""
    rows = {}
    for (u, v), (c, d) in pair_counts.items():
        if distance(c, d, kmer_size) < threshold:  # common 0: distance 1, never below a threshold <= 1
            rows.setdefault(u, []).append((u, v, c, d))
    out = []
    for u in sorted(rows):
        row = sorted(rows[u])
        if knn_k > 0 and len(row) > knn_k:
            row.sort(key=lambda e: (-Fraction(e[2], e[3]), e[1]))
            row = sorted(row[:knn_k])
        out += row
    return out


def weight(common, denom, kmer_size):
    return 1.0 - distance(common, denom, kmer_size)


def weighted(edge_list, kmer_size):
    """[(u, v, weight)] of an edge list"""
    return [(u, v, weight(c, d, kmer_size)) for u, v, c, d in edge_list]


def strict_table(sketch_size, kmer_size, threshold):
    """cmin[d], d = 0 .. sketch_size, by a linear scan"""
    out = []
    for d in range(sketch_size + 1):
        c = 0
        while c <= d and not distance(c, d, kmer_size) < threshold:
            c += 1
        out.append(c)
    return out
