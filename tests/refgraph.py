"""rtc_graph_build's edge rule restated from the reference's KssdLeidenCluster (src/leiden.cpp:168-293) with Python floats and
math.log: which pairs are edges, their weights, and the per-node top-k among the higher-numbered neighbours.

  - distance(): calculate_mash_distance_fast (:109-121);
  - the pairs: every u < v sharing a hash (the inverted index, :193, :201), the size ratio (:206-209), dist < threshold (:214);
  - k-NN (:195-231): node u keeps its knn_k best among v > u.  The reference ranks by the rounded distance with whatever order
    its heap leaves among equals; the library ranks by common / union exactly, larger first, equal ratios to the lower v, which
    is one of the reference's possible outcomes whenever equal distances come from equal ratios."""
import math
from fractions import Fraction


def distance(common, size1, size2, k):
    if common == 0:
        return 1.0
    union = size1 + size2 - common
    if union == 0:
        return 1.0
    jaccard = float(common) / union
    if jaccard <= 0.0:
        return 1.0
    if jaccard >= 1.0:
        return 0.0
    d = -1.0 / k * math.log(2.0 * jaccard / (1.0 + jaccard))
    return max(0.0, min(1.0, d))


def weight(common, size1, size2, k):
    return 1.0 - distance(common, size1, size2, k)


def edges(sketches, threshold, kmer_size, knn_k=0):
    """[(u, v, common)] in (u, v) order"""
    sets = [set(int(h) for h in s) for s in sketches]
    n = len(sets)
    out = []
    for u in range(n):
        row = []
        for v in range(u + 1, n):
            common = len(sets[u] & sets[v])
            if common == 0:
                continue
            a, b = len(sets[u]), len(sets[v])
            small, large = min(a, b), max(a, b)
            if float(small) / large < 0.5:
                continue
            if distance(common, a, b, kmer_size) < threshold:
                row.append((u, v, common))
        if knn_k > 0 and len(row) > knn_k:
            row.sort(key=lambda e: (-Fraction(e[2], len(sets[e[0]]) + len(sets[e[1]]) - e[2]), e[1]))
            row = sorted(row[:knn_k])
        out += row
    return out


def weighted(edge_list, sketches, kmer_size):
    """[(u, v, weight)] of an edge list"""
    return [(u, v, weight(c, len(sketches[u]), len(sketches[v]), kmer_size)) for u, v, c in edge_list]
