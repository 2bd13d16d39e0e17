"""The definition of rtc_graph_snn (include/rtclust.h) with Python sets, nothing clever.

snn(n, records) takes records (u, v) or (u, v, q) in any order; q is not read.  G is the simple undirected graph of the records:
(u, v) and (v, u) are one edge, equal edges collapse, a record with u == v is in no neighbourhood."""


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__("%s: %s" % (status, why))
        self.status = status


def neighbourhoods(n, records):
    if n >= (1 << 31) - 1:
        raise Refused("RTC_ERR_ARG", "%d vertices" % n)
    N = [set() for _ in range(n)]
    for r in records:
        u, v = r[0], r[1]
        if u >= n or v >= n:
            raise Refused("RTC_ERR_ARG", "record (%d, %d) with %d vertices" % (u, v, n))
        if u != v:
            N[u].add(v)
            N[v].add(u)
    return N


def snn(n, records):
    """(shared, deg_u, deg_v, flags) of every record, record for record"""
    N = neighbourhoods(n, records)
    out = []
    for r in records:
        u, v = r[0], r[1]
        if u == v:
            out.append((0, len(N[u]), len(N[u]), 1))
        else:
            out.append((len(N[u] & N[v]), len(N[u]), len(N[v]), 0))
    return out


def weight(shared, deg_u, deg_v):
    """|N[u] & N[v]| / |N[u] | N[v]| on the closed neighbourhoods: one division of two Python floats"""
    return float(shared + 2) / float(deg_u + deg_v - shared)


def weight_of_sets(N, u, v):
    """the same weight from the closed neighbourhoods themselves"""
    a, b = N[u] | {u}, N[v] | {v}
    return len(a & b), len(a | b)


def edges(n, records):
    """the distinct edges of G as (low, high), ascending"""
    return sorted({(min(r[0], r[1]), max(r[0], r[1])) for r in records if r[0] != r[1]})


def triangles(n, records):
    N = neighbourhoods(n, records)
    total = sum(len(N[u] & N[v]) for u, v in edges(n, records))
    assert total % 3 == 0
    return total // 3


def probes(n, records):
    """the elements of the shorter rows, over the records with u != v"""
    N = neighbourhoods(n, records)
    return sum(min(len(N[r[0]]), len(N[r[1]])) for r in records if r[0] != r[1])


def longer_rows(n, records):
    """for every record with u != v, the length of its owner's row: the longer of the two"""
    N = neighbourhoods(n, records)
    return [max(len(N[r[0]]), len(N[r[1]])) for r in records if r[0] != r[1]]


def reweighted(n, records, weights, prune=0.0):
    """clust-leiden --snn on records (u, v) with their similarity weights: every record with u != v takes the SNN weight, one with
    u == v keeps its own; then the records below prune drop out, in one pass.  Returns ([(u, v, w)], pruned)."""
    out, pruned = [], 0
    for (u, v), w0, (s, du, dv, fl) in zip(records, weights, snn(n, records)):
        w = w0 if fl & 1 else weight(s, du, dv)
        if w < prune:
            pruned += 1
        else:
            out.append((u, v, w))
    return out, pruned
