"""rtc_mcl's definition (include/rtclust.h) restated with Python integers: Markov clustering in fixed point.  A matrix is a
list of columns, a column a dict {row: value}; no step forms a floating-point value."""
from math import isqrt

ONE = 1 << 30


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status  # the library's status name


def check_params(h, S):
    if not (isinstance(h, int) and 3 <= h <= 16):
        raise Refused("RTC_ERR_ARG", "inflation_x2 %r" % (h,))
    if not (isinstance(S, int) and 1 <= S <= 4096):
        raise Refused("RTC_ERR_ARG", "select %r" % (S,))


def adjacency(n, records):
    """the symmetric adjacency: duplicates of an unordered pair summed, u == v ignored"""
    adj = [dict() for _ in range(n)]
    for u, v, q in records:
        if u >= n or v >= n or u < 0 or v < 0 or q <= 0:
            raise Refused("RTC_ERR_ARG", "record (%d, %d, %d) with %d vertices" % (u, v, q, n))
        if u == v:
            continue
        adj[u][v] = adj[u].get(v, 0) + q
        adj[v][u] = adj[v].get(u, 0) + q
    for col in adj:
        for x in col.values():
            if x >= 1 << 32:
                raise Refused("RTC_ERR_UNSUPPORTED", "a summed entry of %d" % x)
    return adj


def select(entries, S):
    """entries: (row, x) pairs with x > 0.  The S largest under (x descending, row ascending), normalised to ONE."""
    kept = sorted(entries, key=lambda e: (-e[1], e[0]))[:S]
    X = sum(x for _, x in kept)
    out = {}
    for i, x in kept:
        p = x * ONE // X
        if p:
            out[i] = p
    return out


def start(n, records, S):
    adj = adjacency(n, records)
    M = []
    for j in range(n):
        col = dict(adj[j])
        col[j] = max(adj[j].values()) if adj[j] else 1
        M.append(select(col.items(), S))
    return M


def inflate(e1, h):
    y = e1
    for _ in range(h // 2 - 1):
        y = (y * e1) >> 30
    if h & 1:
        y = (y * isqrt(e1 << 30)) >> 30
    return y


def iterate(M, h, S):
    return iterate_counting(M, h, S)[0]


def iterate_counting(M, h, S):
    """-> (the next matrix, the columns that select cut: those with more than S rows alive after the inflation)"""
    N, cut = [], 0
    for j in range(len(M)):
        s = {}
        for k, pkj in M[j].items():
            for i, pik in M[k].items():
                s[i] = s.get(i, 0) + pik * pkj
        e = {i: v >> 30 for i, v in s.items() if v >> 30}
        if not e:
            N.append({})
            continue
        E = max(e.values())
        y = {}
        for i, ei in e.items():
            yi = inflate(ei * ONE // E, h)
            if yi:
                y[i] = yi
        cut += len(y) > S
        N.append(select(y.items(), S))
    return N, cut


def clusters(M):
    """labels from a matrix: every cluster named by its smallest member"""
    n = len(M)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    attractor = [M[a].get(a, 0) > 0 for a in range(n)]
    for j in range(n):
        if attractor[j]:
            for i in M[j]:
                if attractor[i]:
                    unite(j, i)
        elif M[j]:
            rows = [i for i in M[j] if attractor[i]] or list(M[j])
            unite(j, min(rows, key=lambda i: (-M[j][i], i)))
    return [find(x) for x in range(n)]


def mcl(n, records, h, S, T):
    """-> (labels, iterations, converged, matrix)"""
    check_params(h, S)
    M = start(n, records, S)
    iterations, converged = 0, 0
    while iterations < T:
        N = iterate(M, h, S)
        iterations += 1
        same = N == M
        M = N
        if same:
            converged = 1
            break
    return clusters(M), iterations, converged, M


def entries(M):
    """the matrix as rtc_mcl returns it: (col, row, value) in (col, row) order"""
    return [(j, i, M[j][i]) for j in range(len(M)) for i in sorted(M[j])]


def clusters_of(labels):
    out = {}
    for x, c in enumerate(labels):
        out.setdefault(c, []).append(x)
    return [out[c] for c in sorted(out)]
