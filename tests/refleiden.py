"""rtc_leiden's definition (include/rtclust.h) restated with Python integers: the deterministic, synchronous Leiden the library
runs on the GPU.  Nothing here is taken from igraph; the header is the definition and this file repeats it.

leiden(n, edges, resolution, objective, stats=None) -> (labels, n_clusters, counters), edges an iterable of (u, v, q), q >= 1 the
weight in units of 2^-20, counters the ten of rtc_leiden_counters with the three times left at 0.  After every refinement it
asserts that each refined community lies inside one coarse community and is connected over its positive edges.  stats, a dict,
receives what the counters do not hold: "ineligible" (vertices that failed the eligibility test, all refinements), "split"
(coarse communities a refinement left in two or more pieces) and "row_lengths" (the set of adjacency row lengths met); a list
under "trace", if the caller put one there, receives (iteration, level, coarse, refined) after every refinement.  Lists, one
entry per event: "proposer_rows" (the row length, self entry included, of every vertex that proposed, once per proposal),
"proposer_rows_outside" (the same for proposers with a neighbour outside their coarse community), "proposer_rows_nontarget"
(for proposers with a neighbouring refined community, inside their coarse community, that is no target in that round),
"move_rounds" and "refine_rounds" (the rounds of every level's move phase and refinement) and "levels_by_iteration"."""

import math

CPM = 0
MODULARITY = 1
MAX_ROUNDS = 64
MAX_LEVELS = 32
MAX_ITERATIONS = 100


def _llround(x):
    r = math.floor(x)
    return r + 1 if x - r >= 0.5 else r


def resolution_units(resolution):
    return _llround(resolution * 65536.0)


def normalise_and_quantise(records, objective):
    """The command line's weights to q (leiden_quantise in rtc_host.cpp): records of (u, v, weight as a double).  CPM: when
    max - min < 0.5 and the range is above 1e-6, weight' = (weight - min) / range; q = llround(weight' * 2^20), records with
    q == 0 dropped.  Modularity: q = max(1, llround(weight * 2^20)), nothing dropped.  -> (records of (u, v, q), normalised?)"""
    records = list(records)
    if objective == MODULARITY or not records:
        return [(u, v, max(1, _llround(w * 1048576.0))) for u, v, w in records], False
    lo = min([1.0] + [w for _, _, w in records])  # the reference starts its search at min 1.0, max 0.0
    hi = max([0.0] + [w for _, _, w in records])
    rng = hi - lo
    scaled = hi - lo < 0.5 and rng > 1e-6
    out = []
    for u, v, w in records:
        q = _llround(((w - lo) / rng if scaled else w) * 1048576.0)
        if q >= 1:
            out.append((u, v, q))
    return out, hi - lo < 0.5


def _adjacency(n, entries):
    adj = [dict() for _ in range(n)]
    for a, b, w in entries:
        adj[a][b] = adj[a].get(b, 0) + w
    return adj


def _totals(comm, nu):
    tot = [0] * len(comm)
    for x, c in enumerate(comm):
        tot[c] += nu[x]
    return tot


def _move(adj, nu, comm, A, gB):
    """(a): rtc_louvain's rounds with the general score, from the partition comm -> (comm, rounds, moves)"""
    n = len(adj)
    comm = list(comm)
    N = _totals(comm, nu)
    rounds = moves = idle = 0
    while rounds < MAX_ROUNDS and idle < 2:
        odd = rounds & 1
        new = list(comm)
        moved = 0
        for x in range(n):
            c = comm[x]
            e = {}
            for y, w in adj[x].items():
                if y != x:
                    e[comm[y]] = e.get(comm[y], 0) + w
            s_c = e.get(c, 0) * A - gB * nu[x] * (N[c] - nu[x])
            best_s, best_d = s_c, c
            for d in sorted(e):
                if d == c or (d > c) != bool(odd):
                    continue
                s = e[d] * A - gB * nu[x] * N[d]
                if s > best_s:  # ascending d: an equal score keeps the smaller community
                    best_s, best_d = s, d
            if best_d != c:
                new[x] = best_d
                moved += 1
        comm = new
        N = _totals(comm, nu)
        rounds += 1
        moves += moved
        idle = 0 if moved else idle + 1
    return comm, rounds, moves


def _refine(adj, nu, coarse, A, gB, stats):
    """(b) -> (R, rounds, merges accepted, proposals rejected)"""
    n = len(adj)
    NC = _totals(coarse, nu)
    R = list(range(n))
    inner = [sum(w for y, w in adj[x].items() if y != x and coarse[y] == coarse[x]) for x in range(n)]
    eligible = [inner[x] * A >= gB * nu[x] * (NC[coarse[x]] - nu[x]) for x in range(n)]
    stats["ineligible"] = stats.get("ineligible", 0) + eligible.count(False)
    rounds = merges = rejected = idle = 0
    while rounds < MAX_ROUNDS and idle < 2:
        odd = rounds & 1
        Nr = _totals(R, nu)
        cnt = [0] * n
        E = [0] * n
        for x in range(n):
            cnt[R[x]] += 1
            for y, w in adj[x].items():
                if y != x and coarse[y] == coarse[x] and R[y] != R[x]:
                    E[R[x]] += w
        # a community that has members holds the vertex it is named after, so coarse[r] is its coarse community
        target = [cnt[r] > 0 and E[r] * A >= gB * Nr[r] * (NC[coarse[r]] - Nr[r]) for r in range(n)]
        prop = [None] * n
        for x in range(n):
            if not eligible[x] or cnt[R[x]] != 1:
                continue
            assert R[x] == x
            e = {}
            for y, w in adj[x].items():
                if y != x and coarse[y] == coarse[x]:
                    e[R[y]] = e.get(R[y], 0) + w
            best_s = -1
            for d in sorted(e):
                if d == x or (d > x) != bool(odd) or not target[d]:
                    continue
                s = e[d] * A - gB * nu[x] * Nr[d]
                if s >= 0 and s > best_s:
                    best_s, prop[x] = s, d
            if prop[x] is not None:  # stats only
                stats.setdefault("proposer_rows", []).append(len(adj[x]))
                if any(coarse[y] != coarse[x] for y in adj[x]):
                    stats.setdefault("proposer_rows_outside", []).append(len(adj[x]))
                if any(d != x and not target[d] for d in e):
                    stats.setdefault("proposer_rows_nontarget", []).append(len(adj[x]))
        accepted = 0
        for x in range(n):
            if prop[x] is None:
                continue
            if prop[prop[x]] is None:  # the vertex a community is named after is its only member that can propose
                R[x] = prop[x]
                accepted += 1
            else:
                rejected += 1
        if any(p is not None for p in prop):
            assert accepted > 0, "a round with a proposal makes progress"
        rounds += 1
        merges += accepted
        idle = 0 if accepted else idle + 1
    # every refined community lies inside one coarse community and is connected over its positive edges
    members = {}
    for x in range(n):
        members.setdefault(R[x], []).append(x)
    for r, ms in members.items():
        assert all(coarse[x] == coarse[r] for x in ms)
        seen, todo, inside = {ms[0]}, [ms[0]], set(ms)
        while todo:
            x = todo.pop()
            for y, w in adj[x].items():
                if w > 0 and y in inside and y not in seen:
                    seen.add(y)
                    todo.append(y)
        assert len(seen) == len(ms), "a refined community is disconnected"
    pieces = {}
    for r in members:
        pieces[coarse[r]] = pieces.get(coarse[r], 0) + 1
    stats["split"] = stats.get("split", 0) + sum(1 for c in pieces.values() if c >= 2)
    return R, rounds, merges, rejected


def _by_smallest(comm):
    """comm renumbered 0, 1, ... by the smallest member -> (new numbers, their count)"""
    smallest = {}
    for x, c in enumerate(comm):
        smallest.setdefault(c, x)
    order = {c: i for i, c in enumerate(sorted(smallest, key=smallest.get))}
    return [order[c] for c in comm], len(order)


def _named_by_smallest(comm):
    smallest = {}
    for x, c in enumerate(comm):
        smallest.setdefault(c, x)
    return [smallest[c] for c in comm]


def _iteration(adj0, nu0, start, A, gB, C, stats):
    """one iteration from the partition start (named by smallest member) -> labels numbered by smallest original vertex"""
    adj, nu, coarse = adj0, nu0, list(start)
    label = list(range(len(adj0)))  # the vertex of the current level every original vertex lies in
    levels = 0
    while True:
        stats.setdefault("row_lengths", set()).update(len(row) for row in adj)
        coarse, r, moved = _move(adj, nu, coarse, A, gB)
        C[2] += r
        C[3] += moved
        stats.setdefault("move_rounds", []).append(r)
        R, r, merges, rejected = _refine(adj, nu, coarse, A, gB, stats)
        C[4] += r
        C[5] += merges
        stats.setdefault("refine_rounds", []).append(r)
        C[6] += rejected
        levels += 1
        C[1] += 1
        if "trace" in stats:
            stats["trace"].append((C[0], levels - 1, list(coarse), list(R)))
        if not merges or levels == MAX_LEVELS:
            stats.setdefault("levels_by_iteration", []).append(levels)
            return _by_smallest([coarse[v] for v in label])
        newc, count = _by_smallest(R)
        label = [newc[v] for v in label]
        nxt_coarse = [None] * count
        nxt_nu = [0] * count
        for x in range(len(adj)):
            nxt_coarse[newc[x]] = coarse[x]
            nxt_nu[newc[x]] += nu[x]
        adj = _adjacency(count, [(newc[x], newc[y], w) for x, row in enumerate(adj) for y, w in row.items()])
        nu = nxt_nu
        coarse = _named_by_smallest(nxt_coarse)


def leiden(n, edges, resolution=1.0, objective=CPM, stats=None):
    g = resolution_units(resolution)
    assert 0 < g < (1 << 32) and objective in (CPM, MODULARITY)
    stats = {} if stats is None else stats
    entries = []
    for u, v, q in edges:
        assert 0 <= u < n and 0 <= v < n and q >= 1
        entries += [(u, v, q), (v, u, q)]  # u == v: both land on the self entry, 2q
    C = [0] * 10
    labels = list(range(n))
    if not entries:
        return labels, n, C
    adj = _adjacency(n, entries)
    k = [sum(row.values()) for row in adj]
    M2 = sum(k)
    assert M2 < (1 << 46)
    if objective == CPM:
        nu, A, gB = [1] * n, 65536, g << 20
    else:
        nu, A, gB = k, M2 * 65536, g
    ncl = n
    while C[0] < MAX_ITERATIONS:
        new, ncl = _iteration(adj, nu, _named_by_smallest(labels), A, gB, C, stats)
        C[0] += 1
        same = new == labels
        labels = new
        if same:
            break
    return labels, ncl, C


def quality(n, edges, labels, resolution, objective):
    """*h_quality of rtc_leiden, from the labels"""
    g = resolution_units(resolution)
    ncl = max(labels) + 1 if labels else 0
    inner, tot, size = [0] * ncl, [0] * ncl, [0] * ncl
    for c in labels:
        size[c] += 1
    M2 = 0
    for u, v, q in edges:
        M2 += 2 * q
        tot[labels[u]] += q
        tot[labels[v]] += q
        if labels[u] == labels[v]:
            inner[labels[u]] += 2 * q
    if not M2:
        return 0.0
    if objective == CPM:
        return sum(inner[c] * 65536 - (g << 20) * size[c] * size[c] for c in range(ncl)) / (M2 * 65536)
    return sum(inner[c] * M2 * 65536 - g * tot[c] * tot[c] for c in range(ncl)) / (M2 * M2 * 65536)


def clusters_of(labels):
    """members of every cluster, clusters in label order"""
    out = {}
    for x, c in enumerate(labels):
        out.setdefault(c, []).append(x)
    return [out[c] for c in sorted(out)]
