"""CPU suite: the sets of tests/community_sets.py hold, on the restatements alone (tests/reflouvain.py, tests/refleiden.py), the
cases tests/test_gpu_community_edges.py runs them for: more rows than a launch of the row kernel has workgroups, proposers on
long rows under both objectives, rows at the lengths where the path changes, neighbours that share a table's last home slot,
every cap of the loops, self loops with repeated and reversed records, total weight just under 2^46.  The last test applies
wrong rules to the restatements (ties to the larger id, a filter left out, the self entry counted, caps one short) and asserts
that each changes the answer on one of the sets."""
import functools
import types

import community_sets as S
import refleiden
import reflouvain
from refleiden import CPM, MODULARITY

ONE = S.ONE
NUM_CU = 256  # an MI355X; the GPU test takes the device's own


@functools.lru_cache(maxsize=None)
def _leiden(name, resolution, objective):
    n, edges = _SETS[name]()
    stats = {}
    labels, ncl, C = refleiden.leiden(n, edges, resolution, objective, stats)
    return labels, ncl, C, stats


@functools.lru_cache(maxsize=None)
def _louvain(name):
    n, edges = _SETS[name]()
    return reflouvain.louvain(n, edges, 1.0)


_SETS = {
    "short": lambda: S.many_short_rows(NUM_CU),
    "long": lambda: S.many_long_rows(NUM_CU),
    "heavy": S.heavy_star,
    "light": lambda: S.heavy_star(1),
    "cycling": S.cycling_star,
    "nontarget": S.nontarget_star,
    "loops": S.loops_and_duplicates,
    "loops_large": S.loops_and_duplicates_large,
    "limit": S.near_limit,
}
_SETS.update({"chain_%d" % m: functools.partial(S.chain, m) for m in (8, 40, 70)})
_SETS.update({"colliding_%d" % b: functools.partial(S.colliding_star, b) for b in S.COLLIDING})
_SETS.update({k: functools.partial(S.boundary_star, length, loop) for length in S.BOUNDARY_LENGTHS for loop in (False, True)
              for k in ["star_%d%s" % (length, "_self" if loop else "")]})


def _rows(n, edges):
    """the row lengths, self entry included"""
    row = [set() for _ in range(n)]
    for u, v, _ in edges:
        row[u].add(v)
        row[v].add(u)
    return [len(r) for r in row]


def test_many_short_rows_give_the_wave_path_a_second_turn():
    n, edges = S.many_short_rows(NUM_CU)
    rows = _rows(n, edges)
    assert n == 32 * NUM_CU + 200 and min(rows) >= 1 and max(rows) <= 128
    assert sum(r > 0 for r in rows) > 32 * NUM_CU
    labels, ncl, levels, rounds, _ = _louvain("short")
    assert 1 < levels < reflouvain.MAX_LEVELS and rounds < levels * reflouvain.MAX_ROUNDS and 1 < ncl < n
    for objective, resolution in ((CPM, 0.25), (MODULARITY, 1.0)):
        _, ncl, C, stats = _leiden("short", resolution, objective)
        assert C[0] < refleiden.MAX_ITERATIONS and max(stats["levels_by_iteration"]) < refleiden.MAX_LEVELS and 1 < ncl < n
        assert len(stats["proposer_rows"]) > 32 * NUM_CU  # more proposing rows than workgroups, too


def test_many_long_rows_give_the_block_path_a_second_turn():
    n, edges = S.many_long_rows(NUM_CU)
    rows = _rows(n, edges)
    assert sum(128 < r <= 2048 for r in rows) > 3 * NUM_CU and max(rows) <= 2048
    labels, ncl, levels, rounds, _ = _louvain("long")
    assert ncl == n // S.LONG_BLOCK and all(labels[x] == x // S.LONG_BLOCK for x in range(n))
    for objective, resolution in ((CPM, 0.25), (MODULARITY, 1.0)):
        labels, ncl, C, stats = _leiden("long", resolution, objective)
        assert ncl == n // S.LONG_BLOCK
        assert sum(r > 128 for r in stats["proposer_rows"]) > 3 * NUM_CU
        assert sum(r > 128 for r in stats["proposer_rows_outside"]) > 3 * NUM_CU
        assert C[6] > 0


def test_many_long_rows_have_tied_best_scores():
    """Round 0 of level 0, every vertex alone: staying scores 0, community d < x scores w A - g B nu_x nu_d.  Rows past 128
    entries whose two best candidates score the same, under either objective: the order among equals decides them."""
    n, edges = S.many_long_rows(NUM_CU)
    adj = refleiden._adjacency(n, [r for u, v, q in edges for r in ((u, v, q), (v, u, q))])
    k = [sum(row.values()) for row in adj]
    M2 = sum(k)
    for A, gB, nu, least in ((M2 * 65536, 65536, k, 3), (65536, 16384 << 20, [1] * n, 3 * NUM_CU // 2)):
        tied = 0
        for x in range(n):
            if len(adj[x]) <= 128:
                continue
            scores = sorted((w * A - gB * nu[x] * nu[d] for d, w in adj[x].items() if d < x), reverse=True)
            tied += len(scores) >= 2 and scores[0] > 0 and scores[0] == scores[1]
        assert tied >= least


def test_heavy_star_puts_a_cpm_proposer_on_the_global_path():
    n, edges = S.heavy_star()
    assert 1 << 42 <= 2 * sum(q for _, _, q in edges) < 1 << 43
    labels, ncl, C, stats = _leiden("heavy", 0.25, CPM)
    assert ncl == 1 and sum(r > 2048 for r in stats["proposer_rows"]) >= 2 and max(stats["row_lengths"]) == 2100
    labels, ncl, C, stats = _leiden("light", 1 / 4096, CPM)
    assert ncl == 1 and sum(r > 2048 for r in stats["proposer_rows"]) >= 2
    assert any(r > 2048 for r in stats["proposer_rows_outside"])
    assert any(r > 2048 for r in _leiden("heavy", 1.0, MODULARITY)[3]["proposer_rows"])


def test_boundary_stars_have_the_rows_at_which_the_path_changes():
    for length in S.BOUNDARY_LENGTHS:
        for loop in (False, True):
            name = "star_%d%s" % (length, "_self" if loop else "")
            n, edges = S.boundary_star(length, loop)
            rows = _rows(n, edges)
            assert rows[n - 1] == max(rows) == length and sorted(set(rows))[-2] <= 2
            assert any(u == v for u, v, _ in edges) == loop
            for objective, resolution in ((CPM, 0.25), (MODULARITY, 1.0)):
                stats = _leiden(name, resolution, objective)[3]
                assert length in stats["row_lengths"] and not any(r > length for r in stats["row_lengths"])
            stats = _leiden(name, 1.0, MODULARITY)[3]
            assert length in stats["proposer_rows"]  # the centre proposes: the PROPOSE form at this length too
            assert stats["levels_by_iteration"] and _leiden(name, 1.0, MODULARITY)[2][0] < refleiden.MAX_ITERATIONS
            assert 1 < _louvain(name)[1] < n


def test_colliding_stars_wrap_round_the_end_of_a_table():
    for bits, (n_hit, n_other) in S.COLLIDING.items():
        n, edges = S.colliding_star(bits)
        rows = _rows(n, edges)
        centre = n - 1
        low, high = {8: (1, 128), 12: (129, 2048), 13: (2049, 4096)}[bits]
        assert low <= rows[centre] <= high and rows[centre] == n_hit + n_other
        weight = {u + v - centre: q for u, v, q in edges if centre in (u, v)}
        last = [y for y in weight if S.home_slot(y, bits) == (1 << bits) - 1]
        assert len(last) == n_hit >= 3 and last == [y for y in S.colliding_ids(bits) if y in weight]
        assert S.home_slot(last[0], bits) == ((last[0] * 2654435761) % (1 << 32)) >> (32 - bits)
        # round 0 at level 0, every vertex alone: the centre scores community y at w M2 65536 - g k_centre k_y
        k = [0] * n
        for u, v, q in edges:
            k[u] += q
            k[v] += q
        M2 = sum(k)
        score = {y: w * M2 * 65536 - 65536 * k[centre] * k[y] for y, w in weight.items()}
        top = max(score.values())
        best = [y for y in weight if score[y] == top]
        assert top > 0 and len(best) >= 2 and set(best) <= set(last) and min(best) != min(last)
        labels, ncl, levels, rounds, _ = _louvain("colliding_%d" % bits)
        assert ncl < n - len(weight) // 2
        assert _leiden("colliding_%d" % bits, 0.25, CPM)[1] == n
        if bits > 8:  # the centre proposes on the workgroup's and on the global table, too
            assert rows[centre] in _leiden("colliding_%d" % bits, 1.0, MODULARITY)[3]["proposer_rows"]


def test_chains_reach_the_caps():
    assert max(_leiden("chain_8", 1.0, MODULARITY)[3]["move_rounds"]) == refleiden.MAX_ROUNDS == 64
    labels, ncl, levels, rounds, _ = _louvain("chain_8")
    assert levels < 32 and rounds > 64
    labels, ncl, levels, rounds, _ = _louvain("chain_40")
    assert (levels, rounds) == (32, 2048) == (reflouvain.MAX_LEVELS, reflouvain.MAX_LEVELS * reflouvain.MAX_ROUNDS)
    labels, ncl, levels, rounds, _ = _louvain("chain_70")
    assert (levels, rounds, ncl) == (32, 2048, 36)  # the oscillation is the definition's: DESIGN 3.4h
    labels, ncl, C, stats = _leiden("chain_70", 1 / 65536, CPM)
    assert max(stats["refine_rounds"]) == 64 and max(stats["levels_by_iteration"]) == 32 and max(stats["move_rounds"]) == 64
    assert C[0] < refleiden.MAX_ITERATIONS


def test_cycling_star_reaches_the_iteration_cap():
    labels, ncl, C, stats = _leiden("cycling", 1.0, MODULARITY)
    assert C[0] == refleiden.MAX_ITERATIONS == 100 and len(stats["levels_by_iteration"]) == 100
    assert any(r > 128 for r in stats["proposer_rows"])


def test_a_proposer_meets_a_community_that_is_no_target():
    """on a short row (the chains) and on a row past 128 entries (the second level of nontarget_star)"""
    assert _leiden("chain_40", 1.0, MODULARITY)[3]["proposer_rows_nontarget"]
    stats = _leiden("nontarget", 1.0, MODULARITY)[3]
    assert any(128 < r <= 2048 for r in stats["proposer_rows_nontarget"])


def test_loops_and_duplicates_hold_their_cases():
    n, edges = S.loops_and_duplicates_large()
    pairs = {}
    for u, v, _ in edges:
        pairs[(min(u, v), max(u, v))] = pairs.get((min(u, v), max(u, v)), 0) + 1
    assert all((x, x) in pairs for x in range(n))
    assert 5 * (len(edges) - len(pairs)) >= len(edges) - 20 and sum(u > v for u, v, _ in edges) > 20
    labels, ncl, C, stats = _leiden("loops_large", 0.25, CPM)
    assert stats["ineligible"] > 0 and C[6] > 0 and labels[65] == labels[60] and 1 < ncl < n
    assert 1 < _leiden("loops_large", 1.0, MODULARITY)[1] < n and 1 < _louvain("loops_large")[1] < n
    # the same graph with every pair given once, smaller end first, is the same input
    once = {}
    for u, v, q in edges:
        once[(min(u, v), max(u, v))] = once.get((min(u, v), max(u, v)), 0) + q
    assert max(once.values()) < 1 << 32
    merged = [(u, v, q) for (u, v), q in sorted(once.items())]
    assert refleiden.leiden(n, merged, 0.25, CPM)[:2] == (labels, ncl)
    assert reflouvain.louvain(n, merged, 1.0)[:4] == _louvain("loops_large")[:4]
    n, edges = S.loops_and_duplicates()
    assert any(u == v for u, v, _ in edges) and any(u > v for u, v, _ in edges) and 1 < _louvain("loops")[1] < n


def test_near_limit_is_within_2_to_the_20_of_the_limit():
    n, edges = S.near_limit()
    M2 = 2 * sum(q for _, _, q in edges)
    assert (1 << 46) - (1 << 20) <= M2 < 1 << 46 and max(q for _, _, q in edges) < 1 << 32 and n > 3
    assert _louvain("limit")[0] == [0] * 6 + [1] * 6
    assert _leiden("limit", 1.0, MODULARITY)[0] == [0] * 6 + [1] * 6
    assert refleiden.leiden(n, edges, 65535, MODULARITY)[1] == n and refleiden.leiden(n, edges, 65535, CPM)[1] == 2


# ---- wrong rules: each must show on one of the sets ----
def _variant(module, *swaps):
    """the restatement with lines of its text replaced; every line to replace must be there"""
    src = open(module.__file__).read()
    for old, new, count in swaps:
        assert src.count(old) == count, old
        src = src.replace(old, new)
    mod = types.ModuleType(module.__name__ + "_variant")
    exec(compile(src, module.__file__, "exec"), mod.__dict__)
    return mod


_LARGER = ("for d in sorted(e):", "for d in sorted(e, reverse=True):")
_ROUNDS = ("MAX_ROUNDS = 64", "MAX_ROUNDS = 63", 1)
_LEVELS = ("MAX_LEVELS = 32", "MAX_LEVELS = 31", 1)
LOUVAIN_VARIANTS = {
    "ties_to_the_larger_id": ([_LARGER + (1,)], ["heavy", "colliding_8", "colliding_12", "colliding_13", "limit"]),
    "self_entry_counted": ([("                if y != x:\n", "                if True:\n", 1)], ["loops_large", "star_128_self", "star_2049_self"]),
    "cap_of_63_rounds": ([_ROUNDS], ["chain_8"]),
    "cap_of_31_levels": ([_LEVELS], ["chain_40"]),
}
LEIDEN_VARIANTS = {
    "ties_to_the_larger_id": ([_LARGER + (2,)], [("long", 0.25, CPM), ("long", 1.0, MODULARITY), ("heavy", 0.25, CPM)]),
    # the restatement's own assertion that a refined community stays inside a coarse one goes with the filter
    "no_coarse_filter": ([("                if y != x and coarse[y] == coarse[x]:\n                    e[R[y]]", "                if y != x:\n                    e[R[y]]", 1),
                          ("        assert all(coarse[x] == coarse[r] for x in ms)\n", "", 1)],
                         [("long", 1.0, MODULARITY), ("light", 1 / 4096, CPM)]),
    "no_target_filter": ([(" or not target[d]", "", 1)], [("nontarget", 1.0, MODULARITY), ("heavy", 1.0, MODULARITY), ("chain_40", 1.0, MODULARITY)]),
    "self_entry_counted_in_a_move": ([("                if y != x:\n                    e[comm[y]]", "                if True:\n                    e[comm[y]]", 1)],
                                     [("loops_large", 0.25, CPM), ("loops_large", 1.0, MODULARITY), ("star_2049_self", 1.0, MODULARITY)]),
    "self_entry_counted_in_eligibility": ([("if y != x and coarse[y] == coarse[x]) for x in range(n)]", "if coarse[y] == coarse[x]) for x in range(n)]", 1)],
                                          [("loops_large", 0.25, CPM), ("nontarget", 1.0, MODULARITY)]),
    "cap_of_63_rounds": ([_ROUNDS], [("chain_8", 1.0, MODULARITY), ("chain_70", 1 / 65536, CPM)]),
    "cap_of_31_levels": ([_LEVELS], [("chain_70", 1 / 65536, CPM), ("chain_40", 1.0, MODULARITY)]),
}


def test_wrong_rules_change_the_answer():
    for rule, (swaps, names) in LOUVAIN_VARIANTS.items():
        wrong = _variant(reflouvain, *swaps)
        for name in names:
            n, edges = _SETS[name]()
            assert wrong.louvain(n, edges, 1.0)[:4] != _louvain(name)[:4], (rule, name)
    for rule, (swaps, cases) in LEIDEN_VARIANTS.items():
        wrong = _variant(refleiden, *swaps)
        for name, resolution, objective in cases:
            n, edges = _SETS[name]()
            labels, ncl, C = wrong.leiden(n, edges, resolution, objective)
            assert (labels, ncl, C[:7]) != _leiden(name, resolution, objective)[:2] + (_leiden(name, resolution, objective)[2][:7],), (rule, name)
