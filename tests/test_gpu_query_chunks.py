"""The candidate list that is too short on the first attempt (csrc/rtc_query_chunks.h): 24 queries against 3 000 model sketches
that all hold one hub hash give 72 000 candidates in one chunk, past the list's first room of max(65 536, 24 * 64) records, so
the join runs a second time into a list grown to the count.  Every one of the four placement entry points goes through it once
and must return what its brute-force restatement gives.  Every pair shares the hub alone, so every key is 1 / 7 and the order
among them is the tie rule's (the lower model index); integers only, no tolerances."""
import ctypes as C

import numpy as np
import pytest

import refmstdb as D
import refmststate as M
from tests import refdbscan_assign as A
from tests import refleiden_assign as L

pytestmark = pytest.mark.gpu

K = 21
N_MODEL, N_QUERY = 3000, 24
CANDIDATES = N_MODEL * N_QUERY  # 72 000 > 65 536
HUB = 7


def _sketches():
    """the hub plus three hashes of its own per sketch, model first"""
    return [np.array([HUB, 1000 + 3 * g, 1001 + 3 * g, 1002 + 3 * g], dtype=np.int64) for g in range(N_MODEL + N_QUERY)]


def _set(ctx, sketches, width, kind):
    from rabbittclust_amd import api
    dt = np.uint32 if width == 4 else np.uint64
    return api.SketchSet.from_host([s.astype(dt) for s in sketches], ctx.device, k=K, kind=kind, width=width)


def test_rep_match_regrows_the_candidate_list(ctx):
    from rabbittclust_amd import api
    sk = _sketches()
    s = _set(ctx, sk, 8, "minhash")
    # 1 / 7 is a distance of ln(4) / 21 = 0.066: every (query, model) pair and every pair of queries passes at 0.1
    want = M.brute_pairs(sk, N_MODEL, 0.1, K, False, False)
    assert len(want) == CANDIDATES + N_QUERY * (N_QUERY - 1) // 2
    # through the ABI with room for every pair: Context.rep_match would call twice, the first time to learn the count
    out = np.zeros(len(want), dtype=api.REP_PAIR_DT)
    n = C.c_uint64()
    d0 = ctx.diag()["repmatch_chunks"]
    ctx.check(ctx.lib.rtc_rep_match(ctx.h, api._t_ptr(s.hashes), s.width, api._t_ptr(s.start), api._t_ptr(s.len), N_MODEL, N_QUERY, K, 0, 0,
                                    0.1, 0, api._np_ptr(out), len(out), C.byref(n)))
    assert ctx.diag()["repmatch_chunks"] - d0 == 1
    assert n.value == len(want)
    assert [(int(g["query"]), int(g["slot"]), int(g["common"])) for g in out] == [(q, sl, c) for q, sl, c, _ in want]
    assert [float(g["dist"]) for g in out] == [d for *_, d in want]


def test_rep_topk_regrows_the_candidate_list(ctx):
    sk = _sketches()
    s = _set(ctx, sk, 4, "minhash")
    want = D.topk(sk[:N_MODEL], sk[N_MODEL:], 0, 5)
    assert all(h == [(p, 1, 7) for p in range(5)] for h in want)
    got, per = ctx.rep_topk(s, N_MODEL, 0, 5)
    assert per.tolist() == [5] * N_QUERY
    assert [tuple(int(x) for x in g) for g in got] == [(q, sl, c, d) for q, h in enumerate(want) for sl, c, d in h]
    c = ctx.rep_topk_counters()
    assert c["chunks"] == 1 and c["candidates"] == CANDIDATES
    assert ctx.rep_topk_last_path() == 1


def test_dbscan_assign_regrows_the_candidate_list(ctx):
    sk = _sketches()
    model, queries = sk[:N_MODEL], sk[N_MODEL:]
    s = _set(ctx, sk, 4, "kssd")
    # the rule takes any labelling: labels and core flags that make min, max and the core count differ from each other
    rng = np.random.default_rng(3)
    labels = rng.integers(2, 9, N_MODEL).astype(np.int32)
    core = rng.random(N_MODEL) < 0.5
    eps, min_pts = 0.1, 5  # t = 0.065: 1 (1 + t) >= 8 t, every model point is a neighbour of every query
    want = A.place_all(model, labels, core, queries, eps, min_pts, K)
    assert want["n_neighbours"].tolist() == [N_MODEL] * N_QUERY and want["nearest"].tolist() == [0] * N_QUERY
    assert 0 < want["n_core"][0] < N_MODEL and want["label"][0] != want["label_max"][0]
    got = ctx.dbscan_assign(s, N_MODEL, labels, core, eps, min_pts, K)
    for f in A.PLACE_DT.names:
        assert got[f].tolist() == want[f].tolist(), f
    c = ctx.dbscan_assign_counters()
    assert c["chunks"] == 1 and c["candidates"] == CANDIDATES and c["fold_paths"] == 1


def test_graph_query_regrows_the_candidate_list(ctx):
    sk = _sketches()
    model, queries = sk[:N_MODEL], sk[N_MODEL:]
    s = _set(ctx, sk, 8, "kssd")
    want_e, want_n = L.graph_query(model, queries, 0.1, K, 5)  # J* = 0.065 < 1 / 7: every candidate passes, five are kept
    assert want_n == [(0, 1, 7, N_MODEL, N_MODEL, 5)] * N_QUERY
    got_e, got_n = ctx.graph_query(s, N_MODEL, 0.1, K, 5)
    assert [(int(r["q"]), int(r["p"]), int(r["common"])) for r in got_e] == want_e
    assert [tuple(int(x) for x in r) for r in got_n.tolist()] == want_n
    c = ctx.graph_query_counters()
    assert c["chunks"] == 1 and c["candidates"] == CANDIDATES and c["passing"] == CANDIDATES and c["kept"] == 5 * N_QUERY
