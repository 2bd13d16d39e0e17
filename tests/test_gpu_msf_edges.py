"""GPU suite: the Boruvka forest kernels of rtc_mst.hip (boruvka_minkey / minweight / minedge / fetch / hook / relabel_reset with
wave_min_update) and the forest sort of rtc_sort.hip against the exact forest of tests/refmsf.py, edge for edge, on the graphs of
tests/msf_sets.py (tests/test_cpu_msf_sets.py shows what each is for and that the sets tell wrong rules from right ones).

One call (rtc_msf_dev through Context.msf) has to leave the reference's records in the reference's order and report its round
count, whatever the order of the list; the per-round primitives (pipeline.HipBoruvkaBackend under pipeline.boruvka_rounds, the
multi-GPU form) have to give the same forest and rounds alone and with the list cut into 2 and 5 parts that run in lockstep.
Every comparison is equality of integers.  Each case prints what the reference and the GPU calls took."""
import time

import numpy as np
import pytest

import msf_sets as S
import refmsf

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(ctx, name):
    """(n, edges, lens, wmode, the forest int64 [f, 3] in (key, i, j) order, rounds, seconds the reference took), once"""
    if name not in _REF:
        n, e, lens, wmode = S.case(name, ctx.num_cu())
        t0 = time.perf_counter()
        want = refmsf.sorted_list(e, lens, wmode) if name in S.IS_FOREST else refmsf.forest(n, e, lens, wmode)
        rounds = refmsf.rounds(n, e, lens, wmode)
        _REF[name] = (n, e, lens, wmode, want, rounds, time.perf_counter() - t0)
    return _REF[name]


def _records(rec):
    return np.stack([rec["i"], rec["j"], rec["common"]], axis=1).astype(np.int64).reshape(-1, 3)


@pytest.mark.parametrize("name", S.names())
def test_one_call_leaves_the_exact_forest_in_order(ctx, name):
    n, e, lens, wmode, want, want_rounds, ref_s = _ref(ctx, name)
    for edges in (e, S.reordered(e, name)):
        t0 = time.perf_counter()
        rec, rounds = ctx.msf(edges, lens, wmode)
        t1 = time.perf_counter()
        print("%s: n %d, %d edges, forest %d / %d, rounds %d / %d, reference %.2f s, call with copies %.3f s"
              % (name, n, len(e), len(rec), len(want), rounds, want_rounds, ref_s, t1 - t0))
        assert np.array_equal(_records(rec), want)
        assert rounds == want_rounds


class _Sizes:
    """what HipBoruvkaBackend reads of a sketch set"""

    def __init__(self, ctx, lens):
        import torch
        self.n = len(lens)
        self.len = torch.from_numpy(lens.view(np.int32).copy()).to(ctx.device)


def _fused_size(ctx, n, lens):
    if n < 2 or int(lens.min()) != int(lens.max()) or int(lens[0]) == 0:
        return 0
    return int(lens[0]) if ctx.lib.rtc_boruvka_key_bits(n, int(lens[0])) else 0


@pytest.mark.parametrize("parts", [1, 2, 5])
@pytest.mark.parametrize("name", [name for name in S.names() if name not in S.LARGEST])
def test_round_primitives_alone_and_in_lockstep_parts(ctx, name, parts):
    """fused (one reduction a round) where the sizes are equal and the key fits, and three passes (three reductions) always"""
    import torch
    from rabbittclust_amd import pipeline
    from test_gpu_mst import _LockstepRanks
    n, e, lens, wmode, want, want_rounds, _ = _ref(ctx, name)
    want_set = sorted(map(tuple, want.tolist()))
    sizes = _Sizes(ctx, lens)
    cuts = [0] + sorted(np.random.default_rng(parts).integers(0, len(e) + 1, size=parts - 1).tolist()) + [len(e)]
    fused = _fused_size(ctx, n, lens)
    for s_fixed in [0] + ([fused] if fused else []):
        backends = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            dev = torch.from_numpy(np.ascontiguousarray(e[a:b]).copy()).to(ctx.device).reshape(-1, 3)
            backends.append(pipeline.HipBoruvkaBackend(ctx, sizes, dev, b - a, wmode))
        ranks = _LockstepRanks(backends) if parts > 1 else backends[0]
        t0 = time.perf_counter()
        sel, rounds = pipeline.boruvka_rounds(ranks, n, None, s_fixed)
        print("%s in %d parts %s, s_fixed %d: forest %d / %d, rounds %d / %d, %.3f s"
              % (name, parts, cuts, s_fixed, len(sel), len(want), rounds, want_rounds, time.perf_counter() - t0))
        assert sorted(map(tuple, _records(sel).tolist())) == want_set
        assert rounds == want_rounds
        if parts > 1:
            assert ranks.reduces == (rounds if s_fixed else 3 * rounds)
        elif n <= 256:
            # one workgroup: the hook pass appends by the id of the recording root, so which root a mutual hook keeps shows
            from test_cpu_distributed import NumpyBoruvkaBackend
            with np.errstate(all="ignore"):  # (its own keys divide by a denom of 0; replaced in the next line)
                host = NumpyBoruvkaBackend(e.astype(np.int64), lens, (wmode & 3) == 1, n)
            host.key = refmsf.keys(e, lens, wmode)
            raw, _ = pipeline.boruvka_rounds(host, n, None, s_fixed)
            assert np.array_equal(_records(sel), _records(raw))
