"""GPU suite: rtc_rep_screen against the restatement of its definition (tests/refscreen.py) on the generated set of
tests/screen_sets.py -- every gather path, the forced global path, chunking, the halving of a chunk that does not fit, the refusal
of a sample that does not fit alone, the live mask and the argument errors -- and clust-mst --db --screen end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import refmststate as M
import refscreen as R
import screen_sets as S
from test_gpu_mst_state import _folders, _genomes, _run, _sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")

_SETS = {}


def _device_set(ctx, width):
    """the generated set on the device, uploaded once per width"""
    from rabbittclust_amd import api
    if width not in _SETS:
        reps, samples, live = S.generated()
        _SETS[width] = (api.SketchSet.from_host(S.as_width(reps, width) + S.as_width(samples, width), ctx.device, k=21, kind="kssd", width=width),
                        len(reps), live)
    return _SETS[width]


def _tuples(a):
    return [tuple(int(x) for x in r) for r in a]


def _want(config):
    hits, sums, info = S.reference(config)
    return R.flat(hits), [s + (0,) for s in sums], info


@pytest.mark.gpu
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("config", S.CONFIGS)
def test_rep_screen_equals_the_definition(ctx, width, config):
    from rabbittclust_amd import api
    sk, R_, live = _device_set(ctx, width)
    want_hits, want_sums, info = _want(config)
    mc, cont, mu, picks = config
    nq = len(want_sums)
    with_cand = sum(1 for s in want_sums if s[3])
    for chunk in (0, 2):
        hits, sums = ctx.rep_screen(sk, R_, mc, cont, mu, picks, live=live, query_chunk=chunk)
        assert _tuples(sums) == want_sums, (config, chunk)
        assert _tuples(hits) == want_hits, (config, chunk)
        cnt = ctx.rep_screen_counters()
        assert cnt["chunks"] == (1 if chunk == 0 else (nq + 1) // 2)
        assert cnt["wave_queries"] + cnt["workgroup_queries"] + cnt["global_queries"] == with_cand
        assert cnt["eligible"] == len(want_hits) and cnt["picks"] == sum(s[4] for s in want_sums)
        assert cnt["rounds_max"] == max(i["rounds"] for i in info) and cnt["matches"] == sum(i["matches"] for i in info)
        assert cnt["candidates"] >= cnt["eligible"]
        if config == S.CONFIGS[0]:
            assert ctx.rep_screen_last_path() == api.SCREEN_PATH_WAVE | api.SCREEN_PATH_BLOCK | api.SCREEN_PATH_GLOBAL
            assert cnt["wave_queries"] >= 1 and cnt["workgroup_queries"] >= 1 and cnt["global_queries"] >= 2


@pytest.mark.gpu
def test_a_short_buffer_returns_the_count_and_complete_sums(ctx):
    from rabbittclust_amd import api
    sk, R_, live = _device_set(ctx, 4)
    want_hits, want_sums, _ = _want(S.CONFIGS[0])
    cap = 100
    assert len(want_hits) > cap
    out = np.zeros(cap, dtype=api.SCREEN_HIT_DT)
    sums = np.zeros(len(want_sums), dtype=api.SCREEN_SUM_DT)
    lv = np.ascontiguousarray(live, dtype=np.uint8)
    n = C.c_uint64()
    ctx.check(ctx.lib.rtc_rep_screen(ctx.h, C.c_void_p(sk.hashes.data_ptr()), sk.width, C.c_void_p(sk.start.data_ptr()), C.c_void_p(sk.len.data_ptr()),
                                     R_, len(want_sums), lv.ctypes.data_as(C.c_void_p), 1, 0, 1, 0, 0, out.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                     sums.ctypes.data_as(C.c_void_p)))
    assert n.value == len(want_hits) and _tuples(out) == want_hits[:cap] and _tuples(sums) == want_sums


@pytest.mark.gpu
@pytest.mark.parametrize("width", [4, 8])
def test_forced_global_path_is_identical(ctx, width):
    from rabbittclust_amd import api
    sk, R_, live = _device_set(ctx, width)
    for config in S.CONFIGS[:2]:
        want_hits, want_sums, _ = _want(config)
        with ctx.env(RTC_SCREEN_GLOBAL="1"):
            hits, sums = ctx.rep_screen(sk, R_, *config, live=live)
            assert ctx.rep_screen_last_path() == api.SCREEN_PATH_GLOBAL
            cnt = ctx.rep_screen_counters()
            assert cnt["wave_queries"] == cnt["workgroup_queries"] == 0 and cnt["global_queries"] == sum(1 for s in want_sums if s[3])
        assert _tuples(hits) == want_hits and _tuples(sums) == want_sums


def _need(info, samples, qs):
    from rabbittclust_amd import api
    return sum(len(samples[q]) for q in qs) * api.SCREEN_POS_BYTES + sum(info[q]["matches"] for q in qs) * api.SCREEN_MATCH_BYTES


@pytest.mark.gpu
def test_a_chunk_that_does_not_fit_is_halved(ctx):
    from rabbittclust_amd import _lib
    sk, R_, live = _device_set(ctx, 4)
    _, samples, _ = S.generated()
    want_hits, want_sums, info = _want(S.CONFIGS[0])
    every = range(len(samples))
    largest = max(_need(info, samples, [q]) for q in every)
    assert largest < _need(info, samples, every), "one sample needs what all need: nothing to halve"
    with ctx.env(RTC_SCREEN_BYTES=str(largest)):  # every sample fits alone, all of them together do not
        hits, sums = ctx.rep_screen(sk, R_, *S.CONFIGS[0], live=live)
        assert ctx.rep_screen_counters()["chunks"] > 1
    assert _tuples(hits) == want_hits and _tuples(sums) == want_sums
    # a sample that does not fit alone: RTC_ERR_NOMEM with a message, no crash, no wait
    with ctx.env(RTC_SCREEN_BYTES=str(largest - 1)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.rep_screen(sk, R_, *S.CONFIGS[0], live=live)
        assert e.value.status == _lib.RTC_ERR_NOMEM and "RTC_SCREEN_BYTES" in str(e.value)
    hits, sums = ctx.rep_screen(sk, R_, *S.CONFIGS[0], live=live)  # the context works on
    assert _tuples(hits) == want_hits


@pytest.mark.gpu
def test_live_mask_empty_sides_and_argument_errors(ctx):
    from rabbittclust_amd import _lib, api
    reps, x = S.hand()
    hand = api.SketchSet.from_host(S.as_width(reps + x, 8), ctx.device, k=21, kind="kssd", width=8)
    want, wsum, _ = R.screen(reps, x, 1, 0, 2, 0)
    hits, sums = ctx.rep_screen(hand, 4, 1, 0, 2, 0)  # live None
    assert _tuples(hits) == R.flat(want) and _tuples(sums) == [wsum[0] + (0,)]
    hits1, sums1 = ctx.rep_screen(hand, 4, 1, 0, 2, 0, live=[1, 1, 1, 1])
    assert _tuples(hits1) == _tuples(hits) and _tuples(sums1) == _tuples(sums)
    hits, sums = ctx.rep_screen(hand, 4, 1, 0, 1, 0, live=[0, 1, 1, 1])
    w2, s2, _ = R.screen(reps, x, 1, 0, 1, 0, live=[0, 1, 1, 1])
    assert _tuples(hits) == R.flat(w2) and _tuples(sums) == [s2[0] + (0,)]
    hits, sums = ctx.rep_screen(hand, 4, 1, 0, 1, 0, live=[0, 0, 0, 0])
    assert len(hits) == 0 and _tuples(sums) == [(10, 0, 0, 0, 0, 0)]
    assert ctx.rep_screen_last_path() == 0
    # no sample, no representative
    only_reps = api.SketchSet.from_host(S.as_width(reps, 4), ctx.device, k=21, kind="kssd", width=4)
    hits, sums = ctx.rep_screen(only_reps, 4)
    assert len(hits) == 0 and len(sums) == 0
    hits, sums = ctx.rep_screen(only_reps, 0)
    assert len(hits) == 0 and _tuples(sums) == [(len(r), 0, 0, 0, 0, 0) for r in reps]
    # the argument errors
    out = np.zeros(64, dtype=api.SCREEN_HIT_DT)
    sm = np.zeros(4, dtype=api.SCREEN_SUM_DT)
    n = C.c_uint64()

    def call(width=8, n_reps=4, nq=1, min_unique=1, cont=0, h_sum=True):
        return ctx.lib.rtc_rep_screen(ctx.h, C.c_void_p(hand.hashes.data_ptr()), width, C.c_void_p(hand.start.data_ptr()), C.c_void_p(hand.len.data_ptr()),
                                      n_reps, nq, None, 1, cont, min_unique, 0, 0, out.ctypes.data_as(C.c_void_p), 64, C.byref(n),
                                      sm.ctypes.data_as(C.c_void_p) if h_sum else None)
    assert call() == _lib.RTC_OK and n.value == 4
    assert call(min_unique=0) == _lib.RTC_ERR_ARG
    assert call(cont=(1 << 20) + 1) == _lib.RTC_ERR_ARG
    assert call(cont=1 << 20) == _lib.RTC_OK
    assert call(h_sum=False) == _lib.RTC_ERR_ARG
    assert call(nq=0, h_sum=False) == _lib.RTC_OK and n.value == 0
    assert call(width=2) == _lib.RTC_ERR_ARG
    assert call(n_reps=(1 << 31) - 2, nq=1) == _lib.RTC_ERR_ARG
    assert b"rtc_rep_screen" in ctx.lib.rtc_last_error(ctx.h)


def _fasta(path, seqs):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">rec%d\n" % i + s.tobytes() + b"\n")
    return path


@pytest.mark.gpu
def test_screen_end_to_end(oracle, tmp_path):
    tmp = str(tmp_path)
    mst = os.path.join(BIN, "clust-mst")
    lst, paths, seqs = _genomes(oracle, tmp, "a", 3, 4, 300_000, seed=41)
    db = os.path.join(tmp, "rep.mstdb")
    _run([mst, "--fast", "--db", db, "--build", "-l", "-i", lst, "-k", "21", "-d", "0.05", "-t", "4", "-o", os.path.join(tmp, "b.out")], tmp)
    assert _folders(tmp) == []
    st, _ = M.parse(open(db, "rb").read())
    assert st.kssd and len(st.rep_hashes) < len(paths), "every cluster is a singleton: the test shows nothing"
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    mix = [seqs[0], seqs[8][:150_000], acgt[rng.integers(0, 4, size=200_000)]]
    noise = [acgt[rng.integers(0, 4, size=250_000)]]
    samples = [_fasta(os.path.join(tmp, "mix.fna"), mix), _fasta(os.path.join(tmp, "noise.fna"), noise)]
    lst_s = os.path.join(tmp, "samples.txt")
    open(lst_s, "w").write("\n".join(samples) + "\n")
    # the oracle's sketch of a file: the union of its records' sketches (no k-mer spans two records)
    qsk = [sorted(set().union(*[set(int(h) for h in _sketch(oracle, [r], st)[0]) for r in recs])) for recs in (mix, noise)]
    live = [1 if c else 0 for c in st.clusters]
    ids, k = [], 0
    for c in st.clusters:
        ids.append(k if c else -1)
        k += 1 if c else 0
    sizes = [len(c) for c in st.clusters]
    reps = [[int(h) for h in r] for r in st.rep_hashes]
    out = os.path.join(tmp, "screen.tsv")
    err = _run([mst, "--fast", "--db", db, "--screen", "-l", "-i", lst_s, "-t", "4", "-o", out], tmp)
    assert "time of rep screen (GPU)" in err
    hits, sums, _ = R.screen(reps, qsk, 2, int(round(0.05 * R.Q20)), 2, 0, live)
    assert open(out).read() == R.screen_tsv(samples, st.rep_names, ids, sizes, hits, sums, st.kmer_size)
    assert open(out + ".summary.tsv").read() == R.summary_tsv(samples, sums)
    fams = [set(g // 4 for g in st.clusters[s]) for s, _, _, _, rank in hits[0] if rank]  # genome g is of family g // 4
    assert all(len(f) == 1 for f in fams) and set().union(*fams) == {0, 2}, "the mixture holds family 0 and family 2, and nothing of family 1"
    assert not hits[1] and ("%s\t0\t-1\tno_match\t" % samples[1]) in open(out).read()
    # other thresholds, the flags as spelled; and the records of one FASTA file as samples named query_<i>
    out2 = os.path.join(tmp, "screen2.tsv")
    _run([mst, "--fast", "--db", db, "--screen", "-l", "-i", lst_s, "--min-containment", "0.3", "--min-shared", "5", "--min-unique", "3",
          "--screen-picks", "1", "-t", "4", "-o", out2], tmp)
    hits2, sums2, _ = R.screen(reps, qsk, 5, int(round(0.3 * R.Q20)), 3, 1, live)
    assert open(out2).read() == R.screen_tsv(samples, st.rep_names, ids, sizes, hits2, sums2, st.kmer_size) and sums2[0][4] == 1
    out3 = os.path.join(tmp, "screen3.tsv")
    _run([mst, "--fast", "--db", db, "--screen", "-i", samples[0], "-t", "4", "-o", out3], tmp)
    rsk = [[int(h) for h in _sketch(oracle, [r], st)[0]] for r in mix]
    hits3, sums3, _ = R.screen(reps, rsk, 2, int(round(0.05 * R.Q20)), 2, 0, live)
    assert open(out3).read() == R.screen_tsv([""] * 3, st.rep_names, ids, sizes, hits3, sums3, st.kmer_size)
    assert open(out3 + ".summary.tsv").read() == R.summary_tsv([""] * 3, sums3)
