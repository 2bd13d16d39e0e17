"""CPU suite: the clust-mst --save-rep state without a GPU -- the state file's layout through the host library, the replay of
the append's decisions on hand-built match lists, and the filters' integer truncation -- against tests/refmststate.py."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

import refmststate as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTLIB = os.path.join(ROOT, "rabbittclust_amd", "librtclust_host.so")


def _lib():
    if not os.path.exists(HOSTLIB):
        pytest.fail("librtclust_host.so missing: run __graft_entry__.build()")
    lib = C.CDLL(HOSTLIB)
    lib.rtch_mst_state_resave.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.rtch_mst_state_append.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_long, C.c_char_p, C.c_char_p]
    return lib


def _state(kssd, use64, n_reps, seed, s=40):
    rng = random.Random(seed)
    st = M.State(kssd)
    st.use64 = use64
    st.threshold, st.kmer_size = 0.05, 22 if kssd else 21
    if kssd:
        st.half_k, st.half_subk, st.drlevel = 11, 6, 3
    st.N = 3 * n_reps
    hmax = (1 << 63) if use64 else (1 << 31)
    for r in range(n_reps):
        st.rep_ids.append(3 * r + 1)
        st.rep_lens.append(1_000_000 + r)
        st.rep_names.append("/data/rep%d.fna" % r)
        st.rep_hashes.append(sorted(rng.sample(range(1, hmax), s)))
        st.clusters.append([3 * r, 3 * r + 1, 3 * r + 2])
    st.member_names = ["/data/g%d.fna" % i for i in range(st.N)]
    st.member_lens = [500_000 + 7 * i for i in range(st.N)]
    return st


@pytest.mark.parametrize("kssd,use64", [(False, True), (True, False), (True, True)])
def test_state_round_trip_matches_the_byte_layout(tmp_path, kssd, use64):
    lib = _lib()
    st = _state(kssd, use64, 5, seed=3)
    n_idx = len(M._index(st))
    shuffled = M.save(st, index_order=list(reversed(range(n_idx))))  # the reference's index order is phmap's
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(shuffled)
    assert lib.rtch_mst_state_resave(str(src).encode(), str(dst).encode(), int(kssd)) == 0
    got = dst.read_bytes()
    st2, idx2 = M.parse(got)
    st1, idx1 = M.parse(shuffled)
    assert st2.fields() == st1.fields() == st.fields()
    assert idx2 == idx1
    assert got == M.save(st)  # keys ascending
    # the other magic, a cut file and a missing one do not load (the command line then falls back)
    assert lib.rtch_mst_state_resave(str(src).encode(), str(dst).encode(), int(not kssd)) == 1
    (tmp_path / "cut.bin").write_bytes(shuffled[:len(shuffled) - 9])
    assert lib.rtch_mst_state_resave(str(tmp_path / "cut.bin").encode(), str(dst).encode(), int(kssd)) == 1
    assert lib.rtch_mst_state_resave(str(tmp_path / "none.bin").encode(), str(dst).encode(), int(kssd)) == 1


REP_PAIR = np.dtype([("query", "<u4"), ("slot", "<u4"), ("common", "<u4"), ("pad", "<u4"), ("dist", "<f8")])


def _replay(tmp_path, st, pairs, n_q, tag):
    """the host library's replay and the restatement's on one state and match list: cluster text and saved state"""
    lib = _lib()
    src = tmp_path / ("%s.bin" % tag)
    src.write_bytes(M.save(st))
    rng = random.Random(n_q)
    names = ["/data/new%d.fna" % q for q in range(n_q)]
    lens = [2_000_000 + q for q in range(n_q)]
    qh = [sorted(rng.sample(range(1, 1 << 31), 30)) for _ in range(n_q)]
    dt = np.uint64 if st.use64 else np.uint32
    flat = np.array([h for hs in qh for h in hs], dtype=dt)
    off = np.array([0] + list(np.cumsum([len(h) for h in qh])), dtype=np.uint64)
    pairs = sorted(pairs)  # rtc_rep_match's order
    pa = np.zeros(max(len(pairs), 1), dtype=REP_PAIR)
    for i, (q, s, c, d) in enumerate(pairs):
        pa[i] = (q, s, c, 0, d)
    cn = (C.c_char_p * n_q)(*[n.encode() for n in names])
    ln = np.array(lens, dtype=np.uint64)
    out, out_st = tmp_path / ("%s.cluster" % tag), tmp_path / ("%s.after.bin" % tag)
    nlive = lib.rtch_mst_state_append(str(src).encode(), int(st.kssd), n_q, cn, ln.ctypes.data, flat.ctypes.data, off.ctypes.data,
                                      pa.ctypes.data, len(pairs), str(out).encode(), str(out_st).encode())
    live = M.replay(st, names, lens, qh, pairs)
    assert nlive == len(live)
    assert out.read_text() == M.cluster_text(live, st.member_names, st.member_lens, st.sketch_by_file, st.threshold)
    assert out_st.read_bytes() == M.save(st)
    return live, st


def test_replay_merges_three_clusters_into_the_closest(tmp_path):
    st = _state(False, True, 4, seed=5)
    # query 0 matches representatives 0, 1, 2: 1 is the closest, 0 and 2 are merged into it (union by rank decides the slot)
    live, st = _replay(tmp_path, st, [(0, 0, 30, 0.03), (0, 1, 35, 0.01), (0, 2, 31, 0.02)], 1, "three")
    assert len(live) == 2
    assert sorted(live[0]) == sorted([0, 1, 2, 3, 4, 5, 6, 7, 8, 12])
    assert live[1] == [9, 10, 11]
    assert len(st.rep_hashes) == 2  # compacted


def test_replay_redirects_merged_away_reps_and_needs_the_roots_own_hits(tmp_path):
    st = _state(False, True, 3, seed=6)
    pairs = [(0, 0, 30, 0.02), (0, 1, 30, 0.01),  # 0 and 1 merge; with equal ranks slot 0 becomes the root
             (1, 1, 30, 0.01),                    # only the merged-away slot 1: its root 0 has no own hit -> a new cluster
             (2, 0, 30, 0.04), (2, 1, 39, 0.001)]  # the root's own count decides, not the closer merged-away one
    live, st = _replay(tmp_path, st, pairs, 3, "redirect")
    assert [len(c) for c in live] == [8, 3, 1]
    assert live[0][-1] == 11 and live[2] == [10]


def test_replay_query_that_became_a_rep_is_matched_later(tmp_path):
    st = _state(True, False, 2, seed=7)
    R = 2
    pairs = [(1, R + 0, 28, 0.01),  # query 0 matched nothing: slot R + 0 is its representative
             (2, R + 1, 28, 0.01),  # query 1 joined query 0's cluster: slot R + 1 never became one
             (3, R + 0, 20, 0.03), (3, 0, 25, 0.02)]
    live, st = _replay(tmp_path, st, pairs, 4, "became")
    # query 2's only pair names query 1, which never became a representative: a cluster of its own.  Query 3 is closest to
    # representative 0 and merges query 0's cluster into it; equal ranks leave query 0's slot as the root
    assert live == [[3, 4, 5], [6, 7, 0, 1, 2, 9], [8]]


def test_replay_ties_go_to_the_lowest_slot(tmp_path):
    st = _state(False, True, 3, seed=8)
    live, st = _replay(tmp_path, st, [(0, 2, 30, 0.02), (0, 0, 30, 0.02)], 1, "tie")
    # slot 0 survives, slot 2 merges into it: equal ranks, so slot 2 ends as the root (UnionFind.h) and slot 0's members follow
    assert live == [[3, 4, 5], [6, 7, 8, 0, 1, 2, 9]]


def test_min_common_needed_and_radio_truncation():
    t, k = 0.05, 21
    jmin = M.jaccard_min(t, k)
    assert jmin == pytest.approx(math.exp(-t * k) / (2 - math.exp(-t * k)))
    # Mash form: (int)(jmin (q + r) / (1 + jmin)); find sizes where the real value sits just above an integer
    for q in range(900, 1100):
        v = jmin * (q + 1000) / (1.0 + jmin)
        assert M.min_common_needed(jmin, q, 1000, False) == int(v) == math.floor(v)
        if v - math.floor(v) > 0.97:  # truncation, not rounding: one less than the rounded value passes
            assert M.min_common_needed(jmin, q, 1000, False) == round(v) - 1
    # containment form on the smaller sketch
    assert M.min_common_needed(jmin, 700, 1000, True) == int(jmin * 700)
    # the KSSD size ratio: exp(t k) (not the MST's 2 e^(t (k - 1)) - 1); sizes exactly at the limit are kept
    rad = M.radio(t, 22)
    assert rad == pytest.approx(math.exp(t * 22))
    r = 1000
    q_hi = int(math.floor(rad * r))
    assert M.ratio_ok(q_hi, r, rad) and not M.ratio_ok(q_hi + 1, r, rad)
    assert M.ratio_ok(r, q_hi, rad) and not M.ratio_ok(r, q_hi + 1, rad)
    # keep(): one hit below min_common_needed is dropped; a few above it pass the distance too
    need = M.min_common_needed(M.jaccard_min(0.05, k), 1000, 1000, False)
    assert M.keep(need - 1, 1000, 1000, 0.05, k, False, False) is None
    assert M.keep(need + 5, 1000, 1000, 0.05, k, False, False) is not None
