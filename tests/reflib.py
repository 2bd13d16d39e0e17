"""ctypes loaders of the reference libraries oracle/Makefile builds where the reference tree is present:
oracle/_ref/libref_dbscan.so (KssdDBSCAN + printKssdDBSCANResult behind oracle/ref_dbscan_shims.cpp) and
oracle/_ref/libref_post.so (build_dedup_candidates_per_cluster + select_k_reps_per_cluster_tree behind
oracle/ref_post_shims.cpp).  ref_dbscan() / ref_post() return None where the file is not there; the tests then fall back to
the fixtures tests/golden/ref_dbscan.npz / ref_postprocess.npz.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REF_DBSCAN = os.path.join(REF_DIR, "libref_dbscan.so")
REF_POST = os.path.join(REF_DIR, "libref_post.so")
EDGE_DT = np.dtype([("preNode", "<i4"), ("sufNode", "<i4"), ("dist", "<f8")])  # the reference's EdgeInfo
MAX_THREADS = 16  # the reference's OpenMP teams are sized by the argument

_libs = {}


def _load(path):
    if path not in _libs:
        _libs[path] = C.CDLL(path) if os.path.exists(path) else None
    return _libs[path]


def ref_dbscan():
    L = _load(REF_DBSCAN)
    if L is not None:
        L.ref_kssd_dbscan.restype = L.ref_kssd_dbscan_print.restype = C.c_int
    return L


def ref_post():
    L = _load(REF_POST)
    if L is not None:
        L.ref_dedup_candidates.restype = L.ref_select_k_reps.restype = C.c_int64
    return L


@contextlib.contextmanager
def quiet_stderr():
    """the reference's progress lines (file descriptor 2) into a temporary file; yields a function that reads them"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)

        def text():
            tmp.seek(0)
            return tmp.read().decode(errors="replace")
        try:
            yield text
        finally:
            os.dup2(saved, 2)
            os.close(saved)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def csr(sketches, use64):
    dt = np.uint64 if use64 else np.uint32
    lens = np.array([len(s) for s in sketches], dtype=np.uint64)
    start = np.zeros(len(sketches) + 1, dtype=np.uint64)
    np.cumsum(lens, out=start[1:])
    flat = np.concatenate([np.asarray(s, dtype=dt) for s in sketches]) if len(sketches) and lens.sum() else np.zeros(1, dtype=dt)
    return np.ascontiguousarray(flat, dtype=dt), start


def kssd_dbscan(L, sketches, use64, eps, min_pts, kmer_size, threads=1, max_posting=0):
    """the reference's KssdDBSCAN: (int32 labels with noise as -1, clusters, noise points)"""
    assert 1 <= threads <= MAX_THREADS
    n = len(sketches)
    flat, start = csr(sketches, use64)
    labels = np.full(max(n, 1), -7, dtype=np.int32)
    ncl, nnoise = C.c_int(-1), C.c_int(-1)
    with quiet_stderr():
        rc = L.ref_kssd_dbscan(C.c_int(n), _p(start), _p(flat), C.c_int(int(use64)), C.c_double(eps), C.c_int(min_pts),
                               C.c_int(kmer_size), C.c_int(threads), C.c_int(max_posting), _p(labels), C.byref(ncl), C.byref(nnoise))
    assert rc == 0, "the reference's result does not list every point exactly once"
    return labels[:n].copy(), ncl.value, nnoise.value


def _strings(xs):
    return (C.c_char_p * max(len(xs), 1))(*[x.encode() for x in xs])


def kssd_dbscan_print(L, sketches, use64, eps, min_pts, kmer_size, genomes, by_file, threads=1, max_posting=0):
    """KssdDBSCAN, then printKssdDBSCANResult: (labels, the file's bytes, the reference's stderr).  genomes as
    refdbscan.print_result takes them: (fileName, totalSeqLength, name, comment) with by_file, else (name, length, comment)."""
    assert 1 <= threads <= MAX_THREADS
    n = len(sketches)
    flat, start = csr(sketches, use64)
    labels = np.full(max(n, 1), -7, dtype=np.int32)
    ncl, nnoise = C.c_int(-1), C.c_int(-1)
    if by_file:
        files, lens, names, comments = ([g[i] for g in genomes] for i in range(4))
    else:
        names, lens, comments = ([g[i] for g in genomes] for i in range(3))
        files = [""] * n
    lens = np.ascontiguousarray(np.array(list(lens) + [0], dtype=np.uint64))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ref.out")
        with quiet_stderr() as err:
            rc = L.ref_kssd_dbscan_print(C.c_int(n), _p(start), _p(flat), C.c_int(int(use64)), C.c_double(eps), C.c_int(min_pts),
                                         C.c_int(kmer_size), C.c_int(threads), C.c_int(max_posting), C.c_int(int(by_file)),
                                         _strings(files), _strings(names), _strings(comments), _p(lens), out.encode(), _p(labels),
                                         C.byref(ncl), C.byref(nnoise))
            log = err()
        assert rc == 0, "the reference's result does not list every point exactly once"
        return labels[:n].copy(), open(out, "rb").read(), log


def _lists(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.array([v for x in lists for v in x] + [0], dtype=np.int32)
    return off, flat


def _unlists(off, flat):
    return [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def _edges(edges):
    e = np.zeros(max(len(edges), 1), dtype=EDGE_DT)
    for i, (a, b, w) in enumerate(edges):
        e[i] = (a, b, w)
    return e


def dedup_candidates(L, n, clusters, edges, seq_len, dedup, by_file=True):
    """build_dedup_candidates_per_cluster (KSSD overload): (node_to_rep list, candidate lists)"""
    cl_off, cl_flat = _lists(clusters)
    e = _edges(edges)
    lens = np.ascontiguousarray(np.array(list(seq_len) + [0], dtype=np.uint64))
    rep = np.full(max(n, 1), -7, dtype=np.int32)
    cap = max(n, 1) + sum(len(c) for c in clusters)
    c_off, c_flat = np.zeros(len(clusters) + 1, dtype=np.int64), np.zeros(cap, dtype=np.int32)
    tot = L.ref_dedup_candidates(C.c_int(n), C.c_int(len(clusters)), _p(cl_off), _p(cl_flat), _p(e), C.c_int64(len(edges)), _p(lens),
                                 C.c_int(int(by_file)), C.c_double(dedup), _p(rep), _p(c_off), _p(c_flat), C.c_int64(cap))
    assert tot >= 0
    return rep[:n].tolist(), _unlists(c_off, c_flat)


def select_k_reps(L, n, clusters, cands, edges, rep, k):
    """select_k_reps_per_cluster_tree: the representative lists"""
    cl_off, cl_flat = _lists(clusters)
    cd_off, cd_flat = _lists(cands)
    e = _edges(edges)
    r = np.array(list(rep) + [0], dtype=np.int32)
    cap = max(n, 1) + sum(len(c) for c in cands)
    o_off, o_flat = np.zeros(len(clusters) + 1, dtype=np.int64), np.zeros(cap, dtype=np.int32)
    tot = L.ref_select_k_reps(C.c_int(n), C.c_int(len(clusters)), _p(cl_off), _p(cl_flat), _p(cd_off), _p(cd_flat), _p(e),
                              C.c_int64(len(edges)), _p(r), C.c_int(k), _p(o_off), _p(o_flat), C.c_int64(cap))
    assert tot >= 0
    return _unlists(o_off, o_flat)
