"""ctypes loader for librtclust_host.so: the C++ host side of the drop-in (FASTA reading, parameter
tuning, on-disk formats, KSSD shuffle table) as a small C ABI (rabbittclust_amd/host/host_capi.cpp).
No GPU code; used by bench.py (--mode kssd needs generate_shuffle_dim) and the tests."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librtclust_host.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = C.CDLL(LIB_PATH)
        _lib.rtch_shuffle_dim.restype = C.c_int
        _lib.rtch_shuffle_dim.argtypes = [C.c_int, C.c_void_p]
    return _lib


_shuffle_cache = {}


def generate_shuffle_dim(half_subk):
    """generate_shuffle_dim (src/SketchInfo.cpp:60-102): the glibc srand/rand shuffle table, int32[2^(4*half_subk)]."""
    if half_subk not in _shuffle_cache:
        sd = np.zeros(1 << (4 * half_subk), dtype=np.int32)
        n = load().rtch_shuffle_dim(int(half_subk), sd.ctypes.data_as(C.c_void_p))
        assert n == len(sd)
        _shuffle_cache[half_subk] = sd
    return _shuffle_cache[half_subk]


def leiden_quantise(u, v, weight, objective):
    """leiden_quantise (rtc_host.cpp): the q of clust-leiden --leiden's records from double weights; objective 0 CPM (the
    reference's normalisation, records with q == 0 dropped), 1 modularity.  Returns ((u, v, q) records, narrow range?)."""
    u = np.ascontiguousarray(u, dtype=np.uint32)
    v = np.ascontiguousarray(v, dtype=np.uint32)
    w = np.ascontiguousarray(weight, dtype=np.float64)
    out = np.zeros(max(len(w), 1), dtype=[("u", "<u4"), ("v", "<u4"), ("q", "<u4")])
    n_out = C.c_uint64(0)
    fn = load().rtch_leiden_quantise
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    narrow = fn(u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(w), int(objective),
                out.ctypes.data_as(C.c_void_p), C.byref(n_out))
    return out[:n_out.value].copy(), bool(narrow)
