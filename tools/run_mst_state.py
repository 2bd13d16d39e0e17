"""clust-mst --append against a --save-rep state: the GPU match (rtc_rep_match) and the host replay (append_mst_state), timed
apart, for Q in {1e3, 1e4, 1e5} new sketches against R in {1e3, 1e4} representatives, on KSSD u32 and MinHash u64 sketches.

    python tools/run_mst_state.py [--reps 1000,10000] [--queries 1000,10000,100000] [--repeat 3]

The sets are families of near-identical sketches (a quarter of the queries new families): a representative has a few dozen
partners, as after a real clustering.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _sets(rng, n_reps, n_q, width, size):
    hmax = (1 << 62) if width == 8 else (1 << 31) - 1
    n_fam = n_reps + n_q // 4
    dt = np.uint64 if width == 8 else np.uint32
    bases = rng.integers(1, hmax, size=(n_fam, size), dtype=np.int64)
    out = []
    for g in range(n_reps + n_q):
        f = g if g < n_reps else int(rng.integers(0, n_fam))
        s = bases[f].copy()
        flip = rng.random(size) < 0.02  # ~2 % of the hashes differ from the family's
        s[flip] = rng.integers(1, hmax, size=int(flip.sum()), dtype=np.int64)
        out.append(np.unique(s).astype(dt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", default="1000,10000")
    ap.add_argument("--queries", default="1000,10000,100000")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401
    import refmststate as M
    from rabbittclust_amd import api
    host = C.CDLL(os.path.join(ROOT, "rabbittclust_amd", "librtclust_host.so"))
    host.rtch_mst_state_append.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_long, C.c_char_p, C.c_char_p]
    ctx = api.Context(0)
    tmp = tempfile.mkdtemp()
    for kind, width, size in (("kssd", 4, 600), ("minhash", 8, 1000)):
        kssd = kind == "kssd"
        k = 22 if kssd else 21
        for R in map(int, a.reps.split(",")):
            for Q in map(int, a.queries.split(",")):
                rng = np.random.default_rng(R + Q)
                sk = _sets(rng, R, Q, width, size)
                s = api.SketchSet.from_host(sk, ctx.device, k=k, kind=kind, width=width)
                ctx.rep_match(s, R, 0.05, is_kssd=kssd)  # warm-up
                t_gpu = []
                for _ in range(a.repeat):
                    t0 = time.perf_counter()
                    pairs = ctx.rep_match(s, R, 0.05, is_kssd=kssd)
                    t_gpu.append(time.perf_counter() - t0)
                st = M.State(kssd)
                st.use64, st.kmer_size, st.threshold = width == 8, k, 0.05
                st.N = R
                st.rep_ids, st.rep_lens = list(range(R)), [1_000_000] * R
                st.rep_names = ["r%d" % r for r in range(R)]
                st.rep_hashes = [x.tolist() for x in sk[:R]]
                st.clusters = [[r] for r in range(R)]
                st.member_names, st.member_lens = list(st.rep_names), [1_000_000] * R
                src = os.path.join(tmp, "st.bin")
                open(src, "wb").write(M.save(st))
                flat = np.concatenate(sk[R:])
                off = np.cumsum([0] + [len(x) for x in sk[R:]]).astype(np.uint64)
                names = (C.c_char_p * Q)(*[b"q%d" % q for q in range(Q)])
                lens = np.full(Q, 1_000_000, dtype=np.uint64)
                t0 = time.perf_counter()
                nlive = host.rtch_mst_state_append(src.encode(), int(kssd), Q, names, lens.ctypes.data, flat.ctypes.data, off.ctypes.data,
                                                   pairs.ctypes.data, len(pairs), os.path.join(tmp, "out.cluster").encode(), None)
                t_host = time.perf_counter() - t0  # includes loading the state file and writing the cluster text
                print(json.dumps({"sketch": kind, "width": width, "reps": R, "queries": Q, "pairs": int(len(pairs)),
                                  "gpu_match_ms": round(1e3 * min(t_gpu), 3), "host_replay_ms": round(1e3 * t_host, 3),
                                  "live_clusters": int(nlive)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
