"""GPU suite: rtc_rep_match against a brute force over all pairs, and clust-mst --save-rep / --append end to end against the
restatement of the reference's state (tests/refmststate.py)."""
import os
import subprocess

import numpy as np
import pytest

import refmststate as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


def _sets(rng, n_reps, n_q, width, base=600):
    """representatives and queries drawn from a few families (shared hashes), sizes around `base`; some queries sit exactly
    at the KSSD size-ratio limit of one representative"""
    hmax = (1 << 62) if width == 8 else (1 << 31) - 1
    fams = [np.unique(rng.integers(1, hmax, size=3 * base, dtype=np.int64)) for _ in range(4)]
    out = []
    for g in range(n_reps + n_q):
        f = fams[g % 4]
        size = int(base * rng.uniform(0.7, 1.3))
        out.append(np.sort(rng.choice(f, size=min(size, len(f)), replace=False)))
    rad = M.radio(0.05, 22)
    r0 = out[0]
    for q, fac in ((n_reps, rad), (n_reps + 1, 1.0 / rad)):
        size = int(np.floor(len(r0) * fac))  # sizeQry / sizeRef just inside the limit
        pool = np.union1d(r0, fams[0])
        out[q] = np.sort(rng.choice(pool, size=min(size, len(pool)), replace=False))
    dt = np.uint64 if width == 8 else np.uint32
    return [s.astype(dt) for s in out]


def _want(sketches, n_reps, thr, k, kssd, cont):
    return [(q, s, c, d) for q, s, c, d in M.brute_pairs(sketches, n_reps, thr, k, kssd, cont)]


@pytest.mark.gpu
@pytest.mark.parametrize("width,kssd,cont,thr", [(8, False, False, 0.05), (8, False, True, 0.05), (4, True, False, 0.05),
                                                  (8, True, False, 0.08), (4, True, False, 0.3)])
def test_rep_match_equals_brute_force(ctx, width, kssd, cont, thr):
    from rabbittclust_amd import api
    rng = np.random.default_rng(width * 10 + kssd + 2 * cont)
    k = 22 if kssd else 21
    sk = _sets(rng, 40, 60, width)
    s = api.SketchSet.from_host(sk, ctx.device, k=k, kind="kssd" if kssd else "minhash", width=width)
    want = _want(sk, 40, thr, k, kssd, cont)
    assert want, "nothing passes: the test shows nothing"
    for chunk in (0, 7):
        d0 = ctx.diag()["repmatch_chunks"]
        got = ctx.rep_match(s, 40, thr, is_kssd=kssd, is_containment=cont, query_chunk=chunk)
        assert ctx.diag()["repmatch_chunks"] - d0 == (1 if chunk == 0 else 9)
        assert [(int(g["query"]), int(g["slot"]), int(g["common"])) for g in got] == [(q, sl, c) for q, sl, c, _ in want]
        assert [float(g["dist"]) for g in got] == [d for *_, d in want]


def _genomes(oracle, tmp, tag, n_fam, per, L, seed):
    from rabbittclust_amd import api
    desc = api.synth_family_descs(n_fam, per, global_seed=seed, max_rate=0.02)
    paths, seqs = [], []
    for g, d in enumerate(desc):
        s = oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), L - 997 * (g % 3))
        p = os.path.join(tmp, f"{tag}{g:03d}.fna")
        with open(p, "wb") as f:
            f.write(f">{tag}{g} synthetic family {g // per}\n".encode() + s.tobytes() + b"\n")
        paths.append(p)
        seqs.append(s)
    lst = os.path.join(tmp, f"{tag}.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst, paths, seqs


def _run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _folders(tmp):
    return sorted(os.path.join(tmp, d) for d in os.listdir(tmp) if os.path.isdir(os.path.join(tmp, d)) and d[:2] == "20")


def _edges(folder):
    import struct
    raw = open(os.path.join(folder, "edge.mst"), "rb").read()
    (m,) = struct.unpack_from("<Q", raw, 0)
    a = np.frombuffer(raw, dtype=np.dtype([("p", "<i4"), ("s", "<i4"), ("d", "<f8")]), count=m, offset=8)
    return [(int(x["p"]), int(x["s"]), float(x["d"])) for x in a]


def _sketch(oracle, seqs, st):
    """the sketches a run with the state's parameters computes (the command line tunes k to the genomes' sizes)"""
    if st.kssd:
        return [oracle.kssd_sketch(s, st.kmer_size, st.drlevel) for s in seqs]
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return oracle.sketch_minhash_batch(np.concatenate(seqs), off, st.kmer_size, st.sketch_size)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [True, False])
def test_save_rep_then_append_end_to_end(oracle, tmp_path, fast):
    import time
    from refpost import clusters_bfs, forest
    tmp = str(tmp_path)
    mst = os.path.join(BIN, "clust-mst")
    lst_a, paths_a, seqs_a = _genomes(oracle, tmp, "a", 3, 4, 300_000, seed=31)
    lst_b, paths_b, seqs_b = _genomes(oracle, tmp, "b", 4, 3, 300_000, seed=32)  # families of A and new ones
    lst_c, paths_c, seqs_c = _genomes(oracle, tmp, "c", 2, 3, 300_000, seed=31)
    fl = ["--fast"] if fast else []
    par = ["-k", "21", "-d", "0.05", "-t", "4"] + ([] if fast else ["-s", "1000"])
    # -e: no sketch folder, so no state
    _run([mst] + fl + ["-l", "-i", lst_a, "--save-rep", "-e", "-o", os.path.join(tmp, "e.out")] + par, tmp)
    assert _folders(tmp) == []
    _run([mst] + fl + ["-l", "-i", lst_a, "-o", os.path.join(tmp, "plain.out")] + par, tmp)
    time.sleep(1.1)  # the folders are named by the second
    _run([mst] + fl + ["-l", "-i", lst_a, "--save-rep", "-o", os.path.join(tmp, "a.out")] + par, tmp)
    plain_dir, folder = _folders(tmp)
    assert open(os.path.join(tmp, "a.out"), "rb").read() == open(os.path.join(tmp, "plain.out"), "rb").read()
    assert not os.path.exists(os.path.join(plain_dir, "mst_cluster_state.bin"))
    state_path = os.path.join(folder, "mst_cluster_state.bin")
    initial = open(state_path, "rb").read()
    st, _ = M.parse(initial)
    # the representatives: the restatement's tree medoids on the run's own forest
    n = len(paths_a)
    fo = forest(_edges(folder), 0.05)
    cl = clusters_bfs(fo, n)
    sk_a = _sketch(oracle, seqs_a, st)
    want = M.State(fast)
    for a in ("threshold", "kmer_size", "sketch_size", "contain_compress", "is_containment", "half_k", "half_subk", "drlevel", "use64"):
        setattr(want, a, getattr(st, a))
    M.initial_state(want, paths_a, st.member_lens, cl, fo, sk_a)
    assert st.fields() == want.fields()
    assert len(st.rep_ids) < n, "every cluster is a singleton: the test shows nothing"
    # the state path of --append, against the restatement; --save-rep writes the state back
    out_b = os.path.join(tmp, "b.out")
    err = _run([mst] + fl + ["--append", lst_b, "--presketched", folder, "--save-rep", "-l", "-o", out_b, "-t", "4"], tmp)
    assert "inverted-index state" in err
    live = M.append(want, paths_b, [len(s) for s in seqs_b], _sketch(oracle, seqs_b, st))
    assert open(out_b).read() == M.cluster_text(live, want.member_names, want.member_lens, True, want.threshold)
    assert open(state_path, "rb").read() == M.save(want)
    # a second append on top of the first; -e: the state stays as it is
    before = open(state_path, "rb").read()
    out_c = os.path.join(tmp, "c.out")
    _run([mst] + fl + ["--append", lst_c, "--presketched", folder, "--save-rep", "-e", "-l", "-o", out_c, "-t", "4"], tmp)
    live = M.append(want, paths_c, [len(s) for s in seqs_c], _sketch(oracle, seqs_c, st))
    assert open(out_c).read() == M.cluster_text(live, want.member_names, want.member_lens, True, want.threshold)
    assert open(state_path, "rb").read() == before
    # --presketched with --save-rep writes the state even with -e (clust_from_sketch[es], src/sub_command.cpp:2577, :2814)
    os.remove(state_path)
    _run([mst] + fl + ["--presketched", folder, "--save-rep", "-e", "-o", os.path.join(tmp, "p.out"), "-d", "0.05", "-t", "4"], tmp)
    assert open(state_path, "rb").read() == initial
    # without the state: the classic append, byte for byte what a folder that never had one gives
    os.remove(state_path)
    out1, out2 = os.path.join(tmp, "cl1.out"), os.path.join(tmp, "cl2.out")
    err = _run([mst] + fl + ["--append", lst_b, "--presketched", folder, "-e", "-l", "-o", out1] + par, tmp)
    assert "inverted-index state" not in err
    _run([mst] + fl + ["--append", lst_b, "--presketched", plain_dir, "-e", "-l", "-o", out2] + par, tmp)
    assert open(out1, "rb").read() == open(out2, "rb").read()
