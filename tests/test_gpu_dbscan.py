"""clust-dbscan --fast on the GPU (rtc_dbscan): labels identical to the restated KssdDBSCAN (tests/refdbscan.py) on synthetic
KSSD families, hand-built sets, the eps boundary, u64 sketches, --max-posting, u16 saturation and row chunks, plus the
command line end to end."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import refdbscan as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
SOAK_SEEDS = int(os.environ.get("RTC_SOAK_SEEDS", "3"))  # RTC_SOAK_SEEDS=20: more family layouts


def _family_sketches(ctx, oracle, seed, n_fam=6, per=5, L=400_000, k=21, drlevel=3):
    from rabbittclust_amd import api
    desc = api.synth_family_descs(n_fam, per, global_seed=seed)
    off = np.arange(len(desc) + 1, dtype=np.uint64) * L
    seq = ctx.synth_genomes(desc, off)
    p = oracle.kssd_params(k, drlevel)
    sk = ctx.sketch_kssd(seq, off, oracle.kssd_shuffle_dim(p.half_subk), kmer_size=k, drlevel=drlevel)
    ctx.sync()
    return sk, sk.to_host()


def _check(ctx, sk, host, eps, min_pts, kmer, max_posting=0):
    got = ctx.dbscan(sk, eps, min_pts, kmer, max_posting=max_posting)
    want = R.labels_of(host, eps, min_pts, kmer, sk.width == 8, max_posting)
    assert np.array_equal(got, want), (eps, min_pts, got.tolist(), want.tolist())
    c = ctx.dbscan_counters()
    assert c["asymmetric_pairs"] == 0
    return got, c


@pytest.mark.parametrize("seed", range(1, SOAK_SEEDS + 1))
def test_families_match_the_walk(ctx, oracle, seed):
    sk, host = _family_sketches(ctx, oracle, seed)
    assert sk.width == 4
    # eps values around the within-family distances: some families join, some split, some points become noise
    seen = set()
    for eps in (0.01, 0.02, 0.03, 0.05, 0.1):
        for min_pts in (1, 2, 5, 50):
            got, c = _check(ctx, sk, host, eps, min_pts, 22)
            seen.add(int(got.max()) + 1)
            if min_pts == 1:
                assert (got >= 0).all() and c["core_points"] == sk.n
            if min_pts == 50:
                assert (got == -1).all()
    assert len(seen) > 2  # the eps values cut the families in different ways


def _set(ctx, sketches, width=4):
    from rabbittclust_amd import api
    return api.SketchSet.from_host([np.asarray(s, dtype=np.uint32 if width == 4 else np.uint64) for s in sketches], ctx.device,
                                   k=22, kind="kssd", width=width)


def _block(base, m):
    return np.arange(base, base + m, dtype=np.uint64)


def test_hand_built_border_noise_and_empty(ctx):
    # two chains of sliding windows (100 hashes, step 25: neighbours within two steps at eps 0.04, J >= 0.33), points 0-5 and
    # 7-12; 6 holds half of 5's window and half of 7's: a border point of both clusters (two neighbours, no core at minPts 4)
    # that goes to the first; 0, an end of its chain, is labelled noise when the walk starts and absorbed by cluster 0 later;
    # 13 and 15 are empty, 14 is alone
    def win(i, base):
        return _block(base + 25 * i, 100)
    chain1 = [win(i, 0) for i in range(6)]
    chain2 = [win(i, 100_000) for i in range(6)]
    x = np.concatenate([_block(175, 50), _block(100_000, 50)])
    sk = chain1 + [x] + chain2 + [[], _block(50_000, 80), []]
    host = [np.asarray(v, dtype=np.uint32) for v in sk]
    got, _ = _check(ctx, _set(ctx, sk), host, 0.04, 4, 22)
    assert got.tolist() == [0] * 7 + [1] * 6 + [-1, -1, -1]
    nb = R.neighbour_lists(host, 0.04, 22, False)
    assert sorted(nb[6]) == [5, 7] and sorted(nb[0]) == [1, 2]
    for width in (4, 8):
        s = _set(ctx, sk, width)
        h = [v.astype(np.uint64) for v in host] if width == 8 else host
        for eps in (0.01, 0.04, 0.2):
            for min_pts in (1, 2, 3, 4, 5):
                _check(ctx, s, h, eps, min_pts, 22)


def test_eps_boundary_tolerance(ctx):
    # pairs of equal size a with common c placed just on both sides of the accept boundary c (1 + t) + 1e-12 >= 2 t a
    a = 1000
    sets, base = [], 0
    eps = 0.0731
    t = R.jaccard_min(eps, 22)
    c0 = next(c for c in range(a + 1) if not (c * (1.0 + t) + 1e-12 < t * a + t * a))
    for c in (c0 - 1, c0, c0 + 1):
        x = _block(base, a)
        y = np.concatenate([x[:c], _block(base + 10 * a, a - c)])
        sets += [x, y]
        base += 100 * a
    s = _set(ctx, sets)
    host = [np.asarray(v, dtype=np.uint32) for v in sets]
    got, _ = _check(ctx, s, host, eps, 2, 22)
    assert got[0] == -1 and got[1] == -1 and got[2] >= 0 and got[2] == got[3] and got[4] == got[5] >= 0


def _near_tie(a, b, c, k):
    """eps values on both sides of the 1e-12 tolerance for a pair of sizes a, b sharing c: eps_in makes
    c (1 + t) < t a + t b but not by more than 1e-12 (the tolerance alone accepts it), eps_out makes the gap exceed 1e-12.
    Built from t* = c / (a + b - c), where c (1 + t*) = t* (a + b): x = 2 t* / (1 + t*), eps = -ln(x) / k, then walked ulp by ulp."""
    ts = c / (a + b - c)
    eps0 = -math.log(2.0 * ts / (1.0 + ts)) / k
    e_in = e_out = None
    e = eps0
    for _ in range(4000):  # up: t falls, the right side falls -> towards acceptance; down: towards rejection
        e = math.nextafter(e, -1.0)
        t = R.jaccard_min(e, k)
        lhs, rhs = c * (1.0 + t), t * a + t * b
        if lhs < rhs and not (lhs + 1e-12 < rhs) and e_in is None:
            e_in = e
        if lhs + 1e-12 < rhs:
            e_out = e
            break
    e = eps0
    for _ in range(4000):
        if e_in is not None:
            break
        e = math.nextafter(e, 1.0)
        t = R.jaccard_min(e, k)
        lhs, rhs = c * (1.0 + t), t * a + t * b
        if lhs < rhs and not (lhs + 1e-12 < rhs):
            e_in = e
    return e_in, e_out


@pytest.mark.parametrize("a,b,c", [(1000, 1000, 700), (1000, 900, 612), (333, 517, 250)])
def test_eps_on_both_sides_of_the_1e12_tolerance(ctx, a, b, c):
    k = 22
    e_in, e_out = _near_tie(a, b, c, k)
    assert e_in is not None and e_out is not None, "no eps found within 1e-12 of the boundary"
    for e, accepted in ((e_in, True), (e_out, False)):
        t = R.jaccard_min(e, k)
        lhs, rhs = c * (1.0 + t), t * a + t * b
        assert (lhs < rhs) and ((lhs + 1e-12 < rhs) != accepted)
    x = _block(0, a)
    y = np.concatenate([x[:c], _block(10 * (a + b), b - c)])
    for width in (4, 8):
        dt = np.uint32 if width == 4 else np.uint64
        host = [x.astype(dt), y.astype(dt)]
        s = _set(ctx, [x, y], width)
        assert R.neighbour_lists(host, e_in, k, width == 8) == [[1], [0]]
        assert R.neighbour_lists(host, e_out, k, width == 8) == [[], []]
        got_in, _ = _check(ctx, s, host, e_in, 2, k)
        got_out, _ = _check(ctx, s, host, e_out, 2, k)
        assert got_in.tolist() == [0, 0] and got_out.tolist() == [-1, -1]


def test_u64_sketches(ctx, oracle):
    sk, host = _family_sketches(ctx, oracle, 11, n_fam=4, per=4, L=300_000, k=25, drlevel=3)
    assert sk.width == 8
    for eps in (0.01, 0.03, 0.08):
        for min_pts in (1, 2, 5):
            _check(ctx, sk, host, eps, min_pts, 26)
    # empty u64 sketches are neighbours of each other in the brute force (one cluster at minPts <= their number)
    sets = [_block(0, 200), [], _block(0, 200), [], []]
    h = [np.asarray(x, dtype=np.uint64) for x in sets]
    for min_pts in (1, 3, 4):
        _check(ctx, _set(ctx, sets, 8), h, 0.05, min_pts, 22)


def test_max_posting(ctx, oracle):
    sk, host = _family_sketches(ctx, oracle, 5, n_fam=5, per=4, L=300_000)
    for M in (1, 2, 3, 4, 8, 1000):
        _check(ctx, sk, host, 0.05, 2, 22, max_posting=M)
    # a hash every sketch holds: pruned, it no longer links anything
    common = 7
    sets = [np.unique(np.concatenate([[common], _block(100 * g + 1000, 20 if g % 3 else 3)])) for g in range(12)]
    h = [np.asarray(x, dtype=np.uint32) for x in sets]
    s = _set(ctx, sets)
    for M in (0, 11, 12):
        _check(ctx, s, h, 0.5, 2, 22, max_posting=M)


def test_u16_saturation_flips_a_decision(ctx):
    # sizes 70 000 + 70 000 sharing 68 000: the reference counts at most 65 535 in the u32 path, which fails where 68 000 passes
    a, c = 70_000, 68_000
    x = _block(0, a)
    y = np.concatenate([x[:c], _block(10 * a, a - c)])
    host = [x.astype(np.uint32), y.astype(np.uint32)]
    eps = None
    for e in np.linspace(0.0005, 0.05, 400):
        t = R.jaccard_min(float(e), 22)
        ok_full = not (c * (1.0 + t) + 1e-12 < t * a + t * a)
        ok_sat = not (65535 * (1.0 + t) + 1e-12 < t * a + t * a)
        if ok_full and not ok_sat:
            eps = float(e)
            break
    assert eps is not None
    got, _ = _check(ctx, _set(ctx, [x, y]), host, eps, 2, 22)
    assert (got == -1).all()
    got64, _ = _check(ctx, _set(ctx, [x, y], 8), [v.astype(np.uint64) for v in host], eps, 2, 22)
    assert (got64 == 0).all()


def test_row_chunks_keep_the_labels(ctx, oracle):
    # every sketch shares one hash with every other: the candidate list is the whole triangle and a small edge budget cuts it
    n = 600
    rng = np.random.default_rng(3)
    sets = []
    for g in range(n):
        fam = g % 7
        body = _block(100_000 * fam, 60)[rng.random(60) < 0.9]
        sets.append(np.unique(np.concatenate([[1], body, _block(10_000_000 + 1000 * g, 5)])))
    h = [np.asarray(x, dtype=np.uint32) for x in sets]
    s = _set(ctx, sets)
    want, c1 = _check(ctx, s, h, 0.1, 4, 22)
    assert c1["chunks"] == 1 and c1["candidate_edges"] == n * (n - 1) // 2
    with ctx.env(RTC_EDGE_BUDGET=str(64 * n + 1024)):
        got, c2 = _check(ctx, s, h, 0.1, 4, 22)
    assert np.array_equal(got, want) and c2["chunks"] > 2 and c2["candidate_edges"] == c1["candidate_edges"]
    assert c2["eps_edges"] == c1["eps_edges"]


def _write_fastas(oracle, tmp, n_fam, per, L, seed):
    from rabbittclust_amd import api
    desc = api.synth_family_descs(n_fam, per, global_seed=seed)
    paths, seqs, meta = [], [], []
    for g, d in enumerate(desc):
        s = oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), L)
        p = os.path.join(tmp, f"g{g:03d}.fna")
        with open(p, "wb") as f:
            f.write(f">g{g} synthetic family {g // per}\n".encode())
            raw = s.tobytes()
            for i in range(0, len(raw), 80):
                f.write(raw[i:i + 80] + b"\n")
        paths.append(p)
        seqs.append(s)
        meta.append((p, L, f"g{g}", f"synthetic family {g // per}"))
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst, seqs, meta


def _run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _folders(d):
    return [os.path.join(d, x) for x in os.listdir(d) if os.path.isdir(os.path.join(d, x)) and x[:2] == "20"]


def test_cli_end_to_end(oracle, tmp_path):
    tmp = str(tmp_path)
    L = 1_000_000
    lst, seqs, meta = _write_fastas(oracle, tmp, 4, 4, L, seed=9)
    D = os.path.join(BIN, "clust-dbscan")
    # -k 17: what the KSSD tuner keeps for genomes of 1 Mbp (a larger -k is replaced by it); odd, so half_k * 2 = 18
    ks = [oracle.kssd_sketch(s, 17, 3) for s in seqs]
    d1 = os.path.join(tmp, "l"); os.makedirs(d1)
    out = os.path.join(tmp, "l.out")
    err = _run([D, "--fast", "-l", "-i", lst, "-k", "17", "--eps", "0.03", "--minpts", "2", "-t", "4", "-o", out], d1)
    assert "-----the kmerSize is: 17" in err
    want = R.labels_of(ks, 0.03, 2, 17, False)
    assert open(out).read() == R.print_result(want, meta, True, 0.03, 2)
    ncl = int(want.max()) + 1
    assert f"-----Found {ncl} clusters\n" in err and f"-----Found {int((want < 0).sum())} noise points (outliers)\n" in err
    assert "-----Core points: " in err
    folder = _folders(d1)
    assert len(folder) == 1 and os.path.exists(os.path.join(folder[0], "kssd.hash.sketch"))
    assert not os.path.exists(os.path.join(folder[0], "kssd.sketch.index"))
    raw = open(os.path.join(folder[0], "kssd.hash.sketch"), "rb").read()
    pos = 20
    for w in ks:
        (m,) = struct.unpack_from("<Q", raw, pos); pos += 8
        assert np.array_equal(np.frombuffer(raw, dtype="<u4", count=m, offset=pos), w); pos += 4 * m
    # --presketched with the odd -k: the folder's half_k * 2 = 18 decides, printed with -l from the command line
    want18 = R.labels_of(ks, 0.03, 2, 18, False)
    out2 = os.path.join(tmp, "p.out")
    err2 = _run([D, "--fast", "--presketched", folder[0], "-l", "-k", "17", "--eps", "0.03", "--minpts", "2", "-o", out2], tmp)
    assert open(out2).read() == R.print_result(want18, meta, True, 0.03, 2)
    assert "sketch format mismatch" not in err2
    out3 = os.path.join(tmp, "p3.out")
    err3 = _run([D, "--fast", "--presketched", folder[0], "--eps", "0.03", "--minpts", "2", "-o", out3], tmp)
    assert "Warning: sketch format mismatch" in err3
    # printed in the sequence layout the command line asks for, from fields the -l folder never stored: empty names, length 0
    assert open(out3).read() == R.print_result(want18, [("", 0, "")] * len(seqs), False, 0.03, 2)
    # -e: no folder; one multi-record FASTA without -l: sequence mode
    d2 = os.path.join(tmp, "s"); os.makedirs(d2)
    fa = os.path.join(tmp, "all.fna")
    with open(fa, "wb") as f:
        for g, s in enumerate(seqs):
            f.write(f">r{g} member {g}\n".encode() + s.tobytes() + b"\n")
    out4 = os.path.join(tmp, "s.out")
    _run([D, "--fast", "-i", fa, "-k", "17", "--eps", "0.05", "--minpts", "3", "-e", "-t", "4", "-o", out4], d2)
    assert _folders(d2) == []
    want4 = R.labels_of(ks, 0.05, 3, 17, False)
    seq_meta = [(f"r{g}", L, f"member {g}") for g in range(len(seqs))]
    assert open(out4).read() == R.print_result(want4, seq_meta, False, 0.05, 3)
