"""CPU suite: the oracle against public known answers, committed golden fixtures and independent
brute-force restatements.  No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_murmur3_smhasher_known_answer(oracle):
    # published SMHasher verification value of MurmurHash3_x64_128
    assert oracle.lib().orc_murmur3_smhasher_verification() == 0x6384BA69


def test_murmur3_golden_vectors(oracle):
    g = json.load(open(os.path.join(GOLD, "murmur3_vectors.json")))
    assert g["smhasher_verification"] == "0x6384ba69"
    for v in g["vectors"]:
        assert oracle.murmur3_x64_128(bytes.fromhex(v["key_hex"]), v["seed"]) == (v["h1"], v["h2"])


def test_kmer_hash_is_canonical_and_case_insensitive(oracle):
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rng = np.random.default_rng(1)
    for k in (5, 16, 17, 21, 32):
        kmer = bytes(rng.choice(list(b"ACGT"), size=k).tolist())
        rc = kmer.translate(comp)[::-1]
        h = oracle.kmer_hash(kmer)
        assert h == oracle.kmer_hash(rc) == oracle.kmer_hash(kmer.lower())
        canon = min(kmer, rc)
        h1, _ = oracle.murmur3_x64_128(canon, 42)
        assert h == (h1 if k > 16 else h1 & 0xFFFFFFFF)


def test_minhash_sketch_is_bottom_s_of_all_kmer_hashes(oracle):
    rng = np.random.default_rng(2)
    g = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=4000, p=[.245, .245, .245, .245, .02])
    off = np.array([0, len(g)], dtype=np.uint64)
    k, s = 11, 64
    got = oracle.sketch_minhash_batch(g, off, k, s)[0]
    raw = g.tobytes()
    hs = {oracle.kmer_hash(raw[i:i + k]) for i in range(len(raw) - k + 1) if b"N" not in raw[i:i + k]}
    assert got.tolist() == sorted(hs)[:s]


def test_sketch_fixture_frozen(oracle):
    fx = np.load(os.path.join(GOLD, "sketch_fixture.npz"), allow_pickle=True)
    L = int(fx["L"])
    genomes = [oracle.synth_genome(int(f), int(m), int(t), L, int(ne)) for f, m, t, ne in fx["descs"]]
    seq = np.concatenate(genomes)
    off = np.arange(len(genomes) + 1, dtype=np.uint64) * L
    mh = oracle.sketch_minhash_batch(seq, off, 21, 400, threads=1)
    for a, b in zip(mh, fx["minhash"]):
        assert np.array_equal(a, b)
    for g, b in zip(genomes, fx["kssd"]):
        assert np.array_equal(oracle.kssd_sketch(g, 21, 3), b)
    flat, start, lens = oracle.to_csr(mh)
    mst = oracle.mst(flat, start, lens, 21, 0, 0.05, threads=1)
    assert np.array_equal(mst["dist"].view(np.uint64), fx["mst"]["dist"].view(np.uint64))
    assert np.array_equal(mst["pre"], fx["mst"]["pre"]) and np.array_equal(mst["suf"], fx["mst"]["suf"])


def test_kssd_shuffle_table_matches_fixture(oracle):
    fx = np.load(os.path.join(GOLD, "kssd_shuffle_hs6.npz"))
    sd = oracle.kssd_shuffle_dim(6)
    assert np.array_equal(sd[:64], fx["head"])
    kept = np.nonzero(sd < 4096)[0]
    assert np.array_equal(kept.astype(np.uint32), fx["dim_id"])
    assert np.array_equal(sd[kept].astype(np.uint16), fx["rank"])
    assert len(np.unique(sd)) == 1 << 24


def test_kssd_sketch_matches_bruteforce_restatement(oracle):
    """Independent pure-Python restatement of src/SketchInfo.cpp:1126-1165 on a short genome."""
    rng = np.random.default_rng(3)
    g = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=30000)
    k, dr = 21, 3
    p = oracle.kssd_params(k, dr)
    sd = oracle.kssd_shuffle_dim(p.half_subk)
    half_k, hs = p.half_k, p.half_subk
    K = 2 * half_k
    tupmask = (1 << (4 * half_k)) - 1
    hoc = half_k - hs
    domask = (tupmask >> (4 * hoc)) << (2 * hoc)
    undomask = (tupmask ^ domask) & tupmask
    und1 = undomask & (tupmask >> ((half_k + hs) * 2))
    und0 = undomask ^ und1
    code = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
    tup = rvs = 0
    base = 1
    out = set()
    for ch in g.tolist():
        b = code.get(ch, -1)
        if b < 0:
            base, tup, rvs = 1, 0, 0
            continue
        tup = ((tup << 2) | b) & tupmask
        rvs = (rvs >> 2) + ((b ^ 3) << (4 * half_k - 2))
        base += 1
        if base > K:
            uni = min(tup, rvs)
            dim = (uni & domask) >> (2 * hoc)
            r = int(sd[dim])
            if r >= p.dim_end:
                continue
            out.add(((((uni & und0) | ((uni & und1) << (2 * K - 4 * hoc))) >> (4 * dr)) | r) & 0xFFFFFFFF)
    assert oracle.kssd_sketch(g, k, dr).tolist() == sorted(out)


def test_distances_and_radio(oracle):
    L = oracle.lib()
    assert L.orc_mst_radio(0.05, 21) == 4       # (int)(2*exp(0.05*20) - 1) = 4.436 -> 4
    assert L.orc_mst_distance(1000, 1000, 1000, 21, 0) == 0.0
    assert L.orc_mst_distance(0, 1000, 1000, 21, 0) == 1.0
    j = 500 / 1500
    assert L.orc_mst_distance(500, 1000, 1000, 21, 0) == -(1.0 / 21) * math.log((2.0 * j) / (1.0 + j))
    assert L.orc_mst_distance(300, 600, 1000, 21, 1) == -(1.0 / 21) * math.log(300 / 600)
    # greedy clamps at 1, MST does not
    assert L.orc_greedy_distance(1, 100000, 100000, 5, 0) == 1.0
    assert L.orc_mst_distance(1, 100000, 100000, 5, 0) > 1.0
    assert L.orc_kssd_greedy_distance(0, 10, 10, 21) == 1.0


def test_tune_parameters_table(oracle):
    # 1 Mbp FASTA (1,012,520 B): user -k 21 is replaced by 17; 5 Mbp keeps 21
    r = oracle.tune_parameters(0, 1, 0, 1, 21, 0.05, 1000, 1000, 1012520, 1012520, 1012520)
    assert (r.kmer_size, r.ok) == (17, 1)
    r = oracle.tune_parameters(0, 1, 0, 1, 21, 0.05, 1000, 1000, 5062520, 5062520, 5062520)
    assert (r.kmer_size, r.ok) == (21, 1)
    r = oracle.tune_parameters(0, 0, 0, 0, 19, 0.05, 1000, 1000, 5062520, 5062520, 5062520)
    assert r.kmer_size == 18
    # greedy without -s/-c defaults to containment with compress = avg/1000
    r = oracle.tune_parameters(1, 1, 0, 0, 21, 0.05, 1000, 1000, 5062520, 5062520, 5062520)
    assert (r.is_containment, r.contain_compress) == (1, 5062)
    # -s and -c together are rejected; too large a threshold is rejected
    assert oracle.tune_parameters(0, 1, 1, 1, 21, 0.05, 1000, 1000, 5062520, 5062520, 5062520).ok == 0
    assert oracle.tune_parameters(0, 1, 0, 1, 21, 0.9, 1000, 1000, 5062520, 5062520, 5062520).ok == 0


def _brute_edges(sk, k, containment, thr, oracle):
    n = len(sk)
    radio = oracle.lib().orc_mst_radio(thr, k)
    out = []
    for i in range(n):
        for j in range(i):
            c = len(np.intersect1d(sk[i], sk[j]))
            if c == 0 or len(sk[i]) == 0 or len(sk[j]) == 0:
                continue
            if max(len(sk[i]), len(sk[j])) > radio * min(len(sk[i]), len(sk[j])):
                continue
            out.append((oracle.lib().orc_mst_distance(c, len(sk[i]), len(sk[j]), k, int(containment)), i, j))
    return out


@pytest.mark.parametrize("containment", [False, True])
@pytest.mark.parametrize("threads", [1, 3])
def test_oracle_mst_against_bruteforce_kruskal(oracle, containment, threads):
    rng = np.random.default_rng(4)
    pool = np.unique(rng.integers(1, 1 << 60, size=900, dtype=np.uint64))
    sk = [np.sort(rng.choice(pool, size=int(rng.integers(0, 120)), replace=False)) for _ in range(61)]
    flat, start, lens = oracle.to_csr(sk)
    got = oracle.mst(flat, start, lens, 21, containment, 0.05, threads=threads)
    edges = sorted(_brute_edges(sk, 21, containment, 0.05, oracle))
    parent = list(range(len(sk)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    want = []
    for d, i, j in edges:
        a, b = find(i), find(j)
        if a != b:
            parent[a] = b
            want.append(d)
    assert sorted(got["dist"].tolist()) == sorted(want)
    # candidate pairs = every pair with a non-empty intersection
    cand = oracle.candidate_pairs(flat, start, lens)
    assert len(cand) == sum(1 for i in range(len(sk)) for j in range(i) if len(np.intersect1d(sk[i], sk[j])))


def test_unionfind_and_kruskal_against_reference_fixture(oracle):
    fx = np.load(os.path.join(GOLD, "unionfind.npz"))
    edges = np.zeros(len(fx["xs"]), dtype=oracle.EDGE_DT)
    edges["pre"], edges["suf"], edges["dist"] = fx["xs"], fx["ys"], np.arange(len(fx["xs"]))
    keep = edges[edges["pre"] != edges["suf"]]
    out = np.zeros(len(keep) + 1, dtype=oracle.EDGE_DT)
    m = oracle.lib().orc_kruskal(keep.ctypes.data_as(C.c_void_p), C.c_uint64(len(keep)), C.c_int(200),
                                 out.ctypes.data_as(C.c_void_p))
    # the forest connects exactly what the reference UnionFind connected
    parent = list(range(200))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for e in out[:m]:
        parent[find(int(e["pre"]))] = find(int(e["suf"]))
    roots = fx["roots"]
    for a in range(200):
        for b in (0, 57, 199):
            assert (find(a) == find(b)) == (roots[a] == roots[b])
    assert 200 - m == int(fx["size"])


def test_greedy_oracle_basic_invariants(oracle):
    rng = np.random.default_rng(5)
    anc = [np.unique(rng.integers(0, 1 << 50, size=300, dtype=np.uint64)) for _ in range(8)]
    sk = []
    for a in anc:
        for m in range(4):
            v = a.copy()
            idx = rng.choice(len(v), size=10 * m, replace=False)
            v[idx] = rng.integers(0, 1 << 50, size=len(idx), dtype=np.uint64)
            sk.append(np.unique(v))
    flat, start, lens = oracle.to_csr(sk)
    n, rep = oracle.greedy_minhash(flat, start, lens, 300, 21, False, 0.05)
    assert n == 8
    for i, r in enumerate(rep):
        assert rep[r] == r and r <= i and r // 4 == i // 4


# ---- an independent pure-Python twin of the greedy restatement (dict-based inverted index, the
# reference's own loop order) -- every other restated function has one; src/greedy.cpp:986-1399, :566-899
def _py_greedy(sk, size_cfg, k, containment, thr, kssd=False):
    import math
    n = len(sk)
    rep_of = list(range(n))
    index = {}                                    # hash -> [rep ids in insertion order]
    for h in sk[0].tolist():
        index.setdefault(h, []).append(0)
    x = math.exp(-thr * k)
    jmin = x / (2.0 - x)
    fast = False
    fixed_min = 0
    if not kssd:
        fixed = int(size_cfg[0])
        fast = (not containment) and all(int(size_cfg[i]) == fixed for i in range(1, min(100, n)))
        if fast:
            fixed_min = int(math.ceil(jmin * (2 * fixed) / (1.0 + jmin)))
    for j in range(1, n):
        q = sk[j].tolist()
        size_ref = len(q)
        cnt, touched = {}, []
        for h in q:                               # first-touch order = the -t 1 visiting order
            for r in index.get(h, ()):
                if r not in cnt:
                    cnt[r] = 1
                    touched.append(r)
                else:
                    cnt[r] += 1
        best_rep, best_common, best_dist, best_jac = -1, -1, float("inf"), -1.0
        for r in touched:
            common = cnt[r]
            if kssd:
                size_q = len(sk[r])
                if common < int(math.ceil(jmin * (size_ref + size_q) / (1.0 + jmin))):
                    continue
                den = size_ref + size_q - common
                jac = 1.0 if den == 0 else common / den
                if jac > best_jac:
                    best_jac, best_rep = jac, r
                continue
            size_q = int(size_cfg[r])
            if fast:
                cmin = fixed_min
            elif containment:
                cmin = int(math.ceil(jmin * min(size_ref, size_q)))
            else:
                cmin = int(math.ceil(jmin * (size_ref + size_q) / (1.0 + jmin)))
            if common < cmin:
                continue
            if fast:
                if common > best_common:
                    best_common, best_rep = common, r
            else:
                den = min(size_ref, size_q) if containment else size_ref + size_q - common
                if den == 0:
                    dist = 1.0 if containment else 0.0
                else:
                    jac = common / den
                    if jac >= 1.0:
                        dist = 0.0
                    elif jac <= 0.0:
                        dist = 1.0
                    else:
                        dist = min(-math.log(2.0 * jac / (1.0 + jac)) / k, 1.0)
                if dist <= thr and dist < best_dist:
                    best_dist, best_rep = dist, r
        if best_rep >= 0:
            rep_of[j] = best_rep
        else:
            for h in q:
                index.setdefault(h, []).append(j)
    return sum(1 for i in range(n) if rep_of[i] == i), rep_of


def _greedy_families(rng, n_fam, per, size, ragged, dtype=np.uint64, bits=50):
    sk = []
    for _ in range(n_fam):
        anc = np.unique(rng.integers(0, 1 << bits, size=2 * size, dtype=np.uint64))[:size]
        for m in range(per):
            s = size if not ragged else int(size * rng.uniform(0.3, 1.0))
            v = anc[:s].copy()
            if m % 3:
                idx = rng.choice(len(v), size=int(len(v) * 0.5 * rng.uniform(0, 1)), replace=False)
                v[idx] = rng.integers(0, 1 << bits, size=len(idx), dtype=np.uint64)
            sk.append(np.unique(v).astype(dtype))
    order = rng.permutation(len(sk))
    return [sk[i] for i in order]


@pytest.mark.parametrize("mode", ["fixed", "containment", "variable", "kssd"])
def test_greedy_oracle_equals_python_twin(oracle, mode):
    rng = np.random.default_rng({"fixed": 71, "containment": 72, "variable": 73, "kssd": 74}[mode])
    if mode == "fixed":
        sk = _greedy_families(rng, 30, 6, 200, False)
        cfg = np.full(len(sk), 200, dtype=np.uint32)
        flat, start, lens = oracle.to_csr(sk)
        for thr in (0.02, 0.05):
            want_n, want = _py_greedy(sk, cfg, 21, False, thr)
            got_n, got = oracle.greedy_minhash(flat, start, lens, cfg, 21, False, thr)
            assert got_n == want_n and got.tolist() == want
        assert 1 < got_n < len(sk)
    elif mode in ("containment", "variable"):
        sk = _greedy_families(rng, 25, 6, 300, True)
        cfg = np.array([max(len(s), 100) for s in sk], dtype=np.uint32)
        flat, start, lens = oracle.to_csr(sk)
        cont = mode == "containment"
        want_n, want = _py_greedy(sk, cfg, 21, cont, 0.05)
        got_n, got = oracle.greedy_minhash(flat, start, lens, cfg, 21, cont, 0.05)
        assert got_n == want_n and got.tolist() == want and 1 < got_n < len(sk)
    else:
        sk = _greedy_families(rng, 25, 6, 250, True, dtype=np.uint32, bits=30)
        sk.sort(key=lambda a: -len(a))
        flat, start, lens = oracle.to_csr(sk, dtype=np.uint32)
        want_n, want = _py_greedy(sk, None, 22, False, 0.05, kssd=True)
        got_n, got = oracle.greedy_kssd(flat, start, lens, 22, 0.05)
        assert got_n == want_n and got.tolist() == want and 1 < got_n < len(sk)


def test_sketch_threshold_test_word_bounds():
    """The sketch kernel's one-compare threshold test (csrc/rtc_sketch_minhash.hip, hash_test_word): with a, b the two
    fmix64 halves before their last multiply by C, w = hi32((a + b) * C mod 2^64) + 1 must equal hi32(hash) + {0, 1, 2}
    (mod 2^32) for hash = fin(a * C) + fin(b * C), fin(f) = f ^ f >> 33 -- random halves and halves built so that
    hi(f1) + hi(f2) wraps or sits at 2^32 - 1 / 2^32 - 2 (the cases the slack of 2 exists for)."""
    M64, M32 = (1 << 64) - 1, (1 << 32) - 1
    Cm = 0xc4ceb9fe1a85ec53
    Cinv = pow(Cm, -1, 1 << 64)
    rng = np.random.default_rng(7)

    def check(a, b):
        f1, f2 = a * Cm & M64, b * Cm & M64
        h = ((f1 ^ f1 >> 33) + (f2 ^ f2 >> 33)) & M64
        w = ((((a + b) & M64) * Cm & M64) >> 32) + 1 & M32
        d = (w - (h >> 32)) & M32
        assert d in (0, 1, 2), (hex(a), hex(b), d)
        return d

    seen = set()
    for a, b in rng.integers(0, 1 << 64, size=(20000, 2), dtype=np.uint64).tolist():
        seen.add(check(a, b))
    # products with chosen high words: f1 = x, f2 = y  =>  a = x * C^-1, b = y * C^-1
    for hi_sum in (M32, M32 - 1, 0, 1, (1 << 32), (1 << 32) + 1):
        for _ in range(2000):
            h1 = int(rng.integers(0, 1 << 32))
            h2 = (hi_sum - h1) & M32
            for lo1, lo2 in ((int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))), (M32, M32), (0, 0), (M32, 1)):
                seen.add(check((h1 << 32 | lo1) * Cinv & M64, (h2 << 32 | lo2) * Cinv & M64))
    assert seen == {0, 1, 2}


# ---- the distance half against the reference's own functions (tests/golden/ref_distance_half.npz) -----------------------
INT32_MAX = 2 ** 31 - 1


def _ref_fixture():
    return np.load(os.path.join(GOLD, "ref_distance_half.npz"))


def _make_golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def _saturated_radio(calr):
    """the filter's bound: floor of the reference's calr, saturated at INT32_MAX"""
    return int(calr) if calr < INT32_MAX else INT32_MAX


def test_radio_is_the_reference_calr_saturated(oracle):
    from rabbittclust_amd import api
    fx = _ref_fixture()
    L = oracle.lib()
    seen = set()
    for d, k, calr, msr in zip(fx["radio_d"], fx["radio_k"], fx["calr"], fx["max_size_ratio"]):
        d, k = float(d), int(k)
        # calculateMaxSizeRatio(d, k) is calr(d, k) (the KSSD greedy's double bound, host/main.cpp, test_gpu_cli.py)
        assert msr == 2.0 * math.exp(d * k) - 1.0, (d, k)
        if k == 1:
            assert math.isnan(calr)  # calr(d, 0) throws in the reference; the k-mer sizes here are >= 2
            continue
        want = _saturated_radio(float(calr))
        assert L.orc_mst_radio(d, k) == want, (d, k, calr)
        assert api.mst_radio(d, k) == want, (d, k, calr)
        seen.add("saturated" if want == INT32_MAX else "exact")
        if 2 ** 31 <= calr < 2 ** 32:
            seen.add("past 2^31")
        if calr >= 2 ** 32:
            seen.add("past 2^32")  # where a modulo-2^32 conversion (ctypes c_int) would give a small radio
    assert seen == {"saturated", "exact", "past 2^31", "past 2^32"}
    assert api.mst_radio(0.6931471805862327, 32) == INT32_MAX  # calr = 4 294 967 298: c_int would pass 2
    assert api.mst_radio(1e6, 21) == INT32_MAX and L.orc_mst_radio(1e6, 21) == INT32_MAX  # exp overflows to +inf


def test_mash_distance_fast_equals_reference(oracle):
    """orc_kssd_greedy_distance is calculate_mash_distance_fast; the MST distance (api.mst_distance, orc_mst_distance) is the
    same expression without the clamp at 1"""
    from rabbittclust_amd import api
    fx = _ref_fixture()
    L = oracle.lib()
    got = np.array([L.orc_kssd_greedy_distance(*map(int, a)) for a in fx["mash_args"]])
    assert np.array_equal(got.view(np.uint64), fx["mash_dist"].view(np.uint64))
    for (c, s0, s1, k), want in zip(fx["mash_args"].tolist(), fx["mash_dist"]):
        if c > min(s0, s1):  # no intersection is larger than a set (the grid pins the reference there too)
            continue
        for d in (api.mst_distance(c, s0, s1, k, False), L.orc_mst_distance(c, s0, s1, k, 0)):
            assert min(d, 1.0) == want, (c, s0, s1, k)
    assert {0.0, 1.0} <= set(fx["mash_dist"].tolist()) and ((fx["mash_dist"] > 0) & (fx["mash_dist"] < 1)).sum() > 100


def test_tune_max_distance_is_the_reference_expression(oracle):
    """tune_parameters' maxDist at minJaccard = 1/sketchSize is calculate_mash_distance_fast(1, 1, sketchSize, k)"""
    fx = _ref_fixture()
    n = 0
    for (c, s0, s1, k), want in zip(fx["mash_args"].tolist(), fx["mash_dist"]):
        if (c, s0) != (1, 1) or not 15 <= k <= 21 or s1 < 100:
            continue
        r = oracle.tune_parameters(0, 1, 0, 1, k, 0.01, 1000, s1, 5062520, 5062520, 5062520)
        assert r.kmer_size == k and r.max_dist == want, (s1, k)
        n += 1
    assert n >= 6


def _edges_as_oracle(oracle, e):
    out = np.zeros(len(e), dtype=oracle.EDGE_DT)
    out["pre"], out["suf"], out["dist"] = e["preNode"], e["sufNode"], e["dist"]
    return out


def _partition_of(edges, n):
    from oracle.brute import partition
    return partition(zip(edges["dist"], edges["pre"], edges["suf"]), n)


def test_kruskal_and_forest_cut_equal_reference(oracle):
    """orc_kruskal is kruskalAlgorithm (record for record, ties and self-loops included); orc_forest_clusters cuts at
    dist <= threshold like generateForest, with the threshold on an edge's distance and one ulp either side"""
    fx = _ref_fixture()
    cases = 0
    while f"kr{cases}_n" in fx:
        i = cases
        n, e, tree = int(fx[f"kr{i}_n"]), _edges_as_oracle(oracle, fx[f"kr{i}_edges"]), _edges_as_oracle(oracle, fx[f"kr{i}_tree"])
        out = np.zeros(max(len(e), 1), dtype=oracle.EDGE_DT)
        m = oracle.lib().orc_kruskal(e.ctypes.data_as(C.c_void_p), C.c_uint64(len(e)), C.c_int(n), out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out[:m], tree), i
        for t, thr in enumerate(fx[f"kr{i}_thr"]):
            forest = _edges_as_oracle(oracle, fx[f"kr{i}_forest{t}"])
            assert np.array_equal(forest, tree[tree["dist"] <= thr]), (i, thr)
            got = sorted(tuple(sorted(c)) for c in oracle.forest_clusters(tree, float(thr), n))
            assert got == _partition_of(forest, n), (i, thr)
        cases += 1
    assert cases == 7
    # the thresholds on an edge cut differently from one ulp below
    thr = fx["kr2_thr"]
    tree = fx["kr2_tree"]
    assert (tree["dist"] <= thr[4]).sum() > (tree["dist"] <= thr[3]).sum()


def test_shuffle_table_equals_reference(oracle):
    import hashlib
    fx = _ref_fixture()
    sd = oracle.kssd_shuffle_dim(6)
    assert hashlib.sha256(sd.astype(np.int32).tobytes()).hexdigest() == str(fx["shuffle6_sha256"])
    assert np.array_equal(sd[fx["shuffle6_pos"]], fx["shuffle6_val"])
    hs6 = np.load(os.path.join(GOLD, "kssd_shuffle_hs6.npz"))
    assert np.array_equal(sd[:64], hs6["head"]) and np.array_equal(sd[hs6["dim_id"]], hs6["rank"])
    # half_subk 7 (--drlevel 5): 2^28 entries, hashed in place and freed rather than cached like the hs6 table
    ptr = oracle.lib().orc_kssd_shuffle_dim(7)
    try:
        t7 = np.ctypeslib.as_array(ptr, shape=(1 << 28,))
        assert hashlib.sha256(memoryview(t7)).hexdigest() == str(fx["shuffle7_sha256"])
        assert np.array_equal(t7[fx["shuffle7_pos"]], fx["shuffle7_val"])
        del t7
    finally:
        C.CDLL(None).free(C.cast(ptr, C.c_void_p))


def test_reference_functions_live_against_fixture(oracle):
    """The stored grids are what make_golden.py's generators produce.  Where oracle/_ref is built (a checkout beside the
    reference tree), the reference's functions also run again on them; elsewhere that half has nothing to run and says so
    with a warning, like the kseq test, while the fixture itself is checked by the tests above."""
    import warnings
    mg = _make_golden()
    fx = _ref_fixture()
    d, k = mg.radio_grid()
    assert np.array_equal(d, fx["radio_d"]) and np.array_equal(k, fx["radio_k"])
    assert np.array_equal(mg.mash_grid(), fx["mash_args"])
    if not os.path.exists(mg.REF_FNS):
        warnings.warn("oracle/_ref/libref_fns.so is not built: the reference's functions were not re-run")
        return
    L = mg.ref_fns_lib()
    calr = np.array([L.ref_calr(a, b - 1) for a, b in zip(d, k)])
    assert np.array_equal(calr.view(np.uint64), fx["calr"].view(np.uint64))
    msr = np.array([L.ref_calculate_max_size_ratio(a, b) for a, b in zip(d, k)])
    assert np.array_equal(msr.view(np.uint64), fx["max_size_ratio"].view(np.uint64))
    md = np.array([L.ref_mash_distance_fast(*map(int, r)) for r in fx["mash_args"]])
    assert np.array_equal(md.view(np.uint64), fx["mash_dist"].view(np.uint64))
    for i, (n, e, thr) in enumerate(mg.kruskal_cases()):
        assert np.array_equal(e, fx[f"kr{i}_edges"]) and np.array_equal(thr, fx[f"kr{i}_thr"])
        for t, th in enumerate(thr):
            tree, forest = mg.ref_kruskal_forest(L, e, n, th)
            assert np.array_equal(tree, fx[f"kr{i}_tree"]) and np.array_equal(forest, fx[f"kr{i}_forest{t}"]), (i, t)
    t6 = mg.ref_shuffle_dim(L, 6)
    assert np.array_equal(t6, oracle.kssd_shuffle_dim(6))


def _overflow_sets():
    """MinHash-like u64 sets that share hashes: four of s = 1000, two containment-sized (5.0e4, 5.2e4), one of 6.0e5 and
    sketches of 1 and 3 hashes inside it"""
    rng = np.random.default_rng(77)
    pool = np.unique(rng.integers(1, 1 << 62, size=700_000, dtype=np.uint64))
    rng.shuffle(pool)
    big = np.sort(pool[:600_000])
    sets = [np.sort(np.concatenate([pool[:200], pool[1000 + 800 * i:1000 + 800 * (i + 1)]])) for i in range(4)]
    sets += [np.sort(pool[100:50_100]), np.sort(pool[150:52_150]), big, np.sort(pool[:1]), np.sort(pool[5:8])]
    return sets


@pytest.mark.parametrize("containment", [False, True])
@pytest.mark.parametrize("thr", [0.62, 0.7, 0.8])
def test_oracle_mst_size_filter_past_32_bits(oracle, thr, containment):
    """R * min past 2^31 (d = 0.7: R = 2 405 207, R * 1000 wraps negative in the reference's int product; d = 0.8: wraps
    positive; d = 0.62: control, R * 1000 fits but R * 6e5 / R * 1 decides one pair).  The oracle must equal the exact filter."""
    sets = _overflow_sets()
    flat, start, lens = oracle.to_csr(sets)
    from oracle.brute import mst_forest, partition
    cand, forest = mst_forest(sets, 21, containment, thr)
    got = oracle.mst(flat, start, lens, 21, containment, thr, threads=1)
    assert len(got) == len(forest)
    assert np.array_equal(np.sort(got["dist"]).view(np.uint64), np.sort(np.array([f[0] for f in forest])).view(np.uint64))
    want_part = partition(forest, len(sets))
    assert sorted(tuple(sorted(c)) for c in oracle.forest_clusters(got, 1.0, len(sets))) == want_part
    # the 1-hash sketch and the 6e5 one: ratio 600 000 -- above R = 485 601 at 0.62, below R at 0.7 and 0.8
    pair = any(i == 7 and j == 6 for _, i, j in cand)
    assert pair == (thr > 0.62)
    assert len(cand) >= 30
