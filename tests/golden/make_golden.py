"""Generates the committed fixtures under tests/golden/.  Run in the build container:

    python tests/golden/make_golden.py                              # every fixture
    python tests/golden/make_golden.py ref_dbscan ref_postprocess   # only the named reference pins

Two kinds of fixtures, labelled in MANIFEST.json:
  * "reference": outputs of the reference's own code run here -- oracle/_ref/libref_harness.so is
    compiled from the reference's src/{kseq.h,UnionFind.h} where they lie, oracle/_ref/libref_fns.so from its
    self-contained distance-half functions (oracle/Makefile, REF_FNS).  They pin the host FASTA reader, the
    union-find, the size-ratio bound, the KSSD greedy distance, Kruskal + the forest cut and the KSSD shuffle table.
    oracle/_ref/libref_dbscan.so and libref_post.so are the reference's src/dbscan.cpp and src/cluster_postprocess.cpp
    compiled whole; they pin the DBSCAN labels and printed file and the --dedup-dist / --reps-per-cluster lists.
  * "oracle": outputs of oracle/ (the CPU restatement).  They let the GPU box check the HIP path
    without regenerating expectations, and freeze the oracle against accidental edits.  The MinHash
    ones are NOT pinned against upstream RabbitSketch (see oracle/rtc_oracle.h).
"""
import ctypes as C
import gzip
import hashlib
import json
import math
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O  # noqa: E402
from tests import reflib, refpin_cases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
REF_FNS = os.path.join(ROOT, "oracle", "_ref", "libref_fns.so")
EDGE_DT = np.dtype([("preNode", np.int32), ("sufNode", np.int32), ("dist", np.float64)])  # the reference's EdgeInfo
SHUFFLE_HALF_SUBK = (6, 7)  # half_subk = 6 for --drlevel 0..4, drlevel + 2 = 7 for 5; 8 would overflow 1 << 4 * half_subk


def ref_fns_lib(path=REF_FNS):
    """oracle/_ref/libref_fns.so: the reference's distance-half functions behind oracle/ref_fns_shims.inc"""
    L = C.CDLL(path)
    L.ref_calr.restype = L.ref_calculate_max_size_ratio.restype = L.ref_mash_distance_fast.restype = C.c_double
    L.ref_calr.argtypes = L.ref_calculate_max_size_ratio.argtypes = [C.c_double, C.c_int]
    L.ref_mash_distance_fast.argtypes = [C.c_int] * 4
    L.ref_kruskal_forest.restype = C.c_uint64
    L.ref_kruskal_forest.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    L.ref_generate_shuffle_dim.restype = C.c_int
    L.ref_generate_shuffle_dim.argtypes = [C.c_int, C.c_void_p]
    return L


def ref_kruskal_forest(L, edges, n, thr):
    """(tree, forest) of kruskalAlgorithm + generateForest over edges (EDGE_DT, sorted by dist)"""
    edges = np.ascontiguousarray(edges, dtype=EDGE_DT)
    tree = np.zeros(max(n, 1), dtype=EDGE_DT)
    forest = np.zeros(max(n, 1), dtype=EDGE_DT)
    tm = C.c_uint64()
    fm = L.ref_kruskal_forest(edges.ctypes.data, len(edges), n, thr, tree.ctypes.data, C.byref(tm), forest.ctypes.data)
    return tree[:tm.value], forest[:fm]


def ref_shuffle_dim(L, half_subk):
    out = np.empty(1 << 4 * half_subk, dtype=np.int32)
    assert L.ref_generate_shuffle_dim(half_subk, out.ctypes.data) == len(out)
    return out


def shuffle_sample_positions(half_subk):
    """the table positions a fixture stores: the first 64 and 4096 seeded ones"""
    n = 1 << 4 * half_subk
    return np.concatenate([np.arange(64), np.random.default_rng(half_subk).integers(0, n, size=4096)]).astype(np.int64)


def radio_grid():
    """(d, k) points of the calr / calculateMaxSizeRatio table: d on a 0..1 grid and, for every k, where
    2 e^(d (k-1)) - 1 crosses 2^31 - 1, 2^31 and 2^32 (and one ulp either side), plus the thresholds the tests use"""
    ds, ks = [], []
    for k in range(1, 33):
        pts = list(np.linspace(0.0, 1.0, 101)) + [0.05, 0.62, 0.6931471805862327, 0.7, 0.8]
        if k > 1:
            for v in (2.0 ** 31 - 1, 2.0 ** 31, 2.0 ** 32):
                x = math.log((v + 1.0) / 2.0) / (k - 1)
                pts += [np.nextafter(x, -1.0), x, np.nextafter(x, 2.0)]
        pts = sorted(set(float(p) for p in pts if 0.0 <= p <= 1.0))
        ds += pts
        ks += [k] * len(pts)
    return np.array(ds, dtype=np.float64), np.array(ks, dtype=np.int32)


def mash_grid():
    """(common, size0, size1, k) points of calculate_mash_distance_fast: zeros, denominator 0, common = size, j = 1/s (the
    tuning's max distance), distances past 1 (clamped), large sizes (size0 + size1 below 2^31: the reference's int sum)"""
    rng = np.random.default_rng(11)
    pts = []
    for k in (1, 2, 5, 12, 16, 19, 21, 22, 24, 31, 32):
        for s0, s1 in [(0, 0), (0, 7), (7, 0), (1, 1), (1, 1000), (1000, 1000), (997, 1003), (1, 100000), (60000, 60000),
                       (5_000_000, 3), (1 << 29, 1 << 29), ((1 << 30) - 1, 1 << 30)]:
            for c in {0, 1, 2, min(s0, s1), max(min(s0, s1) - 1, 0), min(s0, s1) // 2, s0 + s1}:
                if s0 + s1 - c < (1 << 31):
                    pts.append((c, s0, s1, k))
        for s in (100, 1000, 5000, 10000, 60000, 100000):  # tune_parameters: maxDist at minJaccard = 1/sketchSize
            pts.append((1, 1, s, k))
        for _ in range(40):
            s0, s1 = (int(x) for x in rng.integers(1, 200_000, size=2))
            pts.append((int(rng.integers(0, min(s0, s1) + 1)), s0, s1, k))
    return np.array(sorted(set(pts)), dtype=np.int32)


def kruskal_cases():
    """seeded edge lists sorted by distance (stable), many equal distances; thresholds on an edge's distance and one ulp
    either side"""
    cases = []
    for seed, n, m, levels in [(1, 30, 80, 6), (2, 200, 900, 12), (3, 500, 3000, 40), (4, 64, 2016, 3), (5, 1, 0, 1),
                               (6, 2, 1, 1), (7, 300, 200, 1000)]:
        rng = np.random.default_rng(100 + seed)
        pre = rng.integers(0, n, size=m).astype(np.int32)
        suf = rng.integers(0, n, size=m).astype(np.int32)
        dist = (rng.integers(0, levels, size=m) / levels * 0.3).astype(np.float64)
        e = np.zeros(m, dtype=EDGE_DT)
        e["preNode"], e["sufNode"], e["dist"] = pre, suf, dist
        e = e[np.argsort(e["dist"], kind="stable")]
        thr = [0.0, 0.05, 1.0]
        for d in (e["dist"][m // 3:m // 3 + 1].tolist() + e["dist"][m // 2:m // 2 + 1].tolist() if m else []):
            thr += [np.nextafter(d, -1.0), d, np.nextafter(d, 2.0)]
        cases.append((n, e, np.array(thr, dtype=np.float64)))
    return cases


def write_ref_distance_half(L):
    """ref_distance_half.npz: the reference's own calr / calculateMaxSizeRatio, calculate_mash_distance_fast,
    kruskalAlgorithm + generateForest and generate_shuffle_dim, evaluated here on fixed grids"""
    out = {}
    d, k = radio_grid()
    out["radio_d"], out["radio_k"] = d, k
    out["calr"] = np.array([L.ref_calr(a, b - 1) for a, b in zip(d, k)], dtype=np.float64)  # calr(threshold, k - 1)
    out["max_size_ratio"] = np.array([L.ref_calculate_max_size_ratio(a, b) for a, b in zip(d, k)], dtype=np.float64)
    g = mash_grid()
    out["mash_args"] = g
    out["mash_dist"] = np.array([L.ref_mash_distance_fast(*map(int, r)) for r in g], dtype=np.float64)
    for i, (n, e, thr) in enumerate(kruskal_cases()):
        out[f"kr{i}_n"] = np.array(n, dtype=np.int32)
        out[f"kr{i}_edges"] = e
        out[f"kr{i}_thr"] = thr
        tree = None
        for t, th in enumerate(thr):
            tree, forest = ref_kruskal_forest(L, e, n, th)
            out[f"kr{i}_forest{t}"] = forest
        out[f"kr{i}_tree"] = tree
    for hs in SHUFFLE_HALF_SUBK:
        t = ref_shuffle_dim(L, hs)
        pos = shuffle_sample_positions(hs)
        out[f"shuffle{hs}_sha256"] = np.array(hashlib.sha256(t.tobytes()).hexdigest())
        out[f"shuffle{hs}_pos"], out[f"shuffle{hs}_val"] = pos, t[pos]
        del t
    np.savez_compressed(os.path.join(HERE, "ref_distance_half.npz"), **out)
    return {"kind": "reference", "source": "calr, calculateMaxSizeRatio, calculate_mash_distance_fast, EdgeInfo, kruskalAlgorithm, "
            "generateForest, shuffle/shuffleN/generate_shuffle_dim via oracle/ref_fns_shims.inc: (d, k) and (common, size0, "
            "size1, k) grids, 7 sorted edge lists with thresholds on an edge and one ulp either side, SHA-256 + 4160 entries "
            "of the shuffle tables at half_subk 6 and 7",
            "pins": "reference-pinned: KSSD shuffle table, size-ratio radio, kruskalAlgorithm + generateForest cut, KSSD greedy "
            "distance, tune_parameters' max distance; still restated: the MinHash k-mer hash and the MST loop's inline distance",
            "filter": "deliberate divergence: a pair is kept iff max <= R * min in exact (64-bit) integers, R = floor(calr) saturated "
            "at INT32_MAX; the reference's int conversion and int product overflow past 2^31 (DESIGN 5)"}


def write_ref_dbscan(L):
    """ref_dbscan.npz: the reference's KssdDBSCAN + printKssdDBSCANResult on refpin_cases.dbscan_cases(): labels, cluster /
    noise / core counts and the SHA-256 of the printed file per case, and a SHA-256 per input set.  Inputs are not stored:
    refpin_cases rebuilds them.  Every case runs with 1 and with 4 threads; the two must agree."""
    import re
    cases = refpin_cases.dbscan_cases()
    labels, ncl, nnoise, ncore, shas, inputs = [], [], [], [], [], {}
    for i, case in enumerate(cases):
        gen, args, eps, min_pts, k, mp = case
        sk = refpin_cases.sketches_of(gen, args)
        use64 = refpin_cases.use64_of(sk)
        inputs[json.dumps([gen, args], sort_keys=True)] = refpin_cases.input_sha(sk)
        by_file = refpin_cases.print_layout(i)
        lab, text, log = reflib.kssd_dbscan_print(L, sk, use64, eps, min_pts, k, refpin_cases.genomes_of(len(sk), by_file), by_file,
                                                  threads=1, max_posting=mp)
        lab4, c4, n4 = reflib.kssd_dbscan(L, sk, use64, eps, min_pts, k, threads=4, max_posting=mp)
        assert np.array_equal(lab, lab4), case
        m = re.search(r"-----Core points: (\d+) ", log)
        labels.append(lab)
        ncl.append(c4)
        nnoise.append(n4)
        ncore.append(int(m.group(1)) if m else 0)
        shas.append(hashlib.sha256(text).hexdigest())
    cli = []  # the printed file under the names clust-dbscan's own run gives the genomes (tests/test_gpu_refpin.py)
    sk = refpin_cases.sketches_of("kssd_family", refpin_cases.KSSD_FAMILY_CLI)
    for eps, min_pts, by_file in refpin_cases.CLI_RUNS:
        _, text, _ = reflib.kssd_dbscan_print(L, sk, False, eps, min_pts, 17, refpin_cases.cli_genomes(by_file), by_file, threads=4)
        cli.append(hashlib.sha256(text).hexdigest())
    off = np.zeros(len(cases) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in labels], out=off[1:])
    np.savez_compressed(os.path.join(HERE, "ref_dbscan.npz"), cli_sha256=np.array(cli), cases=np.array(json.dumps([list(c) for c in cases], sort_keys=True)),
                        inputs=np.array(json.dumps(inputs, sort_keys=True)), labels_flat=np.concatenate(labels).astype(np.int32),
                        labels_off=off, n_clusters=np.array(ncl, dtype=np.int32), n_noise=np.array(nnoise, dtype=np.int32),
                        n_core=np.array(ncore, dtype=np.int64), print_sha256=np.array(shas))
    return {"kind": "reference", "source": "KssdDBSCAN + printKssdDBSCANResult (src/dbscan.cpp compiled whole) via "
            "oracle/ref_dbscan_shims.cpp on tests/refpin_cases.py's %d cases: labels, cluster / noise / core counts, SHA-256 of the "
            "printed file; inputs by generator and seed with a SHA-256 each; threads 1 and 4 agreed on every case" % len(cases),
            "pins": "reference-pinned: tests/refdbscan.py (labels_of, print_result), rtc_dbscan, rtc_dbscan_sweep, clust-dbscan's "
            "output file; still restated only: tests/refkdist.py (the k-distance curve has no counterpart in the reference)",
            "refusal": "u32 sets with ceil(max size / jaccard_min) past INT_MAX: the reference's int conversion overflows and its "
            "labels differ from the restatement (recorded here); the kernels refuse them"}


def big_forests():
    """the 10 000-member groups of tests/test_gpu_postprocess.py"""
    from tests import test_gpu_postprocess as T
    return [(shape, weights) + T._forest(11, [10_000, 3000, 40, 2], shape, weights)
            for shape, weights in [("chain", "rand"), ("star", "tie"), ("random", "tie"), ("random", "rand")]]


def write_ref_postprocess(L):
    """ref_postprocess.npz: the reference's build_dedup_candidates_per_cluster (KSSD overload) and
    select_k_reps_per_cluster_tree on refpin_cases.forest_case(seed): node_to_rep and the candidate lists per dedup distance,
    the representative lists per k; node_to_rep of the forests of tests/test_gpu_postprocess.py (CASES and the 10 000-member
    groups) at dedup distance 0.01."""
    rep_flat, lists, shape = [], [], []
    for seed in refpin_cases.FOREST_SEEDS:
        n, edges, lens, dedups, ks = refpin_cases.forest_case(seed)
        clusters = refpin_cases.components(n, edges)
        shape.append((n, len(edges), len(clusters)))
        for di, dd in enumerate(dedups):
            rep, cand = reflib.dedup_candidates(L, n, clusters, edges, lens, dd, by_file=(seed + di) % 2 == 0)
            rep_flat += rep
            lists += cand
            for k in ks:
                lists += reflib.select_k_reps(L, n, clusters, cand, edges, rep, k)
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    out = dict(shape=np.array(shape, dtype=np.int32), rep_flat=np.array(rep_flat, dtype=np.int32),
               lists_flat=np.array([v for x in lists for v in x], dtype=np.int32), lists_off=off)
    for i, (_, _, n, edges, lens) in enumerate(big_forests()):
        rep, _ = reflib.dedup_candidates(L, n, [list(range(n))], edges, [int(x) for x in lens], 0.01)
        out["big%d_rep" % i] = np.array(rep, dtype=np.int32)
    from tests import test_gpu_postprocess as T
    for i, (seed, sizes, shp, weights) in enumerate(T.CASES):
        n, edges, lens = T._forest(seed, sizes, shp, weights)
        rep, _ = reflib.dedup_candidates(L, n, [list(range(n))], edges, [int(x) for x in lens], 0.01)
        out["small%d_rep" % i] = np.array(rep, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "ref_postprocess.npz"), **out)
    return {"kind": "reference", "source": "build_dedup_candidates_per_cluster (KSSD overload) + select_k_reps_per_cluster_tree "
            "(src/cluster_postprocess.cpp compiled whole) via oracle/ref_post_shims.cpp on tests/refpin_cases.py's %d seeded forests "
            "(chains, stars, caterpillars, random trees; tied and distinct weights and lengths; dedup 0, 0.005, 0.01, 0.015, 1.0, "
            "on an edge weight and one ulp either side; k 0, 1, 2, 3, 1000) and node_to_rep of tests/test_gpu_postprocess.py's "
            "forests, four with 10 000-member groups" % len(refpin_cases.FOREST_SEEDS),
            "pins": "reference-pinned: tests/refpost.py (tree_medoids, dedup_candidates, select_k_reps), rtc_tree_medoids on the GPU "
            "and host paths; still restated only: tests/refmststate.py, tests/refmstdb.py and refpost.py's --auto-threshold / "
            "--stability analysis (src/MST.cpp needs the whole sketch library to compile)"}


REF_PINS = {"ref_dbscan": (reflib.ref_dbscan, write_ref_dbscan), "ref_postprocess": (reflib.ref_post, write_ref_postprocess)}


def write_ref_pins(manifest, names):
    for name in names:
        load, write = REF_PINS[name]
        L = load()
        if L is None:
            raise SystemExit("oracle/_ref/lib%s.so missing: run `make -C oracle` where the reference tree exists"
                             % name.replace("postprocess", "post"))
        manifest[name + ".npz"] = write(L)


def write_fasta_inputs():
    rng = np.random.default_rng(2024)

    def seq(n):
        return "".join(rng.choice(list("ACGT"), size=n))
    files = {}
    s1 = seq(500)
    files["plain.fa"] = ">chr1 first record comment\n" + "\n".join(s1[i:i + 80] for i in range(0, 500, 80)) + "\n" \
        ">chr2\n" + seq(130) + "\n>chr3\tTabbed comment here\n" + seq(77) + "\n"
    files["crlf_blank.fa"] = ">a desc\r\n" + seq(60) + "\r\n\r\n" + seq(45) + "\r\n>b\r\nACGTNNNNacgtRYK\r\n"
    files["noeol.fa"] = ">only_name\n" + seq(100)
    files["leading_junk.fa"] = "junk line before any header\n\n>x  two  spaces\nAC\nGT\n\n>y z\n\n>z\nTTTT"
    files["reads.fq"] = "@r1 fastq comment\nACGTACGTAC\n+\nIIIIIIIIII\n@r2\nGGGGCCCC\nTT\n+r2\nIIIIIIII\nII\n"
    files["empty.fa"] = ""
    for name, text in files.items():
        with open(os.path.join(HERE, "fasta", name), "w", newline="") as f:
            f.write(text)
    with open(os.path.join(HERE, "fasta", "plain.fa.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(files["plain.fa"].encode())
    return sorted(list(files) + ["plain.fa.gz"])


def _kseq_dump(ref, path):
    need = ref.ref_kseq_dump(path.encode(), None, 0)
    if need < 0:
        return None
    buf = C.create_string_buffer(max(need, 1))
    ref.ref_kseq_dump(path.encode(), buf, need)
    return buf.raw[:need]


def write_kseq_random(ref):
    """kseq_random.npz: 20 random FASTA texts (headers of odd characters, CR/LF, blank lines, empty records) and one gzip
    member of five long records, with what the reference's kseq reads from each (the gzip layouts: SHA-256 and length of
    the dump; -1 where kseq reports an error)."""
    rng = np.random.default_rng(9)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for t in range(20):
            parts = []
            for r in range(int(rng.integers(0, 5))):
                hdr = ">" + "".join(rng.choice(list("abcXYZ_ \t|.:"), size=int(rng.integers(0, 20))))
                eol = "\r\n" if rng.random() < 0.3 else "\n"
                parts.append(hdr + eol)
                for _ in range(int(rng.integers(0, 4))):
                    parts.append("".join(rng.choice(list("ACGTNacgt"), size=int(rng.integers(0, 90)))) + eol)
                    if rng.random() < 0.2:
                        parts.append(eol)
            text = "".join(parts).encode()
            p = os.path.join(tmp, f"r{t}.fa")
            open(p, "wb").write(text)
            want = _kseq_dump(ref, p)
            out[f"rand{t}_in"] = np.frombuffer(text, dtype=np.uint8)
            out[f"rand{t}_want"] = np.frombuffer(want if want is not None else b"", dtype=np.uint8)
            out[f"rand{t}_ok"] = np.array(want is not None)
        body = "".join(">rec%d some text\n" % r + "\n".join("".join(rng.choice(list("ACGTNacgt"), size=70)) for _ in range(400)) + "\n"
                       for r in range(5)).encode()
        one = gzip.compress(body, 6, mtime=0)
        out["gz_one"] = np.frombuffer(one, dtype=np.uint8)
        # the layouts the test builds from the stored member: one member, two members, many small members (bgzip style),
        # a file cut short, bytes behind the last member, an empty member
        cases = {
            "one.fa.gz": one,
            "two.fa.gz": gzip.compress(body[:70_000], 6) + gzip.compress(body[70_000:], 1),
            "many.fa.gz": b"".join(gzip.compress(body[i:i + 9_000], 4) for i in range(0, len(body), 9_000)),
            "cut.fa.gz": one[:-1500],
            "trail.fa.gz": one + b"trailing bytes that are no gzip member",
            "hole.fa.gz": gzip.compress(body[:50_000], 6) + gzip.compress(b"", 6) + gzip.compress(body[50_000:], 6),
        }
        for name, data in cases.items():
            p = os.path.join(tmp, name)
            open(p, "wb").write(data)
            want = _kseq_dump(ref, p)
            key = name.split(".")[0]
            out[f"gz_{key}_len"] = np.array(-1 if want is None else len(want), dtype=np.int64)
            out[f"gz_{key}_sha256"] = np.array(hashlib.sha256(want or b"").hexdigest())
    np.savez_compressed(os.path.join(HERE, "kseq_random.npz"), **out)
    return {"kind": "reference", "source": "kseq.h via oracle/ref_harness.cpp on 20 random FASTA texts and 6 gzip layouts"}


def main():
    if len(sys.argv) > 1:  # only the named reference pins; the other entries of the manifest stay
        with open(os.path.join(HERE, "MANIFEST.json")) as f:
            manifest = json.load(f)
        write_ref_pins(manifest, sys.argv[1:])
        with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
        print("wrote", sys.argv[1:])
        return
    manifest = {}
    names = write_fasta_inputs()
    if not os.path.exists(REF):
        raise SystemExit("oracle/_ref/libref_harness.so missing: run `make -C oracle` where /root/reference exists")
    ref = C.CDLL(REF)
    ref.ref_kseq_dump.restype = C.c_long
    manifest["kseq_random.npz"] = write_kseq_random(ref)
    for n in names:
        p = os.path.join(HERE, "fasta", n).encode()
        need = ref.ref_kseq_dump(p, None, 0)
        buf = C.create_string_buffer(max(need, 1))
        ref.ref_kseq_dump(p, buf, need)
        with open(os.path.join(HERE, "kseq_dump_" + n + ".txt"), "wb") as f:
            f.write(buf.raw[:need])
        manifest["kseq_dump_" + n + ".txt"] = {"kind": "reference", "source": "kseq.h via oracle/ref_harness.cpp"}
    # union-find roots after a fixed merge sequence
    rng = np.random.default_rng(7)
    n, m = 200, 150
    xs = rng.integers(0, n, size=m).astype(np.int32)
    ys = rng.integers(0, n, size=m).astype(np.int32)
    roots = np.zeros(n, dtype=np.int32)
    size = C.c_int()
    ref.ref_unionfind(n, xs.ctypes.data_as(C.c_void_p), ys.ctypes.data_as(C.c_void_p), m,
                      roots.ctypes.data_as(C.c_void_p), C.byref(size))
    np.savez(os.path.join(HERE, "unionfind.npz"), xs=xs, ys=ys, roots=roots, size=size.value)
    manifest["unionfind.npz"] = {"kind": "reference", "source": "UnionFind.h via oracle/ref_harness.cpp"}

    # ---- the reference's distance half ----
    if not os.path.exists(REF_FNS):
        raise SystemExit("oracle/_ref/libref_fns.so missing: run `make -C oracle` where the reference tree exists")
    fns = ref_fns_lib()
    manifest["ref_distance_half.npz"] = write_ref_distance_half(fns)
    sd = ref_shuffle_dim(fns, 6)
    kept = np.nonzero(sd < 4096)[0].astype(np.uint32)
    np.savez_compressed(os.path.join(HERE, "kssd_shuffle_hs6.npz"), dim_id=kept, rank=sd[kept].astype(np.uint16),
                        head=sd[:64].astype(np.int32))
    manifest["kssd_shuffle_hs6.npz"] = {"kind": "reference", "source": "generate_shuffle_dim(6) via oracle/ref_fns_shims.inc "
                                        "(glibc srand/rand); 4096 surviving (dim_id, rank) pairs + first 64 table entries"}

    write_ref_pins(manifest, sorted(REF_PINS))

    # ---- oracle fixtures ----
    L = 60_000
    descs = [(11, 0, 0, 0), (11, 5, 300, 0), (11, 6, 900, 0), (12, 0, 0, 0), (12, 9, 500, 7000), (13, 0, 0, 0)]
    genomes = [O.synth_genome(f, m_, t, L, ne) for (f, m_, t, ne) in descs]
    seq = np.concatenate(genomes)
    off = np.arange(len(genomes) + 1, dtype=np.uint64) * L
    mh = O.sketch_minhash_batch(seq, off, 21, 400, threads=1)
    ks = [O.kssd_sketch(g, 21, 3) for g in genomes]
    flat, start, lens = O.to_csr(mh)
    mst = O.mst(flat, start, lens, 21, 0, 0.05, threads=1)
    np.savez_compressed(os.path.join(HERE, "sketch_fixture.npz"), descs=np.array(descs, dtype=np.uint64), L=L,
                        minhash=np.array(mh, dtype=object), kssd=np.array(ks, dtype=object),
                        mst=mst, allow_pickle=True)
    manifest["sketch_fixture.npz"] = {"kind": "oracle", "source": "6 synthetic 60 kbp genomes: MinHash k=21 s=400 "
                                      "(parity unpinned vs RabbitSketch), KSSD k=21 dr=3, MST at d=0.05"}
    vec = []
    for key, seed in [(b"", 0), (b"A", 42), (b"ACGTACGTACGTACGTACGTA", 42), (b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT", 42),
                      (bytes(range(40)), 7)]:
        h1, h2 = O.murmur3_x64_128(key, seed)
        vec.append({"key_hex": key.hex(), "seed": seed, "h1": h1, "h2": h2})
    with open(os.path.join(HERE, "murmur3_vectors.json"), "w") as f:
        json.dump({"smhasher_verification": hex(O.lib().orc_murmur3_smhasher_verification()), "vectors": vec}, f, indent=1)
    manifest["murmur3_vectors.json"] = {"kind": "oracle", "source": "orc_murmur3_x64_128, itself pinned by the public "
                                        "SMHasher verification value 0x6384BA69"}
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(manifest), "fixtures")


if __name__ == "__main__":
    main()
