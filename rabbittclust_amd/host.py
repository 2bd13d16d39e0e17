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


def leiden_quantiser(weight, objective):
    """leiden_quantiser (rtc_host.cpp): what a clust-leiden run's quantisation keeps for its model -> (scale, lo, range, narrow)"""
    w = np.ascontiguousarray(weight, dtype=np.float64)
    scale, lo, rng = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    fn = load().rtch_leiden_quantiser
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    narrow = fn(w.ctypes.data_as(C.c_void_p), len(w), int(objective), C.byref(scale), C.byref(lo), C.byref(rng))
    return bool(scale.value), float(lo.value), float(rng.value), bool(narrow)


def leiden_quantise_weight(weight, objective, scale=False, lo=0.0, rng=1.0):
    """leiden_quantise_weight (rtc_host.cpp): q of one weight as the model's run formed it, 0 where the record drops out"""
    fn = load().rtch_leiden_quantise_weight
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_double, C.c_int, C.c_int, C.c_double, C.c_double]
    return int(fn(float(weight), int(objective), int(bool(scale)), float(lo), float(rng)))


def leiden_assign_weights(edges, model_sizes, query_sizes, kmer_size, objective, scale=False, lo=0.0, rng=1.0, threads=1):
    """leiden_assign_weights (rtc_host.cpp): the records of Context.graph_query (q, p, common) to (u: query, v: model genome, q)
    records through rtc_graph_weight and the model's quantisation, on `threads` host threads"""
    from . import _lib
    e = np.ascontiguousarray(edges)
    ms = np.ascontiguousarray(model_sizes, dtype=np.uint32)
    qs = np.ascontiguousarray(query_sizes, dtype=np.uint32)
    out = np.zeros(max(len(e), 1), dtype=[("u", "<u4"), ("v", "<u4"), ("q", "<u4")])
    n_out = C.c_uint64(0)
    wf = C.cast(_lib.load().rtc_graph_weight, C.c_void_p)
    fn = load().rtch_leiden_assign_weights
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                   C.c_void_p, C.POINTER(C.c_uint64)]
    fn(e.ctypes.data_as(C.c_void_p), len(e), ms.ctypes.data_as(C.c_void_p), qs.ctypes.data_as(C.c_void_p), int(kmer_size), wf, int(objective),
       int(bool(scale)), float(lo), float(rng), int(threads), out.ctypes.data_as(C.c_void_p), C.byref(n_out))
    return out[:n_out.value].copy()


def leiden_model_sums(records, labels, n_clusters):
    """leiden_model_sums (rtc_host.cpp): (k per genome, tot per cluster, M2, size per cluster) of a run's records and labels"""
    r = np.ascontiguousarray(records, dtype=[("u", "<u4"), ("v", "<u4"), ("q", "<u4")])
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    n, nc = len(lab), int(n_clusters)
    k, tot, size, m2 = np.zeros(max(n, 1), np.uint64), np.zeros(max(nc, 1), np.uint64), np.zeros(max(nc, 1), np.uint64), C.c_uint64(0)
    fn = load().rtch_leiden_model_sums
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    if fn(r.ctypes.data_as(C.c_void_p), len(r), lab.ctypes.data_as(C.c_void_p), n, nc, k.ctypes.data_as(C.c_void_p),
          tot.ctypes.data_as(C.c_void_p), size.ctypes.data_as(C.c_void_p), C.byref(m2)) != 0:
        raise ValueError("a record or a label is out of range")
    return k[:n].copy(), tot[:nc].copy(), int(m2.value), size[:nc].copy()


def leiden_model_save(path, head, min_len, threshold, resolution, lo, rng, m2, labels, tot, names, lens, sketches):
    """save_leiden_model (rtc_host.cpp) from its parts; head: algorithm, objective, width, sketch_by_file, kmer_size, half_k,
    half_subk, drlevel, knn, n_clusters, scale"""
    head = np.ascontiguousarray(head, dtype=np.int32)
    assert head.shape == (11,)
    width = int(head[2])
    dt = np.uint64 if width == 8 else np.uint32
    n = len(labels)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    t = np.ascontiguousarray(tot, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in sketches])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=dt) for s in sketches]) if n else np.zeros(1, dtype=dt))
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
    fn = load().rtch_leiden_model_save
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn(str(path).encode(), head.ctypes.data_as(C.c_void_p), int(min_len), float(threshold), float(resolution), float(lo), float(rng),
              int(m2), n, lab.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), arr, ln.ctypes.data_as(C.c_void_p),
              flat.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))


def leiden_model_resave(in_path, out_path):
    """load_leiden_model, then save_leiden_model -> (0, "") or (-1, the loader's reason)"""
    why = C.create_string_buffer(256)
    fn = load().rtch_leiden_model_resave
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    rc = fn(str(in_path).encode(), str(out_path).encode(), why, 256)
    return rc, why.value.decode()


def nj_newick(labels, members, joins):
    """get_nj_newick (rtc_host.cpp): the Newick text of one neighbour-joining tree.  labels[g]: the label of genome g; members: the
    genome indices of the tree; joins: its rtc_njoin records (api.NJOIN_DT), a, b and c as genome indices."""
    mem = np.ascontiguousarray(sorted(int(g) for g in members), dtype=np.uint32)
    j = np.ascontiguousarray(joins)
    assert j.dtype.itemsize == 40
    arr = (C.c_char_p * max(len(labels), 1))(*[s.encode() for s in labels])
    fn = load().rtch_nj_newick
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_long]
    need = fn(arr, mem.ctypes.data_as(C.c_void_p), len(mem), j.ctypes.data_as(C.c_void_p), len(j), None, 0)
    buf = C.create_string_buffer(max(int(need), 1))
    fn(arr, mem.ctypes.data_as(C.c_void_p), len(mem), j.ctypes.data_as(C.c_void_p), len(j), buf, need)
    return buf.raw[:need].decode()


def nj_support_newick(labels, members, joins, support, replicates):
    """nj_support_newick_text (rtc_host.cpp): nj_newick's text with the support of every node that names a split, in percent (half
    up), between its ")" and its ":".  support: one count per record (Context.nj_support's), of `replicates`."""
    mem = np.ascontiguousarray(sorted(int(g) for g in members), dtype=np.uint32)
    j = np.ascontiguousarray(joins)
    sup = np.ascontiguousarray(support, dtype=np.uint32)
    assert j.dtype.itemsize == 40 and len(sup) == len(j)
    if int(replicates) < 1:
        raise ValueError("replicates must be at least 1")
    arr = (C.c_char_p * max(len(labels), 1))(*[s.encode() for s in labels])
    fn = load().rtch_nj_support_newick
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_long]
    args = (arr, mem.ctypes.data_as(C.c_void_p), len(mem), j.ctypes.data_as(C.c_void_p), len(j), sup.ctypes.data_as(C.c_void_p), int(replicates))
    need = fn(*args, None, 0)
    buf = C.create_string_buffer(max(int(need), 1))
    fn(*args, buf, need)
    return buf.raw[:need].decode()


def quality_report(names, cluster_of, records, sil):
    """quality_report_text (rtc_host.cpp): the two reports of clust-mst --quality as (quality_tsv, silhouette_tsv).  names[g] and
    cluster_of[g] (the cluster number <output> gives genome g) for every genome, records: api.SIL_DT, sil: their silhouettes."""
    n = len(names)
    lab = np.ascontiguousarray(cluster_of, dtype=np.int32)
    rec = np.ascontiguousarray(records)
    val = np.ascontiguousarray(sil, dtype=np.float64)
    assert rec.dtype.itemsize == 40 and len(lab) == len(rec) == len(val) == n
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
    fn = load().rtch_quality_report
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_long]
    if n and int(lab.min()) < 0:
        raise ValueError("cluster_of must name a cluster for every genome: the reports are of a run's clusters, which hold them all")
    ncl = int(lab.max()) + 1 if n else 0
    out = []
    for which in (0, 1):
        args = (arr, lab.ctypes.data_as(C.c_void_p), ncl, rec.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), n, which)
        need = fn(*args, None, 0)
        if need < 0:
            raise ValueError("cluster_of outside the clusters")
        buf = C.create_string_buffer(max(int(need), 1))
        fn(*args, buf, need)
        out.append(buf.raw[:need].decode())
    return tuple(out)


def upgma_newick(labels, members, merges):
    """upgma_newick_text (rtc_host.cpp): the Newick text of one average-linkage tree, node height = distance / 2.  labels[g]: the
    label of genome g; members: the genome indices of the tree; merges: its rtc_umerge records (api.UMERGE_DT), a and b as genome
    indices."""
    mem = np.ascontiguousarray(sorted(int(g) for g in members), dtype=np.uint32)
    j = np.ascontiguousarray(merges)
    assert j.dtype.itemsize == 24
    arr = (C.c_char_p * max(len(labels), 1))(*[s.encode() for s in labels])
    fn = load().rtch_upgma_newick
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_long]
    need = fn(arr, mem.ctypes.data_as(C.c_void_p), len(mem), j.ctypes.data_as(C.c_void_p), len(j), None, 0)
    buf = C.create_string_buffer(max(int(need), 1))
    fn(arr, mem.ctypes.data_as(C.c_void_p), len(mem), j.ctypes.data_as(C.c_void_p), len(j), buf, need)
    return buf.raw[:need].decode()


def upgma_keep(sum, size_a, size_b, threshold):
    """upgma_keep (rtc_host.cpp): the command line's integer cut rule for one merge"""
    fn = load().rtch_upgma_keep
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_double]
    return bool(fn(int(sum), int(size_a), int(size_b), float(threshold)))


def upgma_report(cluster_of, merges, first, threshold):
    """upgma_report (rtc_host.cpp): what clust-mst --upgma writes from the records of Context.upgma_clusters(sk, cluster_of, k) ->
    (the text of <output>.upgma.linkage.txt, the refined clusters at the threshold as lists of ascending genome indices ordered
    by smallest member, the merges kept).  cluster_of[g]: the cluster number <output> gives genome g."""
    lab = np.ascontiguousarray(cluster_of, dtype=np.int32)
    n = len(lab)
    mg = np.ascontiguousarray(merges)
    fs = np.ascontiguousarray(first, dtype=np.uint64)
    assert mg.dtype.itemsize == 24
    ncl = int(lab.max()) + 1 if n else 0
    assert len(fs) >= ncl + 1
    refined = np.full(max(n, 1), -1, dtype=np.int32)
    kept = C.c_uint64(0)
    fn = load().rtch_upgma_report
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_long]
    args = (lab.ctypes.data_as(C.c_void_p), ncl, n, mg.ctypes.data_as(C.c_void_p), fs.ctypes.data_as(C.c_void_p), float(threshold),
            refined.ctypes.data_as(C.c_void_p), C.byref(kept))
    need = fn(*args, None, 0)
    if need < 0:
        raise ValueError("cluster_of must number the clusters 0 .. n_clusters - 1, none of them empty")
    buf = C.create_string_buffer(max(int(need), 1))
    fn(*args, buf, need)
    out = [[] for _ in range(int(refined[:n].max()) + 1 if n else 0)]
    for g in range(n):
        out[int(refined[g])].append(g)
    return buf.raw[:need].decode(), out, int(kept.value)


def support_report(names, cluster_of, records, together, replicates):
    """support_report_text (rtc_host.cpp): the two reports of clust-mst --cluster-support as (support_tsv, genomes_tsv).  names[g]
    and cluster_of[g] (the cluster number <output> gives genome g) for every genome; records: api.CSUPPORT_DT, one per cluster in
    the library's order (that of the clusters' smallest members); together: Context.cluster_support's, one per genome."""
    n = len(names)
    lab = np.ascontiguousarray(cluster_of, dtype=np.int32)
    rec = np.ascontiguousarray(records)
    tog = np.ascontiguousarray(together, dtype=np.uint64)
    if n and int(lab.min()) < 0:
        raise ValueError("cluster_of must name a cluster for every genome")
    ncl = int(lab.max()) + 1 if n else 0
    assert rec.dtype.itemsize == 24 and len(lab) == len(tog) == n and len(rec) == ncl
    if int(replicates) < 1:
        raise ValueError("replicates must be at least 1")
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
    fn = load().rtch_support_report
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_long]
    out = []
    for which in (0, 1):
        args = (arr, lab.ctypes.data_as(C.c_void_p), ncl, rec.ctypes.data_as(C.c_void_p), tog.ctypes.data_as(C.c_void_p), n, int(replicates), which)
        need = fn(*args, None, 0)
        if need < 0:
            raise ValueError("cluster_of outside the clusters, or a cluster without a member")
        buf = C.create_string_buffer(max(int(need), 1))
        fn(*args, buf, need)
        out.append(buf.raw[:need].decode())
    return tuple(out)


def pangenome_report(names, cluster_of, clusters, hist, genomes):
    """pangenome_report_text (rtc_host.cpp): the four reports of clust-mst --pangenome as (pangenome_tsv, genomes_tsv, hist_tsv,
    curve_tsv).  names[g] and cluster_of[g] (the cluster number <output> gives genome g) for every genome; clusters (api.PAN_DT),
    hist and genomes (api.PAN_GENOME_DT): Context.pangenome's, the clusters in the library's order (that of their smallest
    members)."""
    n = len(names)
    lab = np.ascontiguousarray(cluster_of, dtype=np.int32)
    rec = np.ascontiguousarray(clusters)
    hs = np.ascontiguousarray(hist, dtype=np.uint64)
    gen = np.ascontiguousarray(genomes)
    if n and int(lab.min()) < 0:
        raise ValueError("cluster_of must name a cluster for every genome")
    ncl = int(lab.max()) + 1 if n else 0
    assert rec.dtype.itemsize == 64 and gen.dtype.itemsize == 32 and len(lab) == len(gen) == n and len(hs) >= n and len(rec) == ncl
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
    from . import _lib
    growth = C.cast(_lib.load().rtc_pan_growth, C.c_void_p)
    fn = load().rtch_pangenome_report
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    out = []
    for which in range(4):
        args = (arr, lab.ctypes.data_as(C.c_void_p), ncl, rec.ctypes.data_as(C.c_void_p), hs.ctypes.data_as(C.c_void_p),
                gen.ctypes.data_as(C.c_void_p), n, growth, which)
        need = fn(*args, None, 0)
        if need < 0:
            raise ValueError("cluster_of outside the clusters, a cluster without a member, or records that are not these clusters'")
        buf = C.create_string_buffer(max(int(need), 1))
        fn(*args, buf, need)
        out.append(buf.raw[:need].decode())
    return tuple(out)


def screen_report(names, rep_names, cluster_id, cluster_size, hits, sums, kmer_size):
    """screen_report_text (rtc_host.cpp): the two reports of clust-mst --db --screen as (screen_tsv, summary_tsv).  names[q]: the
    samples (an empty name prints as query_<q>); rep_names, cluster_id and cluster_size by slot; hits: api.SCREEN_HIT_DT sorted by
    sample, in Context.rep_screen's order; sums: api.SCREEN_SUM_DT, one per sample."""
    nq, nr = len(names), len(rep_names)
    hit = np.ascontiguousarray(hits)
    sm = np.ascontiguousarray(sums)
    cid = np.ascontiguousarray(cluster_id, dtype=np.int32)
    csz = np.ascontiguousarray(cluster_size, dtype=np.int32)
    assert hit.dtype.itemsize == 24 and sm.dtype.itemsize == 24 and len(sm) == nq and len(cid) == len(csz) == nr
    arr = (C.c_char_p * max(nq, 1))(*[s.encode() for s in names])
    rarr = (C.c_char_p * max(nr, 1))(*[s.encode() for s in rep_names])
    from . import _lib
    idf = C.cast(_lib.load().rtc_screen_identity, C.c_void_p)
    fn = load().rtch_screen_report
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p,
                   C.c_int, C.c_void_p, C.c_long]
    out = []
    for which in (0, 1):
        args = (arr, nq, rarr, cid.ctypes.data_as(C.c_void_p), csz.ctypes.data_as(C.c_void_p), nr, hit.ctypes.data_as(C.c_void_p), len(hit),
                sm.ctypes.data_as(C.c_void_p), int(kmer_size), idf, which)
        need = fn(*args, None, 0)
        if need < 0:
            raise ValueError("a hit names a sample or a slot out of range, or the hits are not sorted by sample")
        buf = C.create_string_buffer(max(int(need), 1))
        fn(*args, buf, need)
        out.append(buf.raw[:need].decode())
    return tuple(out)
