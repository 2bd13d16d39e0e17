"""clust-mst --nj-support on the device: the counting kernel's pair routine against numpy for every pair and all 64 lanes,
rtc_nj_support against the restatement (tests/refnjsupport.py) over family sets, its invariance under the joining path, the
grouping of the replicates and the fill's kernel, and the command line end to end.  Every comparison is exact."""
import functools
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import linkage_sets as S
from tests import nj_support_sets as NS
from tests import refnj as R
from tests import refnjsupport as RS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
WAVE, WORKGROUP, GRID = 1, 2, 4
CAP = 1024  # api.JK_LDS_ELEMS, asserted below


def _tuples(joins):
    return [(int(r["a"]), int(r["b"]), int(r["c"]), float(r["len_a"]), float(r["len_b"]), float(r["len_c"])) for r in joins]


@pytest.fixture
def switch(ctx, monkeypatch):
    names = set()

    def set_switch(name, v):
        names.add(name)
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
        ctx.reload_options()
    for name in ("RTC_NJ_GRID_MIN", "RTC_NJ_BYTES", "RTC_PAIR_FORCE_MERGE"):
        set_switch(name, None)
    yield set_switch
    for name in names:
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


def _sketch_set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=21, kind="kssd", width=width)


# ---- the counts ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _count_lists():
    """ascending lists of values below 2^32: the lengths 0, 1, 63, 64, 65, CAP and CAP + 1 drawn from one universe (so they
    overlap), copies of two of them (identical lists), a list from elsewhere (disjoint from all), and two pairs whose only match
    is the last element of the longer or of the shorter list; 0xFFFFFFFF ends two of the drawn lists"""
    rng = np.random.default_rng(11)
    universe = rng.choice(1 << 31, size=3 * CAP, replace=False).astype(np.uint64)
    top = np.uint64(0xFFFFFFFF)
    lists = []
    for n in (0, 1, 63, 64, 65, CAP, CAP + 1):
        lists.append(np.sort(rng.choice(universe, size=n, replace=False)))
    lists[3] = np.sort(np.concatenate([lists[3][:-1], [top]]))   # 64 elements, the last one 0xFFFFFFFF
    lists[6] = np.sort(np.concatenate([lists[6][:-1], [top]]))   # CAP + 1 elements, the last one 0xFFFFFFFF
    lists.append(lists[5].copy())                                # identical, at the cap
    lists.append(lists[6].copy())                                # identical, past it
    lists.append(np.arange(65, dtype=np.uint64) * 2 + (np.uint64(1) << np.uint64(31)) + np.uint64(1))  # disjoint from everything
    base = (np.uint64(1) << np.uint64(31)) + np.uint64(1 << 20)
    longer = base + np.arange(100, dtype=np.uint64) * 2               # evens; the last one is base + 198
    lists.append(longer)
    lists.append(np.sort(np.concatenate([base + np.uint64(198) + np.arange(1, 5, dtype=np.uint64) * 2 - np.uint64(1), [base + np.uint64(198)],
                                         base - np.arange(1, 4, dtype=np.uint64)])))  # shorter: meets `longer` at its last element only
    shorter = base + np.uint64(1 << 12) + np.arange(9, dtype=np.uint64) * 2 + np.uint64(1)  # odds; the last one is base + 4096 + 17
    lists.append(shorter)
    lists.append(np.sort(np.concatenate([base + np.uint64(1 << 12) + np.arange(70, dtype=np.uint64) * 2, [shorter[-1]]])))  # longer: meets `shorter` at its last only
    for s in lists:
        assert len(s) == len(np.unique(s)) and (len(s) < 2 or np.all(s[1:] > s[:-1]))
    assert len(set(lists[10].tolist()) & set(lists[11].tolist())) == 1 and lists[10][-1] in lists[11] and len(lists[11]) < len(lists[10])
    assert len(set(lists[12].tolist()) & set(lists[13].tolist())) == 1 and lists[12][-1] in lists[13] and len(lists[12]) < len(lists[13])
    return lists


def _widen(s):
    """a strictly increasing map of the 32-bit values onto hashes that use all 64 bits"""
    s = np.asarray(s, dtype=np.uint64)
    return (s << np.uint64(32)) | ((s * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF))


def _np_mix(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _np_bits(s, seed, word):
    """[len(s), 64]: bit r of every hash's mask word"""
    key = np.uint64(RS.mix((seed + word) & RS.M64))
    w = _np_mix(np.asarray(s, dtype=np.uint64) ^ key)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint32)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("word", [0, 1])
@pytest.mark.parametrize("width", [4, 8])
def test_jackknife_pairs_against_numpy(ctx, width, word, seed):
    from rabbittclust_amd import api
    assert api.JK_LDS_ELEMS == CAP
    lists = _count_lists() if width == 4 else [_widen(s) for s in _count_lists()]
    n = len(lists)
    assert int(_np_mix(np.array([12345 ^ RS.mix(7 + 1)], dtype=np.uint64))[0]) == RS.word(12345, 7, 1)  # the numpy mix is the definition's
    sk = _sketch_set(ctx, lists, width)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    common, size = ctx.jackknife_pairs(sk, pairs, seed=seed, word=word)
    bits = [_np_bits(s, seed, word) for s in lists]
    want_size = np.stack([b.sum(axis=0, dtype=np.uint32) for b in bits])
    assert size.shape == (n, 64) and np.array_equal(size, want_size)
    want = np.stack([bits[i][np.isin(lists[i], lists[j])].sum(axis=0, dtype=np.uint32) for i, j in pairs])
    bad = np.flatnonzero((common != want).any(axis=1))
    assert common.shape == (n * n, 64) and len(bad) == 0, [pairs[e] for e in bad[:8]]
    # what the cases are there for: something is counted, the identical lists count their sizes, the disjoint list nothing
    assert np.array_equal(common[5 * n + 7], want_size[5]) and np.array_equal(common[8 * n + 6], want_size[6])
    assert not common[9 * n:10 * n][np.arange(n) != 9].any() and want.sum() > 0
    assert common[10 * n + 11].sum() == bits[10][-1].sum() and common[13 * n + 12].sum() == bits[12][-1].sum()
    # without sizes, and no pairs at all
    c2, s2 = ctx.jackknife_pairs(sk, pairs[:3], seed=seed, word=word, sizes=False)
    assert s2 is None and np.array_equal(c2, want[:3])
    c0, _ = ctx.jackknife_pairs(sk, [], seed=seed, word=word)
    assert c0.shape == (0, 64)


# ---- rtc_nj_support ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_components(replicates=3, seed=0):
    sketches, comp = NS.component_set()
    return RS.clusters(sketches, comp, 21, replicates, seed)


@pytest.mark.parametrize("width", [4, 8])
def test_nj_support_components_against_the_restatement(ctx, switch, width):
    sketches, comp = NS.component_set()
    assert all(40 <= len(s) <= 200 for s in sketches)
    want, want_first, want_support = _want_components()
    assert sorted(np.diff(want_first).tolist()) == [0, 1, 1, 2, 3, 62, 63] and len(want_support) == len(want) == 132
    assert 0 < sum(want_support) < 3 * 126 and max(want_support) == 3  # some splits in every replicate, some not
    sk = _sketch_set(ctx, sketches, width)
    joins, first, support = ctx.nj_support(sk, comp, 21, 3)
    assert R.bits(_tuples(joins)) == R.bits(want) and first.tolist() == want_first
    assert support.tolist() == want_support
    # the main trees are rtc_nj_clusters', the counters name the paths
    c = ctx.nj_counters()
    assert (c["components"], c["wave_components"], c["workgroup_components"], c["grid_components"]) == (6, 5, 1, 0)
    assert c["records"] == 132 and c["paths"] == WAVE | WORKGROUP
    s = ctx.nj_support_counters()
    assert (s["replicates"], s["replicate_trees"], s["splits"], s["count_sum"]) == (3, 3 * 4, 1 + 2 + 61 + 62, sum(want_support))
    assert s["groups"] == 1 and s["total_ns"] >= s["count_ns"] + s["distance_ns"] + s["join_ns"] + s["split_ns"] > 0
    plain, plain_first = ctx.nj_clusters(sk, comp, 21)
    assert plain.tobytes() == joins.tobytes() and plain_first.tolist() == first.tolist()
    # another seed is another jackknife
    _, _, other = ctx.nj_support(sk, comp, 21, 3, seed=1)
    assert other.tolist() == _want_components(3, 1)[2] != want_support


@pytest.mark.parametrize("replicates", [1, 64, 65, 100])
def test_nj_support_a_component_of_six_across_the_words(ctx, switch, replicates):
    sketches = NS.six()
    want, want_first, want_support = RS.clusters(sketches, [0] * 6, 21, replicates, 9)
    sk = _sketch_set(ctx, sketches, 8)
    joins, first, support = ctx.nj_support(sk, np.zeros(6, dtype=np.int64), 21, replicates, seed=9)
    assert R.bits(_tuples(joins)) == R.bits(want) and first.tolist() == want_first == [0, 4]
    assert support.tolist() == want_support and support[-1] == 0 and max(want_support) <= replicates
    s = ctx.nj_support_counters()
    assert (s["replicates"], s["replicate_trees"], s["splits"]) == (replicates, replicates, 3)


def test_nj_support_invariance_and_limits(ctx, switch):
    from rabbittclust_amd import _lib
    sketches, comp = NS.component_set()
    want, want_first, want_support = _want_components()
    sk = _sketch_set(ctx, sketches, 4)

    def check():
        joins, first, support = ctx.nj_support(sk, comp, 21, 3)
        assert R.bits(_tuples(joins)) == R.bits(want) and first.tolist() == want_first and support.tolist() == want_support
    # the grid path for every tree of four or more, replicates included
    switch("RTC_NJ_GRID_MIN", 4)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 3))  # and several host threads for the distances and the splits
    check()
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 1))
    c = ctx.nj_counters()
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (2, 0, 4) and c["paths"] == WAVE | GRID
    switch("RTC_NJ_GRID_MIN", None)
    # the per-pair merge kernel in the fill
    switch("RTC_PAIR_FORCE_MERGE", 1)
    check()
    switch("RTC_PAIR_FORCE_MERGE", None)
    # room for the 65's block, one replicate block and one band: the 64 and the 65 each go alone with one replicate a group
    need = 2 * S.block_bytes(65) + S.band_bytes(65)
    switch("RTC_NJ_BYTES", need)
    check()
    assert ctx.nj_counters()["batches"] >= 2
    s = ctx.nj_support_counters()
    assert s["groups"] >= 6 and s["replicate_trees"] == 12
    switch("RTC_NJ_BYTES", need - 1)
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_support(sk, comp, 21, 3)
    assert e.value.status == _lib.RTC_ERR_NOMEM and "m = 65" in str(e.value) and str(need) in str(e.value)
    switch("RTC_NJ_BYTES", None)
    # the errors of rtc_nj_clusters, and the replicate cap
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_support(sk, comp, 21, 3, cap=len(want) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.nj_records_needed == len(want)
    for bad in (0, 257):
        with pytest.raises(_lib.RtcError) as e:
            ctx.nj_support(sk, comp, 21, bad)
        assert e.value.status == _lib.RTC_ERR_ARG
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_support(sk, comp, 0, 3)
    assert e.value.status == _lib.RTC_ERR_ARG
    # every sketch its own component: nothing to do
    j1, f1, s1 = ctx.nj_support(sk, np.arange(sk.n), 21, 3)
    assert len(j1) == 0 and len(s1) == 0 and f1.tolist() == [0] * (sk.n + 1)


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 1_000_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """11 genomes of 1 Mbp, listed in an order that scatters them: families of 5, 4 and 2 (copies of a base, 0.4 % mutated each)"""
    tmp = str(tmp_path_factory.mktemp("njs_fa"))
    rng = np.random.default_rng(29)
    seqs = []
    for size in (5, 4, 2):
        base = rng.integers(0, 4, size=L)
        seqs += [_mutate(rng, base, 0.004) for _ in range(size)]
    order = rng.permutation(len(seqs)).tolist()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths = []
    for g, o in enumerate(order):
        p = os.path.join(tmp, f"g{g:02d}.fna")
        with open(p, "wb") as f:
            f.write(f">s{g} genome {g}\n".encode() + acgt[seqs[o]].tobytes() + b"\n")
        paths.append(p)
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return {"list": lst, "paths": paths}


def _run(args, cwd, env=None):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _parse_clusters(path):
    clusters = []
    for ln in open(path):
        if ln.startswith("the cluster"):
            clusters.append([])
        elif ln.startswith("\t"):
            clusters[-1].append(int(ln.split("\t")[2]))
    return clusters


def _tsv_want(cluster, joins, support, replicates, m):
    """the table's lines of one tree: the records that name a split, with the leaves below their node"""
    if m < 4:
        return []
    below, out = {}, []
    for e, r in enumerate(joins):
        if int(r["c"]) != R.NONE:
            continue
        s = below.get(int(r["a"]), 1) + below.get(int(r["b"]), 1)
        below[int(r["a"])] = s
        out.append((cluster, e, s, int(support[e]), replicates))
    return out


def test_cli_writes_the_support(ctx, genomes, tmp_path):
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    args = ["--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", "0.05", "-t", "4", "--nj-tree", "--nj-all"]
    d1 = os.path.join(tmp, "plain"); os.makedirs(d1)
    d2 = os.path.join(tmp, "support"); os.makedirs(d2)
    out1, out2, mj = os.path.join(d1, "result.cluster"), os.path.join(d2, "result.cluster"), os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", out1], d1)
    err = _run([M] + args + ["-o", out2, "--nj-support", "10", "--nj-seed", "3"], d2, env={"RTC_METRICS_JSON": mj})
    for ext in ("", ".nj.newick", ".nj.all.newick"):
        assert open(out1 + ext, "rb").read() == open(out2 + ext, "rb").read(), ext  # as without the flag, byte for byte
    for ext in (".nj.support.newick", ".nj.all.support.newick", ".nj.support.tsv", ".nj.all.support.tsv"):
        assert not os.path.exists(out1 + ext) and os.path.exists(out2 + ext), ext
    assert re.search(r"jackknife support: \d+ trees, \d+ splits, 10 replicates, mean count [0-9.]+\n", err)
    clusters = _parse_clusters(out2)
    paths = genomes["paths"]
    n = len(paths)
    assert sorted(len(c) for c in clusters) == [2, 4, 5]
    # the labelled trees strip to the plain ones, and carry a label at every inner branch
    strip = lambda text: re.sub(r"\)\d+:", "):", text)
    labelled = open(out2 + ".nj.support.newick").read()
    assert strip(labelled) == open(out2 + ".nj.newick").read()
    assert [len(re.findall(r"\)\d+:", ln)) for ln in labelled.split("\n")[:-1]] == [max(len(c) - 3, 0) for c in clusters]
    labelled_all = open(out2 + ".nj.all.support.newick").read()
    assert strip(labelled_all) == open(out2 + ".nj.all.newick").read() and len(re.findall(r"\)\d+:", labelled_all)) == n - 3
    # the counts are the library's over the sketches the run saved
    folder = [os.path.join(d2, x) for x in os.listdir(d2) if os.path.isdir(os.path.join(d2, x))]
    assert len(folder) == 1
    raw = open(os.path.join(folder[0], "kssd.hash.sketch"), "rb").read()
    pos, sketches = 20, []
    for _ in range(n):
        (cnt,) = struct.unpack_from("<Q", raw, pos); pos += 8
        sketches.append(np.frombuffer(raw, dtype="<u4", count=cnt, offset=pos).copy()); pos += 4 * cnt
    assert pos == len(raw)
    m = json.load(open(mj))
    k = int(m["kmer_size"])
    sk = _sketch_set(ctx, sketches, 4)
    comp = np.zeros(n, dtype=np.int64)
    for q, c in enumerate(clusters):
        comp[c] = q
    joins, first, support = ctx.nj_support(sk, comp, k, 10, seed=3)
    rank = {q: r for r, q in enumerate(sorted(range(len(clusters)), key=lambda q: min(clusters[q])))}
    want = []
    for q, c in enumerate(clusters):
        a, b = int(first[rank[q]]), int(first[rank[q] + 1])
        want += _tsv_want(q, joins[a:b], support[a:b], 10, len(c))
    lines = open(out2 + ".nj.support.tsv").read().split("\n")
    assert lines[0] == "cluster\trecord\tleaves\tcount\treplicates" and lines[-1] == ""
    assert [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:-1]] == want and len(want) == 3
    # the printed labels are the counts in percent, in tree order
    from rabbittclust_amd import host
    for q, (c, ln) in enumerate(zip(clusters, labelled.split("\n"))):
        a, b = int(first[rank[q]]), int(first[rank[q] + 1])
        assert ln == host.nj_support_newick(paths, c, joins[a:b], support[a:b], 10)
    all_joins, _, all_support = ctx.nj_support(sk, np.zeros(n, dtype=np.int64), k, 10, seed=3)
    lines = open(out2 + ".nj.all.support.tsv").read().split("\n")
    assert [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:-1]] == _tsv_want(0, all_joins, all_support, 10, n)
    assert labelled_all == host.nj_support_newick(paths, range(n), all_joins, all_support, 10) + "\n"
    # the three families are apart in every replicate
    assert max(all_support.tolist()) == 10
    for key in ("nj_support_count_s", "nj_support_distance_s", "nj_support_join_s", "nj_support_split_s", "nj_support_replicates", "nj_support_mean"):
        assert key in m, key
    assert m["nj_support_replicates"] == 10 and 0 <= m["nj_support_mean"] <= 10
