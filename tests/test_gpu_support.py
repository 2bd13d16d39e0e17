"""clust-mst --cluster-support on the device: rtc_components64_dev against a per-lane union-find, rtc_cluster_support against the
restatement (tests/refsupport.py) over the sets of tests/support_sets.py, its invariance under the row chunks, the words held at
once and the pair routine's paths, and the command line end to end.  Every comparison is exact."""
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import refsupport as R
from tests import support_sets as SS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
KMER, THRESHOLD = SS.KMER, SS.THRESHOLD


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
    for name in ("RTC_EDGE_BUDGET", "RTC_SUPPORT_BYTES", "RTC_PAIR_FORCE_MERGE"):
        set_switch(name, None)
    yield set_switch
    for name in names:
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


def _widen(s):
    """a strictly increasing map of the 32-bit values onto hashes that use all 64 bits"""
    s = np.asarray(s, dtype=np.uint64)
    return (s << np.uint64(32)) | ((s * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF))


def _sketch_set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=KMER, kind="kssd", width=width)


def _tuples(rec):
    return [tuple(int(x) for x in r) for r in rec.tolist()]


# ---- rtc_components64_dev ------------------------------------------------------------------------------------------------------
def _lane_union_find(n, edges, masks):
    """[n, 64]: the smallest vertex of every component, lane after lane"""
    out = np.zeros((n, 64), dtype=np.uint32)
    for r in range(64):
        parent = list(range(n))
        for (u, v), mk in zip(edges, masks):
            if (int(mk) >> r) & 1:
                R._union(parent, int(u), int(v))
        out[:, r] = [R._find(parent, g) for g in range(n)]
    return out


def test_components64_of_nothing(ctx):
    got = ctx.components64(1, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.uint64))
    assert got.shape == (1, 64) and not got.any()
    got = ctx.components64(5, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.uint64))
    assert np.array_equal(got, np.repeat(np.arange(5, dtype=np.uint32), 64).reshape(5, 64))


def test_components64_on_a_zigzag_path(ctx):
    """a path of 300 whose vertex numbers zigzag: lane 0 holds every edge, lane 1 none, lane 2 the even edges, lane 63 a star"""
    n = 300
    at = SS.zigzag(n)
    assert at[:4] == [0, 299, 1, 298]
    edges = [(at[p], at[p + 1]) for p in range(n - 1)]
    masks = [1 | (4 if p % 2 == 0 else 0) for p in range(n - 1)]
    edges += [(150, v) for v in range(n) if v != 150]
    masks += [1 << 63] * (n - 1)
    want = _lane_union_find(n, edges, masks)
    assert not want[:, 0].any() and not want[:, 63].any() and np.array_equal(want[:, 1], np.arange(n)) and len(np.unique(want[:, 2])) == 150
    got = ctx.components64(n, edges, masks)
    assert np.array_equal(got, want)
    # a second call on converged labels changes nothing
    assert np.array_equal(ctx.components64(n, edges, masks, labels=got), want)
    # chunks of edges, one after another and in the other order
    half = len(edges) // 2
    first = ctx.components64(n, edges[half:], masks[half:])
    assert np.array_equal(ctx.components64(n, edges[:half], masks[:half], labels=first), want)


def test_components64_on_random_graphs(ctx):
    rng = np.random.default_rng(17)
    n, m = 500, 1500
    edges = rng.integers(0, n, size=(m, 2))
    edges[100:160] = edges[:60]             # duplicates
    edges[200:230] = edges[:30][:, ::-1]    # and in the other orientation
    edges[300] = (7, 7)                     # a loop
    masks = rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
    masks[::9] &= rng.integers(0, 1 << 64, size=len(masks[::9]), dtype=np.uint64)
    want = _lane_union_find(n, edges, masks)
    got = ctx.components64(n, edges, masks)
    assert np.array_equal(got, want)
    assert np.array_equal(ctx.components64(n, edges, masks, labels=got), want)
    thirds = [slice(0, 500), slice(500, 1000), slice(1000, 1500)]
    lab = None
    for t in thirds:
        lab = ctx.components64(n, edges[t], masks[t], labels=lab)
    assert np.array_equal(lab, want)


# ---- rtc_cluster_support against the restatement -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _constructed(width, seed):
    """(sketches, labels, the 256 outcomes of the restatement, members) -- at width 8 over the widened hashes"""
    sk, _ = SS.constructed()
    sk = [_widen(s) for s in sk] if width == 8 else sk
    lab = R.mst_partition(sk, KMER, THRESHOLD)
    outs, members = R.outcomes(sk, lab, KMER, THRESHOLD, 256, seed)
    return sk, lab, outs, members


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("B", [1, 64, 65, 100, 256])
@pytest.mark.parametrize("width", [4, 8])
def test_cluster_support_on_the_constructed_set(ctx, switch, width, B, seed):
    sk, lab, outs, members = _constructed(width, seed)
    want, want_together = R.tally(outs, members, B)
    assert all(sum(r[1:5]) == B for r in want)
    if B >= 100:  # what the set is there for
        assert any(r[2] > 0 and r[3] > 0 and r[4] > 0 for r in want) and any(0 < r[1] < B for r in want)
        seven = [m for m in members if len(m) == 7][0]
        assert len({want_together[g] for g in seven}) > 1
    got, together = ctx.cluster_support(_sketch_set(ctx, sk, width), lab, KMER, THRESHOLD, B, seed=seed)
    assert _tuples(got) == want
    assert together.tolist() == want_together
    c = ctx.cluster_support_counters()
    assert c["chunks"] == 1 and c["candidates"] == len(R.candidates(sk, THRESHOLD, KMER)) and c["hook_passes"] >= 2
    assert c["total_ns"] >= c["pair_ns"] + c["count_ns"] + c["components_ns"] + c["tally_ns"] > 0


@pytest.mark.parametrize("shift", [110, 116])
def test_cluster_support_on_the_zigzag_chain(ctx, switch, shift):
    """one cluster that is a path whose genome numbers zigzag: a hooking loop that stops early leaves it in pieces"""
    B = 64
    sk = SS.chain(shift)
    lab = [0] * len(sk)
    want, want_together = R.support(sk, lab, KMER, THRESHOLD, B, 1)
    assert len(want) == 1
    if shift == 110:
        assert 0 < want[0][1] < B
    else:
        assert want[0][5] >= 3
    got, together = ctx.cluster_support(_sketch_set(ctx, sk, 4), lab, KMER, THRESHOLD, B, seed=1)
    assert _tuples(got) == want and together.tolist() == want_together


@pytest.mark.parametrize("labelling", ["one", "own"])
def test_cluster_support_under_other_labellings(ctx, switch, labelling):
    sk, _ = SS.constructed()
    lab = [0] * len(sk) if labelling == "one" else list(range(len(sk)))[::-1]
    want, want_together = R.support(sk, lab, KMER, THRESHOLD, 65, 2)
    got, together = ctx.cluster_support(_sketch_set(ctx, sk, 4), lab, KMER, THRESHOLD, 65, seed=2)
    assert _tuples(got) == want and together.tolist() == want_together
    if labelling == "one":
        assert len(want) == 1 and want[0][3] == want[0][4] == 0 and want[0][5] >= 8
    else:
        assert len(want) == len(sk) and any(r[3] > 0 for r in want) and not any(want_together)


@functools.lru_cache(maxsize=None)
def _paths_want(B=70, seed=5):
    sk, comp = SS.paths()
    return R.support(sk, comp, KMER, THRESHOLD, B, seed)


def test_cluster_support_paths_and_invariance(ctx, switch):
    from rabbittclust_amd import api
    sk, comp = SS.paths()
    long = [len(s) for s, c in zip(sk, comp) if c == 4]
    assert len(long) == 3 and min(long) > api.JK_LDS_ELEMS  # the pair routine searches these where they lie
    want, want_together = _paths_want()
    assert sorted(r[0] for r in want) == [1, 2, 3, 64, 65]
    assert any(0 < r[1] < 70 and r[5] >= 2 for r in want if r[0] >= 64)
    ss = _sketch_set(ctx, sk, 8)

    def check():
        got, together = ctx.cluster_support(ss, comp, KMER, THRESHOLD, 70, seed=5)
        assert _tuples(got) == want and together.tolist() == want_together
        return ctx.cluster_support_counters()
    plain = check()
    assert plain["chunks"] == 1
    switch("RTC_PAIR_FORCE_MERGE", 1)
    assert check()["candidates"] == plain["candidates"]
    switch("RTC_PAIR_FORCE_MERGE", None)
    # one word of 64 replicates at a time: the pair phase runs once per word
    switch("RTC_SUPPORT_BYTES", 1)
    one = check()
    assert one["chunks"] == 2 and (one["inner_kept"], one["crossing_kept"]) == (plain["inner_kept"], plain["crossing_kept"])
    switch("RTC_SUPPORT_BYTES", None)


def test_cluster_support_in_row_chunks(ctx, switch):
    """every sketch holds hash 1: under RTC_EDGE_BUDGET=1 (raised to 64 n + 1 024) the triangle of candidates comes in several
    row chunks"""
    sk, comp = SS.dense()
    n = len(sk)
    want, want_together = R.support(sk, comp, KMER, THRESHOLD, 3, 7)
    assert n * (n - 1) // 2 > 2 * (64 * n + 1024) and any(r[3] + r[4] > 0 for r in want)
    ss = _sketch_set(ctx, sk, 4)
    got, together = ctx.cluster_support(ss, comp, KMER, THRESHOLD, 3, seed=7)
    assert _tuples(got) == want and together.tolist() == want_together
    assert ctx.cluster_support_counters()["chunks"] == 1
    whole70 = ctx.cluster_support(ss, comp, KMER, THRESHOLD, 70, seed=7)
    switch("RTC_EDGE_BUDGET", 1)
    got, together = ctx.cluster_support(ss, comp, KMER, THRESHOLD, 3, seed=7)
    c = ctx.cluster_support_counters()
    assert _tuples(got) == want and together.tolist() == want_together
    assert c["chunks"] > 2 and c["candidates"] == len(R.candidates(sk, THRESHOLD, KMER))
    cut70 = ctx.cluster_support(ss, comp, KMER, THRESHOLD, 70, seed=7)
    assert cut70[0].tobytes() == whole70[0].tobytes() and cut70[1].tobytes() == whole70[1].tobytes()
    switch("RTC_EDGE_BUDGET", None)


def test_cluster_support_errors(ctx, switch):
    from rabbittclust_amd import _lib
    sk, _ = SS.constructed()
    lab = R.mst_partition(sk, KMER, THRESHOLD)
    ss = _sketch_set(ctx, sk, 4)
    for args, status in (((KMER, THRESHOLD, 0), _lib.RTC_ERR_ARG), ((KMER, THRESHOLD, 257), _lib.RTC_ERR_ARG),
                         ((KMER, float("nan"), 10), _lib.RTC_ERR_ARG), ((KMER, -0.01, 10), _lib.RTC_ERR_ARG), ((0, THRESHOLD, 10), _lib.RTC_ERR_ARG),
                         ((KMER, 1.0, 10), _lib.RTC_ERR_UNSUPPORTED)):
        with pytest.raises(_lib.RtcError) as e:
            ctx.cluster_support(ss, lab, *args)
        assert e.value.status == status, args
    ss.width = 3
    with pytest.raises(_lib.RtcError) as e:
        ctx.cluster_support(ss, lab, KMER, THRESHOLD, 10)
    assert e.value.status == _lib.RTC_ERR_ARG
    ss.width = 4
    # and the call is whole after them
    want, want_together = R.support(sk, lab, KMER, THRESHOLD, 2, 0)
    got, together = ctx.cluster_support(ss, lab, KMER, THRESHOLD, 2)
    assert _tuples(got) == want and together.tolist() == want_together


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 500_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """11 genomes of 0.5 Mbp, listed in an order that scatters them: families of 5, 4 and 2, copies of a base mutated at 0.4 %,
    1.5 % and 0.4 % -- the middle family sits near the threshold"""
    tmp = str(tmp_path_factory.mktemp("csup_fa"))
    rng = np.random.default_rng(31)
    seqs = []
    for size, rate in ((5, 0.004), (4, 0.015), (2, 0.004)):
        base = rng.integers(0, 4, size=L)
        seqs += [_mutate(rng, base, rate) for _ in range(size)]
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


def test_cli_writes_the_support(ctx, genomes, tmp_path):
    from rabbittclust_amd import api, host
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    args = ["--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", "0.05", "-t", "4"]
    dirs = {}
    for name in ("plain", "support", "beside"):
        dirs[name] = os.path.join(tmp, name)
        os.makedirs(dirs[name])
    out1, out2, out3 = (os.path.join(dirs[name], "result.cluster") for name in ("plain", "support", "beside"))
    mj = os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", out1], dirs["plain"])
    err = _run([M] + args + ["-o", out2, "--cluster-support", "20", "--support-seed", "3"], dirs["support"], env={"RTC_METRICS_JSON": mj})
    _run([M] + args + ["-o", out3, "--cluster-support", "20", "--support-seed", "3", "--quality", "--nj-tree"], dirs["beside"])
    assert open(out1, "rb").read() == open(out2, "rb").read() == open(out3, "rb").read()  # as without the flag, byte for byte
    for ext in (".support.tsv", ".support.genomes.tsv"):
        assert not os.path.exists(out1 + ext) and os.path.exists(out2 + ext), ext
        assert open(out2 + ext, "rb").read() == open(out3 + ext, "rb").read(), ext
    assert os.path.exists(out3 + ".quality.tsv") and os.path.exists(out3 + ".nj.newick")
    assert "cluster support: " in err and " 20 replicates, " in err
    clusters = _parse_clusters(out2)
    paths = genomes["paths"]
    n = len(paths)
    assert sorted(g for c in clusters for g in c) == list(range(n))
    # the restatement over the sketches the run saved
    folder = [os.path.join(dirs["support"], x) for x in os.listdir(dirs["support"]) if os.path.isdir(os.path.join(dirs["support"], x))]
    assert len(folder) == 1
    raw = open(os.path.join(folder[0], "kssd.hash.sketch"), "rb").read()
    pos, sketches = 20, []
    for _ in range(n):
        (cnt,) = struct.unpack_from("<Q", raw, pos); pos += 8
        sketches.append(np.frombuffer(raw, dtype="<u4", count=cnt, offset=pos).copy()); pos += 4 * cnt
    assert pos == len(raw)
    m = json.load(open(mj))
    k = int(m["kmer_size"])
    cluster_of = np.zeros(n, dtype=np.int64)
    for q, c in enumerate(clusters):
        cluster_of[c] = q
    want, want_together = R.support(sketches, cluster_of.tolist(), k, 0.05, 20, 3)
    rec = np.array(want, dtype=api.CSUPPORT_DT)
    s_text, g_text = host.support_report(paths, cluster_of, rec, want_together, 20)
    assert open(out2 + ".support.tsv").read() == s_text
    assert open(out2 + ".support.genomes.tsv").read() == g_text
    assert s_text.count("\n") == 1 + len(clusters) and g_text.count("\n") == 1 + n
    # and the library agrees with both
    got, together = ctx.cluster_support(_sketch_set(ctx, sketches, 4), cluster_of, k, 0.05, 20, seed=3)
    assert _tuples(got) == want and together.tolist() == want_together
    for key in ("support_pair_s", "support_count_s", "support_components_s", "support_tally_s", "support_replicates", "support_recovered_mean"):
        assert key in m, key
    assert m["support_replicates"] == 20 and 0 <= m["support_recovered_mean"] <= 20
