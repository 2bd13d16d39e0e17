"""clust-mst --nj-tree / --nj-all on the GPU: rtc_nj_dev on additive and non-additive matrices through the wave, workgroup and grid
paths, rtc_nj_clusters over components of sketches in batches, and the command line end to end.  Every comparison is on bits:
the records of the restatement (tests/refnj.py), and for additive matrices the tree that generated them."""
import ctypes as C
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import linkage_sets as S
from tests import nj_sets as N
from tests import reflinkage as RL
from tests import refnj as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
WAVE, WORKGROUP, GRID = 1, 2, 4


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


def _path_of(m, grid_min):
    return GRID if m >= grid_min else WAVE if m <= 64 else WORKGROUP


def _check_counters(ctx, m, grid_min, n_records):
    from rabbittclust_amd import api
    c = ctx.nj_counters()
    path = _path_of(m, grid_min if grid_min else api.NJ_GRID_MIN)
    assert c["paths"] == path, (m, grid_min, c)
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (int(path == WAVE), int(path == WORKGROUP), int(path == GRID))
    assert c["components"] == 1 and c["records"] == n_records


@functools.lru_cache(maxsize=None)
def _want_additive(m):
    D, tree = N.additive(m)
    return R.nj(D)


# ---- rtc_nj_dev ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", N.ADDITIVE_SIZES)
def test_nj_dev_additive_matrices_on_every_path(ctx, switch, m):
    D, tree = N.additive(m)
    want = _want_additive(m)
    assert R.splits(want, m) == tree
    for grid_min in (None, 4):
        switch("RTC_NJ_GRID_MIN", grid_min)
        got = _tuples(ctx.nj(D))
        assert R.bits(got) == R.bits(want), (m, grid_min, got[:3], want[:3])
        assert R.splits(got, m) == tree
        _check_counters(ctx, m, grid_min, max(m - 2, 1))


@functools.lru_cache(maxsize=None)
def _want_case(name, m):
    return R.nj(N.case(name, m))


@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_nj_dev_non_additive_matrices_on_every_path(ctx, switch, name):
    for m in N.CASE_SIZES:
        D, want = N.case(name, m), _want_case(name, m)
        for grid_min in (None, 4):
            switch("RTC_NJ_GRID_MIN", grid_min)
            got = _tuples(ctx.nj(D))
            assert R.bits(got) == R.bits(want), (name, m, grid_min, got[:3], want[:3])
            _check_counters(ctx, m, grid_min, m - 2)


@pytest.mark.parametrize("m", [64, 65])
def test_nj_dev_padded_rows_diagonal_and_argument_errors(ctx, switch, m):
    from rabbittclust_amd import _lib
    D, want = N.case("random_ties", m), _want_case("random_ties", m)
    ld = m + 3
    padded = np.full((m, ld), np.nan)  # what lies beyond a row's m entries must never be read, nor the diagonal
    padded[:, :m] = D
    padded[np.arange(m), np.arange(m)] = 7.0
    for grid_min in (None, 4):
        switch("RTC_NJ_GRID_MIN", grid_min)
        assert R.bits(_tuples(ctx.nj(padded))) == R.bits(want), (m, grid_min)
    import torch
    d = torch.from_numpy(D.reshape(-1).copy()).to(ctx.device)
    out = np.zeros(m, dtype=np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("pad", "<u4"), ("la", "<f8"), ("lb", "<f8"), ("lc", "<f8")]))
    nj = C.c_uint32(77)
    ptr, outp = C.c_void_p(d.data_ptr()), out.ctypes.data_as(C.c_void_p)
    assert ctx.lib.rtc_nj_dev(ctx.h, m, ptr, m - 1, outp, C.byref(nj)) == _lib.RTC_ERR_ARG and nj.value == 0  # ld < m
    assert ctx.lib.rtc_nj_dev(ctx.h, 0x7fffffff, ptr, 0x7fffffff, outp, C.byref(nj)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_nj_dev(ctx.h, m, None, m, outp, C.byref(nj)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_nj_dev(ctx.h, m, ptr, m, None, C.byref(nj)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_nj_dev(ctx.h, m, ptr, m, outp, None) == _lib.RTC_ERR_ARG
    assert len(ctx.nj(np.zeros((1, 1)))) == 0 and len(ctx.nj(np.zeros((0, 0)))) == 0 and ctx.nj_counters()["components"] == 0


def test_nj_dev_takes_the_grid_path_by_itself(ctx, switch):
    """one point past the default RTC_NJ_GRID_MIN, no switch: checked against the generating tree alone"""
    from rabbittclust_amd import api
    m = api.NJ_GRID_MIN + 1
    D, tree = N.additive(m)
    got = _tuples(ctx.nj(D))
    assert R.splits(got, m) == tree
    c = ctx.nj_counters()
    assert c["paths"] == GRID and c["grid_components"] == 1 and c["records"] == m - 2


# ---- rtc_nj_clusters -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _component_case(kmer_size=21):
    """(sketches, comp, records with genome indices, first, pairs at distance 1): every component's restatement over distances
    formed here from brute-force intersections"""
    sketches, comp = S.component_set()
    groups = {}
    for g, lab in enumerate(comp):
        groups.setdefault(int(lab), []).append(g)
    records, first, ones = [], [0], 0
    for members in sorted(groups.values()):
        m = len(members)
        if m >= 2:
            keys = RL.keys_of([sketches[g] for g in members])
            D = np.zeros((m, m))
            for i in range(m):
                for j in range(i):
                    D[i, j] = D[j, i] = RL.distance(int(keys[i, j, 0]), int(keys[i, j, 1]), kmer_size)
                    ones += int(D[i, j] == 1.0)
            records += [(members[a], members[b], members[c] if c != R.NONE else c, la, lb, lc) for a, b, c, la, lb, lc in R.nj(D)]
        first.append(len(records))
    return sketches, comp, records, first, ones


def _sketch_set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=21, kind="kssd", width=width)


@pytest.mark.parametrize("width", [4, 8])
def test_nj_clusters_components_batches_and_limits(ctx, switch, width):
    from rabbittclust_amd import _lib
    sketches, comp, want, want_first, ones = _component_case()
    assert want_first == [0, 62, 190, 253, 256, 257, 257, 257] and len(want) == 257
    assert ones >= 4  # pairs without a common hash -- the empty sketch's at least -- are in it, at exactly 1
    sk = _sketch_set(ctx, sketches, width)
    got, first = ctx.nj_clusters(sk, comp, 21)
    assert R.bits(_tuples(got)) == R.bits(want) and first.tolist() == want_first
    c = ctx.nj_counters()
    assert (c["components"], c["wave_components"], c["workgroup_components"], c["grid_components"]) == (5, 3, 2, 0)  # 64, 5 and 2 in a wave
    assert c["records"] == 257 and c["batches"] == 1 and c["paths"] == WAVE | WORKGROUP
    # the grid path inside the call, and several host threads for the distances
    switch("RTC_NJ_GRID_MIN", 4)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 3))
    got_g, first_g = ctx.nj_clusters(sk, comp, 21)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 1))
    assert R.bits(_tuples(got_g)) == R.bits(want) and first_g.tolist() == want_first
    c = ctx.nj_counters()
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (1, 0, 4) and c["paths"] == WAVE | GRID
    switch("RTC_NJ_GRID_MIN", None)
    # the per-pair merge kernel instead of the tiled one in the fill
    switch("RTC_PAIR_FORCE_MERGE", 1)
    got_m, first_m = ctx.nj_clusters(sk, comp, 21)
    switch("RTC_PAIR_FORCE_MERGE", None)
    assert R.bits(_tuples(got_m)) == R.bits(want) and first_m.tolist() == want_first
    # the 130 alone needs its block and one band; with just that the components go in three batches: 64 | 130 | 65, 5, 2
    need = S.block_bytes(130) + S.band_bytes(130)
    switch("RTC_NJ_BYTES", need)
    got3, first3 = ctx.nj_clusters(sk, comp, 21)
    assert R.bits(_tuples(got3)) == R.bits(want) and first3.tolist() == want_first
    assert ctx.nj_counters()["batches"] >= 3
    switch("RTC_NJ_BYTES", need - 1)
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_clusters(sk, comp, 21)
    assert e.value.status == _lib.RTC_ERR_NOMEM and "m = 130" in str(e.value) and str(need) in str(e.value)
    switch("RTC_NJ_BYTES", None)
    # room for one record fewer than there are: the count comes back
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_clusters(sk, comp, 21, cap=len(want) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.nj_records_needed == len(want)
    # argument errors
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_clusters(sk, comp, 0)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = 3
    with pytest.raises(_lib.RtcError) as e:
        ctx.nj_clusters(sk, comp, 21)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = width
    # every sketch its own component: nothing to do
    got1, first1 = ctx.nj_clusters(sk, np.arange(sk.n), 21)
    assert len(got1) == 0 and first1.tolist() == [0] * (sk.n + 1) and ctx.nj_counters()["components"] == 0


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 1_000_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """12 genomes of 1 Mbp, listed in an order that scatters them: families of 4, 3 and 2 (copies of a base, 0.4 % mutated each)
    and three strangers"""
    tmp = str(tmp_path_factory.mktemp("nj_fa"))
    rng = np.random.default_rng(23)
    seqs = []
    for size in (4, 3, 2, 1, 1, 1):
        base = rng.integers(0, 4, size=L)
        seqs += [_mutate(rng, base, 0.004) for _ in range(size)] if size > 1 else [base]
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


def test_cli_writes_the_trees(ctx, genomes, tmp_path):
    from rabbittclust_amd import host
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    args = ["--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", "0.05", "-t", "4"]
    d1 = os.path.join(tmp, "plain"); os.makedirs(d1)
    d2 = os.path.join(tmp, "nj"); os.makedirs(d2)
    plain, out, mj = os.path.join(tmp, "plain.cluster"), os.path.join(tmp, "result.cluster"), os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", plain], d1)
    err = _run([M] + args + ["-o", out, "--nj-tree", "--nj-all"], d2, env={"RTC_METRICS_JSON": mj})
    assert open(out, "rb").read() == open(plain, "rb").read()  # the plain result, byte for byte
    assert not os.path.exists(plain + ".nj.newick") and not os.path.exists(plain + ".nj.all.newick")
    assert out + ".nj.newick\n" in err and out + ".nj.all.newick\n" in err
    clusters = _parse_clusters(out)
    paths = genomes["paths"]
    n = len(paths)
    assert sorted(len(c) for c in clusters) == [1, 1, 1, 2, 3, 4]
    lines = open(out + ".nj.newick").read().split("\n")
    assert lines[-1] == "" and len(lines) == len(clusters) + 1
    for c, ln in zip(clusters, lines):
        assert ln.endswith(";") and [g for g in range(n) if paths[g] in ln] == sorted(c)
        assert ln.count(":") == (2 * len(c) - 3 if len(c) >= 3 else 2 if len(c) == 2 else 0)
    # the same text from the library over the sketches the run saved
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
    joins, first = ctx.nj_clusters(sk, comp, k)
    rank = {q: r for r, q in enumerate(sorted(range(len(clusters)), key=lambda q: min(clusters[q])))}
    want = [host.nj_newick(paths, c, joins[int(first[rank[q]]):int(first[rank[q] + 1])]) for q, c in enumerate(clusters)]
    assert lines[:-1] == want
    all_joins, _ = ctx.nj_clusters(sk, np.zeros(n, dtype=np.int64), k)
    text = open(out + ".nj.all.newick").read()
    assert text == host.nj_newick(paths, range(n), all_joins) + "\n"
    assert all(p in text for p in paths) and text.count(":") == 2 * n - 3
    for key in ("nj_fill_s", "nj_distance_s", "nj_join_s", "nj_components", "nj_records"):
        assert key in m, key
    assert m["nj_components"] == sum(1 for c in clusters if len(c) >= 2) + 1
    assert m["nj_records"] == sum(max(len(c) - 2, 1) for c in clusters if len(c) >= 2) + n - 2
