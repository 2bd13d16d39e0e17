"""clust-mst --upgma on the GPU: rtc_upgma_dev record for record against the restatement (tests/refupgma.py) on every matrix of
tests/upgma_sets.py through the wave, workgroup and grid paths, rtc_upgma_clusters over components of sketches in batches, and
the command line end to end against the restatement's writers."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import linkage_sets as S
from tests import reflinkage as RL
from tests import refupgma as R
from tests import upgma_sets as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
WAVE, WORKGROUP, GRID = 1, 2, 4
# RTC_UPGMA_GRID_MIN: the default, everything from 4 on the grid path, 65 still on the workgroup path and 66 on the grid path, and
# nothing on the grid path (257 and 300 in one workgroup)
GRID_MINS = (None, 4, 66, 100000)


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
    for name in ("RTC_UPGMA_GRID_MIN", "RTC_UPGMA_BYTES", "RTC_PAIR_FORCE_MERGE"):
        set_switch(name, None)
    yield set_switch
    for name in names:
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


@functools.lru_cache(maxsize=None)
def _sets():
    return {name: (Sm, w) for name, Sm, w in U.dev_sets()}


@functools.lru_cache(maxsize=None)
def _want(name):
    Sm, w = _sets()[name]
    return R.rowcache(Sm, w)[0]  # test_cpu_upgma.py holds it to the naive scan on every set


SET_NAMES = [name for name, _, _ in U.dev_sets()]


def _path_of(m, grid_min):
    from rabbittclust_amd import api
    gm = api.UPGMA_GRID_MIN if grid_min is None else max(grid_min, 4)
    return GRID if m >= gm else WAVE if m <= 64 else WORKGROUP


def _check_counters(ctx, m, grid_min):
    c = ctx.upgma_counters()
    path = _path_of(m, grid_min)
    assert c["paths"] == path == ctx.upgma_last_path(), (m, grid_min, c)
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (int(path == WAVE), int(path == WORKGROUP), int(path == GRID))
    assert c["components"] == 1 and c["merges"] == m - 1 and c["row_rescans"] == 0
    return path


# ---- rtc_upgma_dev -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SET_NAMES)
def test_upgma_dev_records_on_every_path(ctx, switch, name):
    Sm, w = _sets()[name]
    m = len(Sm)
    want = _want(name)
    arr = np.array(Sm, dtype=np.uint64)
    seen = 0
    for grid_min in GRID_MINS:
        switch("RTC_UPGMA_GRID_MIN", grid_min)
        got = R.as_tuples(ctx.upgma(arr, w))
        assert got == want, (name, grid_min, [x for x in zip(got, want) if x[0] != x[1]][:3])
        seen |= _check_counters(ctx, m, grid_min)
    assert seen == (WAVE if m < 4 else WAVE | GRID if m <= 64 else WORKGROUP | GRID), (name, seen)


@pytest.mark.parametrize("m", [64, 65])
def test_upgma_dev_padded_rows_diagonal_and_argument_errors(ctx, switch, m):
    from rabbittclust_amd import _lib
    name = "random_ties_%d" % m
    Sm, _ = _sets()[name]
    ld = m + 3
    padded = np.full((m, ld), (1 << 64) - 1, dtype=np.uint64)  # what lies beyond a row's m entries must never be read, nor the diagonal
    padded[:, :m] = np.array(Sm, dtype=np.uint64)
    padded[np.arange(m), np.arange(m)] = (1 << 63) + 7
    for grid_min in (None, 4):
        switch("RTC_UPGMA_GRID_MIN", grid_min)
        assert R.as_tuples(ctx.upgma(padded)) == _want(name), (m, grid_min)
    ones = np.ones(m, dtype=np.uint32)
    arr = np.array(Sm, dtype=np.uint64)
    for bad_sizes in (np.where(np.arange(m) == m // 2, 0, ones), np.full(m, ((1 << 22) + m - 1) // m, dtype=np.uint32)):
        with pytest.raises(_lib.RtcError) as e:  # a size of 0; the sizes sum to 2^22 or more
            ctx.upgma(arr, bad_sizes)
        assert e.value.status == _lib.RTC_ERR_ARG
    just = np.ones(m, dtype=np.uint32)
    just[0] = (1 << 22) - m  # W = 2^22 - 1: the largest that is taken
    assert len(ctx.upgma(arr, just)) == m - 1
    with pytest.raises(_lib.RtcError) as e:
        ctx.upgma(arr, ld=m - 1)
    assert e.value.status == _lib.RTC_ERR_ARG
    import torch
    d = torch.from_numpy(arr.view(np.int64).reshape(-1).copy()).to(ctx.device)
    out = np.zeros(m, dtype=[("a", "<u4"), ("b", "<u4"), ("sa", "<u4"), ("sb", "<u4"), ("s", "<u8")])
    ptr, outp = C.c_void_p(d.data_ptr()), out.ctypes.data_as(C.c_void_p)
    assert ctx.lib.rtc_upgma_dev(ctx.h, m, None, m, None, outp) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_upgma_dev(ctx.h, m, ptr, m, None, None) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_upgma_dev(None, m, ptr, m, None, outp) == _lib.RTC_ERR_ARG
    assert len(ctx.upgma(np.zeros((1, 1), dtype=np.uint64))) == 0 and ctx.upgma_counters()["components"] == 0
    assert len(ctx.upgma(np.zeros((0, 0), dtype=np.uint64))) == 0


# ---- rtc_upgma_clusters --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _component_case(kmer_size=21):
    sketches, comp = S.component_set()
    merges, first = R.clusters(sketches, comp, kmer_size)
    return sketches, comp, merges, first


def _sketch_set(ctx, sketches, width, kind):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=21, kind=kind, width=width)


@pytest.mark.parametrize("width,kind", [(4, "kssd"), (8, "minhash")])
def test_upgma_clusters_components_batches_and_limits(ctx, switch, width, kind):
    from rabbittclust_amd import _lib
    sketches, comp, want, want_first = _component_case()
    assert want_first == [0, 63, 192, 256, 260, 261, 261, 261] and len(want) == 261  # 64, 130, 65, 5, 2, 1, 1 members
    assert any(s == R.Q1 * na * nb for _, _, na, nb, s in want)  # the empty sketch is at exactly 1 from everything
    sk = _sketch_set(ctx, sketches, width, kind)
    got, first = ctx.upgma_clusters(sk, comp, 21)
    assert R.as_tuples(got) == want and first.tolist() == want_first
    c = ctx.upgma_counters()
    # one component on each path in one call: 64, 5 and 2 in a wave, 65 in a workgroup, 130 on the grid
    assert (c["components"], c["wave_components"], c["workgroup_components"], c["grid_components"]) == (5, 3, 1, 1)
    assert c["merges"] == 261 and c["row_rescans"] == 0 and c["paths"] == WAVE | WORKGROUP | GRID
    assert c["fill_ns"] > 0 and c["distance_ns"] > 0 and c["agglomerate_ns"] > 0 and c["total_ns"] >= c["agglomerate_ns"]
    # 130 in a workgroup too; and several host threads for the distances
    switch("RTC_UPGMA_GRID_MIN", 131)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 3))
    got_g, first_g = ctx.upgma_clusters(sk, comp, 21)
    ctx.check(ctx.lib.rtc_ctx_set_host_threads(ctx.h, 1))
    assert R.as_tuples(got_g) == want and first_g.tolist() == want_first
    c = ctx.upgma_counters()
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (3, 2, 0) and c["paths"] == WAVE | WORKGROUP
    switch("RTC_UPGMA_GRID_MIN", 4)
    got_4, first_4 = ctx.upgma_clusters(sk, comp, 21)
    assert R.as_tuples(got_4) == want and first_4.tolist() == want_first
    c = ctx.upgma_counters()
    assert (c["wave_components"], c["workgroup_components"], c["grid_components"]) == (1, 0, 4) and c["paths"] == WAVE | GRID
    switch("RTC_UPGMA_GRID_MIN", None)
    # the 130 alone needs its block and one band; with just that the components go in several batches, the records the same
    need = S.block_bytes(130) + S.band_bytes(130)
    switch("RTC_UPGMA_BYTES", need)
    got3, first3 = ctx.upgma_clusters(sk, comp, 21)
    assert R.as_tuples(got3) == want and first3.tolist() == want_first
    switch("RTC_UPGMA_BYTES", need - 1)
    with pytest.raises(_lib.RtcError) as e:
        ctx.upgma_clusters(sk, comp, 21)
    assert e.value.status == _lib.RTC_ERR_NOMEM and "rtc_upgma_clusters" in str(e.value) and "m = 130" in str(e.value) and str(need) in str(e.value)
    switch("RTC_UPGMA_BYTES", None)
    # room for one record fewer than there are: the count comes back
    with pytest.raises(_lib.RtcError) as e:
        ctx.upgma_clusters(sk, comp, 21, cap=len(want) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.upgma_merges_needed == len(want)
    # argument errors
    with pytest.raises(_lib.RtcError) as e:
        ctx.upgma_clusters(sk, comp, 0)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = 3
    with pytest.raises(_lib.RtcError) as e:
        ctx.upgma_clusters(sk, comp, 21)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = width
    # every sketch its own component: nothing to do
    got1, first1 = ctx.upgma_clusters(sk, np.arange(sk.n), 21)
    assert len(got1) == 0 and first1.tolist() == [0] * (sk.n + 1) and ctx.upgma_counters()["components"] == 0


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 1_000_000
THRESHOLD = 0.03


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """13 genomes of 1 Mbp: two chains of four (each a mutated copy of the one before it, 1.8 % a step: neighbours are within
    0.03, the ends are not, so single linkage joins a chain and average linkage cuts it), a tight family of three and two
    strangers, listed in an order that scatters them"""
    tmp = str(tmp_path_factory.mktemp("upgma_fa"))
    rng = np.random.default_rng(31)
    seqs, names = [], []
    for c in range(2):
        s = rng.integers(0, 4, size=L)
        for i in range(4):
            seqs.append(s); names.append((f"c{c}_{i}", f"chain {c}"))
            s = _mutate(rng, s, 0.018)
    base = rng.integers(0, 4, size=L)
    for i in range(3):
        seqs.append(_mutate(rng, base, 0.004)); names.append((f"f_{i}", "family"))
    for x in range(2):
        seqs.append(rng.integers(0, 4, size=L)); names.append((f"x{x}", "stranger"))
    order = rng.permutation(len(seqs)).tolist()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths, meta, ascii_seqs = [], [], []
    for g, o in enumerate(order):
        p = os.path.join(tmp, f"g{g:02d}.fna")
        body = acgt[seqs[o]]
        with open(p, "wb") as f:
            f.write(f">{names[o][0]} {names[o][1]}\n".encode() + body.tobytes() + b"\n")
        paths.append(p); ascii_seqs.append(body); meta.append((p, L, names[o][0], names[o][1]))
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    fa = os.path.join(tmp, "all.fna")
    with open(fa, "wb") as f:
        for g in range(len(paths)):
            f.write(open(paths[g], "rb").read())
    return {"tmp": tmp, "list": lst, "fasta": fa, "meta": meta, "seqs": ascii_seqs}


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


def _oracle_sketches(oracle, seqs, fast, k):
    if fast:
        return [oracle.kssd_sketch(s, k, 3) for s in seqs]
    off = np.arange(len(seqs) + 1, dtype=np.uint64) * L
    return oracle.sketch_minhash_batch(np.concatenate(seqs), off, k, 1000)


def _check_outputs(oracle, genomes, out, metrics, fast, meta, by_file):
    m = json.load(open(metrics))
    k = int(m["kmer_size"])  # what the distances are formed with (a --fast folder reports half_k * 2)
    sk = _oracle_sketches(oracle, genomes["seqs"], fast, 17 if fast else k)
    n = len(sk)
    single = _parse_clusters(out)
    comp = [0] * n
    for q, c in enumerate(single):
        for g in c:
            comp[g] = q
    merges, first = R.clusters(sk, comp, k)
    label = lambda g: meta[g][0]  # the file, or the sequence's name: meta's first field either way
    want_cl, want_lk, want_nw = R.report(single, merges, first, THRESHOLD, n, label)
    assert open(out + ".upgma").read() == RL.cluster_text(want_cl, meta, by_file, THRESHOLD)
    assert open(out + ".upgma.linkage.txt").read() == want_lk
    assert open(out + ".upgma.newick").read() == want_nw
    assert want_lk.count("\n") == n - len(single)  # every merge, nothing cut off
    for key in ("upgma_fill_s", "upgma_distance_s", "upgma_agglomerate_s", "upgma_components", "upgma_merges", "upgma_clusters"):
        assert key in m, key
    assert m["upgma_clusters"] == len(want_cl) and m["upgma_merges"] == n - len(single)
    assert m["upgma_components"] == sum(1 for c in single if len(c) >= 2)
    return single, want_cl


def test_cli_fast_list_and_beside_the_other_refinements(oracle, genomes, tmp_path):
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    args = ["--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", str(THRESHOLD), "-t", "4", "-e"]
    others = ["--linkage", "complete", "--nj-tree", "--quality"]
    plain, out, mj = os.path.join(tmp, "plain.cluster"), os.path.join(tmp, "result.cluster"), os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", plain] + others, tmp)
    err = _run([M] + args + ["-o", out, "--upgma"] + others, tmp, env={"RTC_METRICS_JSON": mj})
    assert open(out, "rb").read() == open(plain, "rb").read()  # the plain result, byte for byte
    for ext in (".complete", ".complete.linkage.txt", ".nj.newick", ".quality.tsv", ".silhouette.tsv"):
        assert open(out + ext, "rb").read() == open(plain + ext, "rb").read(), ext  # what the other flags write, unchanged
    for ext in (".upgma", ".upgma.linkage.txt", ".upgma.newick"):
        assert not os.path.exists(plain + ext)
    assert "-----write the average-linkage cluster result into: " + out + ".upgma\n" in err
    single, refined = _check_outputs(oracle, genomes, out, mj, True, genomes["meta"], True)
    # single linkage joins each chain; its ends are further apart than the threshold
    name = {g: mt[2] for g, mt in enumerate(genomes["meta"])}
    for c in range(2):
        chain = sorted(g for g in name if name[g].startswith(f"c{c}_"))
        assert sorted(next(cl for cl in single if chain[0] in cl)) == chain
    assert len(refined) >= len(single)


def test_cli_presketched_and_single_fasta(oracle, genomes, tmp_path):
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    # --fast from a saved folder, with the tree flags and the post-processing beside it
    d1 = os.path.join(tmp, "a"); os.makedirs(d1)
    _run([M, "--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", str(THRESHOLD), "-t", "4", "-o", os.path.join(d1, "a.cluster")], d1)
    folder = [os.path.join(d1, x) for x in os.listdir(d1) if os.path.isdir(os.path.join(d1, x))]
    assert len(folder) == 1
    out, mj = os.path.join(tmp, "p.cluster"), os.path.join(tmp, "p.json")
    _run([M, "--fast", "--presketched", folder[0], "-l", "-d", str(THRESHOLD), "-o", out, "--upgma", "--linkage-matrix", "--dedup-dist", "0.01"],
         tmp, env={"RTC_METRICS_JSON": mj})
    assert open(out, "rb").read() == open(os.path.join(d1, "a.cluster"), "rb").read()
    assert os.path.exists(out + ".linkage.txt") and os.path.exists(out + ".dedup")  # what the other flags write is still written
    _check_outputs(oracle, genomes, out, mj, True, genomes["meta"], True)
    # MinHash from one FASTA: sequences instead of files
    d2 = os.path.join(tmp, "s"); os.makedirs(d2)
    out2, mj2, plain2 = os.path.join(tmp, "s.cluster"), os.path.join(tmp, "s.json"), os.path.join(tmp, "s.plain")
    margs = [M, "-i", genomes["fasta"], "-k", "21", "-s", "1000", "-d", str(THRESHOLD), "-t", "4", "-e"]
    _run(margs + ["-o", plain2], d2)
    _run(margs + ["-o", out2, "--upgma"], d2, env={"RTC_METRICS_JSON": mj2})
    assert open(out2, "rb").read() == open(plain2, "rb").read()
    seq_meta = [(mt[2], L, mt[3]) for mt in genomes["meta"]]
    _check_outputs(oracle, genomes, out2, mj2, False, seq_meta, False)
