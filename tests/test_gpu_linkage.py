"""clust-mst --linkage complete on the GPU: rtc_linkage_dev on synthetic key matrices through both kernel paths, rtc_linkage_complete
over components of sketches in batches, and the command line end to end -- merge lists record for record against the
restatement (tests/reflinkage.py)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import linkage_sets as S
from tests import reflinkage as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")


def _tuples(merges):
    return [tuple(int(v) for v in r) for r in merges.tolist()]


# ---- rtc_linkage_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(S.CASES))
def test_linkage_dev_matches_the_restatement(ctx, case):
    for m in S.SIZES:
        keys = S.CASES[case](m)
        for kmin in ((0, 1), S.median_bound(keys)):  # no bound, and one that ends the run mid-way
            want, rescans = R.rowbest(keys, kmin)
            got = _tuples(ctx.linkage(keys, kmin))
            assert got == want, (case, m, kmin, got[:4], want[:4])
            c = ctx.linkage_counters()
            if m < 2:
                assert c["components"] == 0 and got == []
                continue
            assert c["merges"] == len(want) and c["rescans"] == rescans, (case, m, kmin)
            assert (c["wave_components"], c["workgroup_components"]) == ((1, 0) if m <= 64 else (0, 1))
            assert c["components"] == 1 and c["largest_m"] == m
            if kmin == (0, 1):
                if case == "zeros":
                    assert got == []
                if case == "star":  # every live row looks again at every step
                    assert rescans == (m - 1) * m // 2
                if case in ("all_equal", "star"):
                    assert [(a, b) for a, b, *_ in got] == [(0, j) for j in range(1, m)]
                if case == "equal_kappa":
                    assert [(cm, d) for _, _, cm, d, _ in got] == [(2, 4)] + [(1, 2)] * (m - 2)
                if case in ("tie_free", "near_2_31", "chain"):
                    assert len(got) == m - 1 and got[-1][4] == m
            elif case in ("tie_free", "near_2_31") and m >= 3:
                assert 0 < len(got) < m - 1


def _dev(ctx, keys, m, ld, kmin=(0, 1), null_out=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32).reshape(-1).copy()).to(ctx.device)
    out = np.zeros(max(m, 1), dtype=np.dtype([("a", "<u4"), ("b", "<u4"), ("common", "<u4"), ("denom", "<u4"), ("size", "<u4")]))
    nm = C.c_uint32(77)
    st = ctx.lib.rtc_linkage_dev(ctx.h, m, C.c_void_p(d.data_ptr()), ld, kmin[0], kmin[1], None if null_out else out.ctypes.data_as(C.c_void_p),
                                 C.byref(nm))
    return st, _tuples(out[:nm.value])


@pytest.mark.parametrize("m", [40, 100])
def test_linkage_dev_padded_rows_and_argument_errors(ctx, m):
    from rabbittclust_amd import _lib
    keys = S.random_ties(m, seed=9)
    ld = m + 7
    padded = np.full((m, ld, 2), 0xFFFFFFFF, dtype=np.uint32)  # what lies beyond a row's m entries must never be read as a key
    padded[:, :m] = keys
    st, got = _dev(ctx, padded, m, ld)
    assert st == _lib.RTC_OK and got == R.rowbest(keys)[0]
    assert _dev(ctx, keys, m, m, kmin=(1, 0))[0] == _lib.RTC_ERR_ARG  # kmin_den == 0
    assert _dev(ctx, keys, m, m - 1)[0] == _lib.RTC_ERR_ARG            # ld < m
    assert _dev(ctx, keys, m, m, null_out=True)[0] == _lib.RTC_ERR_ARG
    nm = C.c_uint32(0)
    assert ctx.lib.rtc_linkage_dev(ctx.h, m, None, m, 0, 1, None, C.byref(nm)) == _lib.RTC_ERR_ARG
    assert ctx.lib.rtc_linkage_dev(ctx.h, m, None, m, 0, 1, None, None) == _lib.RTC_ERR_ARG


# ---- rtc_linkage_complete ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _component_case(kmin):
    sketches, comp = S.component_set()
    return sketches, comp, R.complete(sketches, comp, kmin)


def _sketch_set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=21, kind="kssd", width=width)


@pytest.fixture
def linkage_bytes(ctx, monkeypatch):
    def set_budget(v):
        if v is None:
            monkeypatch.delenv("RTC_LINKAGE_BYTES", raising=False)
        else:
            monkeypatch.setenv("RTC_LINKAGE_BYTES", str(v))
        ctx.reload_options()
    yield set_budget
    monkeypatch.delenv("RTC_LINKAGE_BYTES", raising=False)
    ctx.reload_options()


@pytest.fixture
def fill_switch(ctx, monkeypatch):
    def set_switch(name, v):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
        ctx.reload_options()
    yield set_switch
    for name in ("RTC_LINKAGE_SPAN", "RTC_PAIR_FORCE_MERGE"):
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


@pytest.mark.parametrize("width", [4, 8])
def test_linkage_complete_components_batches_and_limits(ctx, linkage_bytes, fill_switch, width):
    from rabbittclust_amd import _lib
    sketches, comp, (want, want_first) = _component_case((0, 1))
    assert len(want_first) == len(S.COMPONENT_SIZES) + 1 and want_first[-1] == len(want) > 200
    sk = _sketch_set(ctx, sketches, width)
    linkage_bytes(None)
    got, first = ctx.linkage_complete(sk, comp)
    assert _tuples(got) == want and first.tolist() == want_first
    c = ctx.linkage_counters()
    assert (c["components"], c["wave_components"], c["workgroup_components"]) == (5, 3, 2)  # 64, 5 and 2 in a wave; 130 and 65 not
    assert c["merges"] == len(want) and c["largest_m"] == 130 and c["batches"] == 1
    # a stop bound
    kmin = R.bound(0.05, 21)
    _, _, (want_b, first_b) = _component_case(kmin)
    got_b, fb = ctx.linkage_complete(sk, comp, kmin)
    assert _tuples(got_b) == want_b and fb.tolist() == first_b and 0 < len(want_b) < len(want)
    # the 130 alone needs its block and one band; with just that the components go in three batches: 64 | 130 | 65, 5, 2
    need = S.block_bytes(130) + S.band_bytes(130)
    linkage_bytes(need)
    got3, first3 = ctx.linkage_complete(sk, comp)
    assert _tuples(got3) == want and first3.tolist() == want_first
    assert ctx.linkage_counters()["batches"] >= 3
    linkage_bytes(need - 1)
    with pytest.raises(_lib.RtcError) as e:
        ctx.linkage_complete(sk, comp)
    assert e.value.status == _lib.RTC_ERR_NOMEM and "130" in str(e.value) and str(need) in str(e.value)
    linkage_bytes(None)
    # the fill's two switches: bands of 64 rows instead of one, and the per-pair merge kernel instead of the tiled one
    for name, value in (("RTC_LINKAGE_SPAN", "64"), ("RTC_PAIR_FORCE_MERGE", "1")):
        fill_switch(name, value)
        got_s, first_s = ctx.linkage_complete(sk, comp)
        fill_switch(name, None)
        assert _tuples(got_s) == want and first_s.tolist() == want_first, name
    # room for fewer merges than there are: the count comes back
    with pytest.raises(_lib.RtcError) as e:
        ctx.linkage_complete(sk, comp, cap=len(want) - 1)
    assert e.value.status == _lib.RTC_ERR_OVERFLOW and ctx.linkage_merges_needed == len(want)
    # argument errors
    with pytest.raises(_lib.RtcError) as e:
        ctx.linkage_complete(sk, comp, kmin=(1, 0))
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = 3
    with pytest.raises(_lib.RtcError) as e:
        ctx.linkage_complete(sk, comp)
    assert e.value.status == _lib.RTC_ERR_ARG
    sk.width = width
    nm = C.c_uint64(0)
    lab = np.zeros(sk.n, dtype=np.uint32)
    assert ctx.lib.rtc_linkage_complete(ctx.h, C.c_void_p(sk.hashes.data_ptr()), width, C.c_void_p(sk.start.data_ptr()), C.c_void_p(sk.len.data_ptr()),
                                        sk.n, lab.ctypes.data_as(C.c_void_p), 0, 1, None, 0, C.byref(nm), None) == _lib.RTC_ERR_ARG
    # every sketch its own component: nothing to do
    got1, first1 = ctx.linkage_complete(sk, np.arange(sk.n))
    assert len(got1) == 0 and first1.tolist() == [0] * (sk.n + 1) and ctx.linkage_counters()["components"] == 0


# ---- the command line --------------------------------------------------------------------------------------------------------
L = 1_000_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """20 genomes of 1 Mbp: three chains of four (each a mutated copy of the one before it, 1.8 % a step: neighbours are within
    0.03, the ends are not), two tight families of three and two strangers, listed in an order that scatters them"""
    tmp = str(tmp_path_factory.mktemp("linkage_fa"))
    rng = np.random.default_rng(11)
    seqs, names = [], []
    for c in range(3):
        s = rng.integers(0, 4, size=L)
        for i in range(4):
            seqs.append(s); names.append((f"c{c}_{i}", f"chain {c}"))
            s = _mutate(rng, s, 0.018)
    for f in range(2):
        base = rng.integers(0, 4, size=L)
        for i in range(3):
            seqs.append(_mutate(rng, base, 0.004)); names.append((f"f{f}_{i}", f"family {f}"))
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


def _check_outputs(oracle, genomes, out, metrics, fast, meta, by_file, threshold):
    m = json.load(open(metrics))
    k = int(m["kmer_size"])  # what the distances are formed with (a --fast folder reports half_k * 2)
    sk = _oracle_sketches(oracle, genomes["seqs"], fast, 17 if fast else k)
    single = _parse_clusters(out)
    want_cl, want_lines = R.refine(sk, single, threshold, k)
    assert open(out + ".complete").read() == R.cluster_text(want_cl, meta, by_file, threshold)
    assert open(out + ".complete.linkage.txt").read() == want_lines
    for key in ("linkage_fill_s", "linkage_agglomerate_s", "linkage_components", "linkage_merges", "linkage_clusters"):
        assert key in m, key
    assert m["linkage_clusters"] == len(want_cl) and m["linkage_merges"] == want_lines.count("\n")
    assert m["linkage_components"] == sum(1 for c in single if len(c) >= 2)
    # every two members of a result cluster are within the threshold
    sets = [set(int(h) for h in s) for s in sk]
    for c in want_cl:
        for i in c:
            for j in c:
                cm = len(sets[i] & sets[j])
                assert i == j or R.distance(cm, len(sets[i]) + len(sets[j]) - cm, k) <= threshold
    return single, want_cl


@pytest.mark.parametrize("mode", ["fast", "minhash"])
def test_cli_refines_the_clusters(oracle, genomes, tmp_path, mode):
    tmp = str(tmp_path)
    fast = mode == "fast"
    M = os.path.join(BIN, "clust-mst")
    args = ["-l", "-i", genomes["list"], "-d", "0.03", "-t", "4", "-e"] + (["--fast", "-k", "17"] if fast else ["-k", "21", "-s", "1000"])
    plain, out, mj = os.path.join(tmp, "plain.cluster"), os.path.join(tmp, "result.cluster"), os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", plain], tmp)
    err = _run([M] + args + ["-o", out, "--linkage", "complete"], tmp, env={"RTC_METRICS_JSON": mj})
    assert open(out, "rb").read() == open(plain, "rb").read()  # the plain result, byte for byte
    assert not os.path.exists(plain + ".complete")
    assert "-----write the complete-linkage cluster result into: " + out + ".complete\n" in err
    single, refined = _check_outputs(oracle, genomes, out, mj, fast, genomes["meta"], True, 0.03)
    # single linkage joins each chain, complete linkage splits it
    name = {g: mt[2] for g, mt in enumerate(genomes["meta"])}
    for c in range(3):
        chain = sorted(g for g in name if name[g].startswith(f"c{c}_"))
        assert sorted(next(cl for cl in single if chain[0] in cl)) == chain
        assert len([cl for cl in refined if set(cl) & set(chain)]) >= 2
    assert len(refined) > len(single)


def test_cli_presketched_and_single_fasta(oracle, genomes, tmp_path):
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    # --fast from a saved folder, with the tree flags and the post-processing beside it
    d1 = os.path.join(tmp, "a"); os.makedirs(d1)
    _run([M, "--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", "0.03", "-t", "4", "-o", os.path.join(d1, "a.cluster")], d1)
    folder = [os.path.join(d1, x) for x in os.listdir(d1) if os.path.isdir(os.path.join(d1, x))]
    assert len(folder) == 1
    out, mj = os.path.join(tmp, "p.cluster"), os.path.join(tmp, "p.json")
    _run([M, "--fast", "--presketched", folder[0], "-l", "-d", "0.03", "-o", out, "--linkage", "complete", "--linkage-matrix", "--dedup-dist", "0.01"],
         tmp, env={"RTC_METRICS_JSON": mj})
    assert os.path.exists(out + ".linkage.txt") and os.path.exists(out + ".dedup")  # what the other flags write is still written
    _check_outputs(oracle, genomes, out, mj, True, genomes["meta"], True, 0.03)
    # MinHash from one FASTA: sequences instead of files
    d2 = os.path.join(tmp, "s"); os.makedirs(d2)
    out2, mj2 = os.path.join(tmp, "s.cluster"), os.path.join(tmp, "s.json")
    _run([M, "-i", genomes["fasta"], "-k", "21", "-s", "1000", "-d", "0.03", "-t", "4", "-e", "-o", out2, "--linkage", "complete"], d2,
         env={"RTC_METRICS_JSON": mj2})
    seq_meta = [(mt[2], L, mt[3]) for mt in genomes["meta"]]
    _check_outputs(oracle, genomes, out2, mj2, False, seq_meta, False, 0.03)
