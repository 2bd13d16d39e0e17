"""clust-mst --pangenome on the device: rtc_pangenome against the restatement (tests/refpangenome.py) over the sets of
tests/pangenome_sets.py at width 4 and 8, by default and with every cluster in the arena (RTC_PAN_GLOBAL=1), its invariance under
the grouping, its refusal of a budget below one cluster, and the command line end to end.  Every comparison is exact; the path
counters are asserted, so a path that silently never ran fails."""
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pangenome_sets as PS
from tests import refpangenome as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
WIDTHS = (4, 8)
MODES = ("paths", "global")


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
    for name in ("RTC_PAN_GLOBAL", "RTC_PAN_BYTES"):
        set_switch(name, None)
    yield set_switch
    for name in names:
        monkeypatch.delenv(name, raising=False)
    ctx.reload_options()


def _sketch_set(ctx, sketches, width):
    from rabbittclust_amd import api
    dt = np.uint64 if width == 8 else np.uint32
    return api.SketchSet.from_host([np.asarray(s, dtype=dt) for s in sketches], ctx.device, k=21, kind="kssd", width=width)


@functools.lru_cache(maxsize=None)
def _reference(name, width, soft=95, cloud=15):
    """the set `name` at a width and what the restatement says of it: computed once, shared, never changed"""
    sketches, labels = _SETS[name](width)
    hashes = PS.materialise(sketches, width)
    want = R.pangenome(hashes, labels, soft, cloud)
    for a in want:
        a.setflags(write=False)
    return hashes, labels, want


def _turn_members():
    import torch
    from rabbittclust_amd import api
    return 4 * api.PAN_GLOBAL_WGS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count + 117


_SETS = {
    "edges": lambda w: PS.path_edges(),
    "wide": lambda w: PS.wide(),
    "tall": lambda w: PS.tall(),
    "turn": lambda w: PS.second_turn(_turn_members()),
    "wrap": lambda w: PS.wrapping(w),
    "markers": lambda w: PS.markers(),
    "labels": lambda w: PS.mixed_labels(),
    "arena": lambda w: PS.several_arena(),
    "one": lambda w: ([np.asarray([3, 9, 11], dtype=np.uint64)], [0]),
    "singletons": lambda w: (PS.mixed_labels()[0], list(range(len(PS.mixed_labels()[0])))),
    "everything": lambda w: (PS.mixed_labels()[0], [5] * len(PS.mixed_labels()[0])),
    "m2": lambda w: PS.thresholds(2),
    "m7": lambda w: PS.thresholds(7),
    "m20": lambda w: PS.thresholds(20),
}
# the clusters of a set on the wave / workgroup / arena path when the paths are chosen by record count
_PATHS = {"edges": (1, 2, 1), "wide": (0, 1, 0), "tall": (0, 1, 1), "turn": (0, 0, 1), "wrap": (0, 0, 1), "markers": (4, 1, 1),
          "arena": (2, 0, 6), "one": (1, 0, 0), "everything": (0, 0, 1)}


def _check(ctx, name, width, mode, switch, soft=95, cloud=15):
    from rabbittclust_amd import api
    hashes, labels, want = _reference(name, width, soft, cloud)
    switch("RTC_PAN_GLOBAL", 1 if mode == "global" else None)
    got = ctx.pangenome(_sketch_set(ctx, hashes, width), labels, soft, cloud)
    for g, w, what in zip(got, want, ("clusters", "hist", "genomes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (name, width, mode, what, bad[:5].tolist(), g[bad[:3]].tolist(), w[bad[:3]].tolist())
    cnt = ctx.pangenome_counters()
    n_cl = len(want[0])
    assert cnt["clusters"] == n_cl and cnt["clustered"] == int(want[0]["size"].sum()) and cnt["records"] == int(want[0]["total"].sum())
    assert cnt["distinct"] == int(want[0]["pan"].sum()) and cnt["groups"] >= 1
    if mode == "global":
        paths = (0, 0, n_cl)
    else:
        paths = _PATHS.get(name)
    if paths is not None:
        assert (cnt["wave_clusters"], cnt["block_clusters"], cnt["global_clusters"]) == paths, (name, cnt)
        bits = (api.PAN_PATH_WAVE if paths[0] else 0) | (api.PAN_PATH_BLOCK if paths[1] else 0) | (api.PAN_PATH_GLOBAL if paths[2] else 0)
        assert ctx.pangenome_last_path() == bits
    assert cnt["wave_clusters"] + cnt["block_clusters"] + cnt["global_clusters"] == n_cl
    return cnt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "wide", "tall", "wrap", "markers", "labels", "arena", "one", "singletons", "everything"])
def test_against_the_restatement(ctx, switch, name, width, mode):
    _check(ctx, name, width, mode, switch)


def test_the_sets_are_what_they_claim():
    """record counts at the limits, a histogram past 1 024 entries, the marker values present at both widths"""
    from rabbittclust_amd import api
    sk, lab = PS.path_edges()
    per = [sum(len(s) for s, x in zip(sk, lab) if x == c) for c in range(4)]
    assert per == [api.PAN_WAVE_RECORDS, api.PAN_WAVE_RECORDS + 1, api.PAN_BLOCK_RECORDS, api.PAN_BLOCK_RECORDS + 1]
    sk, lab = PS.tall()
    assert lab.count(0) == lab.count(1) == 1100 > api.PAN_BLOCK_HIST and sum(len(s) for s in sk[1100:]) <= api.PAN_BLOCK_RECORDS
    sk, lab = PS.markers()
    for width in WIDTHS:
        flat = np.concatenate(PS.materialise(sk, width))
        assert (flat == 0).sum() >= 8 and (flat == np.uint64(0xFFFFFFFF if width == 4 else api.PAN_EMPTY)).sum() >= 8


@pytest.mark.parametrize("width", WIDTHS)
def test_the_count_grid_takes_a_second_turn(ctx, switch, width):
    from rabbittclust_amd import api
    import torch
    cnt = _check(ctx, "turn", width, "paths", switch)
    assert cnt["clustered"] > 4 * api.PAN_GLOBAL_WGS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name,soft,cloud", [("m2", 100, 1), ("m2", 50, 50), ("m2", 51, 50), ("m7", 100, 1), ("m7", 86, 14), ("m7", 85, 15),
                                             ("m7", 43, 43), ("m20", 100, 1), ("m20", 95, 15), ("m20", 95, 16), ("m20", 96, 15), ("m20", 5, 5), ("m20", 6, 6),
                                             ("m20", 50, 50)])
def test_class_boundaries(ctx, switch, name, soft, cloud, width, mode):
    """100 occ against pct m at the values where a hash changes class: m = 2 at 50 / 51, m = 7 at 85 / 86 (occ 6) and 14 / 15
    (occ 1), m = 20 at 95 / 96 (occ 19), 15 / 16 (occ 3) and 5 / 6 (occ 1); 100 / 1 and equal values among them"""
    _check(ctx, name, width, mode, switch, soft, cloud)


def test_class_boundaries_move_a_hash():
    """the pairs above differ: the restatement puts a hash into another class on either side of each boundary"""
    def classes(m, soft, cloud):
        c, _, _ = R.pangenome(*PS.thresholds(m), soft, cloud)
        return tuple(int(c[0][k]) for k in ("core", "soft", "shell", "cloud"))
    assert classes(2, 50, 50) == (1, 1, 0, 0) and classes(2, 51, 50) == (1, 0, 1, 0) and classes(2, 100, 1) == (1, 0, 1, 0)
    assert classes(7, 85, 15) != classes(7, 86, 14) and classes(7, 85, 15)[1] == 1 and classes(7, 86, 14)[1] == 0
    assert classes(7, 85, 15)[3] == 1 and classes(7, 86, 14)[3] == 0
    assert classes(20, 95, 15)[3] == 2 and classes(20, 95, 16)[3] == 3 and classes(20, 5, 5)[3] == 0 and classes(20, 6, 6)[3] == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", WIDTHS)
def test_groups_give_the_same_records(ctx, switch, width, mode):
    from rabbittclust_amd import api
    hashes, labels, want = _reference("arena", width)
    biggest = max(api.pan_cluster_bytes(int(r["total"]), int(r["size"]), all_global=True) for r in want[0])
    switch("RTC_PAN_BYTES", 2 * biggest)
    cnt = _check(ctx, "arena", width, mode, switch)
    assert cnt["groups"] >= 3, cnt


def test_a_budget_below_one_cluster_is_refused(ctx, switch):
    from rabbittclust_amd import _lib, api
    hashes, labels, want = _reference("arena", 4)
    biggest = max(api.pan_cluster_bytes(int(r["total"]), int(r["size"])) for r in want[0])
    ss = _sketch_set(ctx, hashes, 4)
    switch("RTC_PAN_BYTES", biggest - 1)
    with pytest.raises(api.RtcError) as e:
        ctx.pangenome(ss, labels)
    assert e.value.status == _lib.RTC_ERR_NOMEM and str(biggest) in str(e.value), str(e.value)
    switch("RTC_PAN_BYTES", biggest)  # exactly one cluster's need: every cluster a group of its own at the most
    _check(ctx, "arena", 4, "paths", switch)
    switch("RTC_PAN_BYTES", None)
    _check(ctx, "arena", 4, "paths", switch)


def test_arguments(ctx, switch):
    from rabbittclust_amd import _lib, api
    hashes, labels, _ = _reference("labels", 4)
    ss = _sketch_set(ctx, hashes, 4)
    for soft, cloud in ((95, 0), (10, 20), (101, 15), (0, 0)):
        with pytest.raises(api.RtcError) as e:
            ctx.pangenome(ss, labels, soft, cloud)
        assert e.value.status == _lib.RTC_ERR_ARG
    bad = list(labels)
    bad[3] = len(bad)
    with pytest.raises(api.RtcError) as e:
        ctx.pangenome(ss, bad)
    assert e.value.status == _lib.RTC_ERR_ARG
    c, h, g = ctx.pangenome(ss, [-1] * len(labels))  # nobody is clustered
    assert len(c) == 0 and not h.any() and not g.view(np.uint8).any()


# ---- the command line ----------------------------------------------------------------------------------------------------------
L = 300_000


def _mutate(rng, seq, rate):
    out = seq.copy()
    at = np.flatnonzero(rng.random(len(seq)) < rate)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """10 genomes of 0.3 Mbp, listed in an order that scatters them: families of 5, 3 and 1 and one far copy, mutated at 0.4 %"""
    tmp = str(tmp_path_factory.mktemp("pan_fa"))
    rng = np.random.default_rng(41)
    seqs = []
    for size, rate in ((5, 0.004), (3, 0.006), (1, 0.0), (1, 0.0)):
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


EXTS = (".pangenome.tsv", ".pangenome.genomes.tsv", ".pangenome.hist.tsv", ".pangenome.curve.tsv")


def test_cli_writes_the_pangenome(ctx, genomes, tmp_path):
    from rabbittclust_amd import host
    tmp = str(tmp_path)
    M = os.path.join(BIN, "clust-mst")
    args = ["--fast", "-l", "-i", genomes["list"], "-k", "17", "-d", "0.05", "-t", "4"]
    dirs = {}
    for name in ("plain", "pan", "beside"):
        dirs[name] = os.path.join(tmp, name)
        os.makedirs(dirs[name])
    out1, out2, out3 = (os.path.join(dirs[name], "result.cluster") for name in ("plain", "pan", "beside"))
    mj = os.path.join(tmp, "m.json")
    _run([M] + args + ["-o", out1], dirs["plain"])
    err = _run([M] + args + ["-o", out2, "--pangenome", "--pan-soft", "80", "--pan-cloud", "30"], dirs["pan"], env={"RTC_METRICS_JSON": mj})
    _run([M] + args + ["-o", out3, "--pangenome", "--pan-soft", "80", "--pan-cloud", "30", "--quality", "--upgma"], dirs["beside"])
    assert open(out1, "rb").read() == open(out2, "rb").read() == open(out3, "rb").read()  # as without the flag, byte for byte
    for ext in EXTS:
        assert not os.path.exists(out1 + ext) and os.path.exists(out2 + ext), ext
        assert open(out2 + ext, "rb").read() == open(out3 + ext, "rb").read(), ext
    assert os.path.exists(out3 + ".quality.tsv") and os.path.exists(out3 + ".upgma.newick")
    assert "-----pangenome: " in err
    clusters = _parse_clusters(out2)
    paths = genomes["paths"]
    n = len(paths)
    assert sorted(g for c in clusters for g in c) == list(range(n)) and 2 <= len(clusters) < n
    # the restatement over the sketches the run saved
    folder = [os.path.join(dirs["pan"], x) for x in os.listdir(dirs["pan"]) if os.path.isdir(os.path.join(dirs["pan"], x))]
    assert len(folder) == 1
    raw = open(os.path.join(folder[0], "kssd.hash.sketch"), "rb").read()
    pos, sketches = 20, []
    for _ in range(n):
        (cnt,) = struct.unpack_from("<Q", raw, pos); pos += 8
        sketches.append(np.frombuffer(raw, dtype="<u4", count=cnt, offset=pos).copy()); pos += 4 * cnt
    assert pos == len(raw)
    cluster_of = np.zeros(n, dtype=np.int64)
    for q, c in enumerate(clusters):
        cluster_of[c] = q
    want = R.pangenome([s.astype(np.uint64) for s in sketches], cluster_of.tolist(), 80, 30)
    assert R.identities(*want, cluster_of.tolist()) == []
    texts = host.pangenome_report(paths, cluster_of, *want)
    for ext, text in zip(EXTS, texts):
        assert open(out2 + ext).read() == text, ext
    assert texts[0].count("\n") == 1 + len(clusters) and texts[1].count("\n") == 1 + n
    assert int(want[0]["core"].sum()) > 0 and len(texts[3].splitlines()) == 1 + sum(len(c) for c in clusters if len(c) >= 2)
    # and the library agrees with both
    got = ctx.pangenome(_sketch_set(ctx, sketches, 4), cluster_of, 80, 30)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    m = json.load(open(mj))
    for key in ("pangenome_count_s", "pangenome_sweep_s", "pangenome_genome_s", "pangenome_clusters", "pangenome_hashes", "pangenome_core_share_mean"):
        assert key in m, key
    assert m["pangenome_clusters"] == len(clusters) and m["pangenome_hashes"] == int(want[0]["pan"].sum()) and 0 < m["pangenome_core_share_mean"] <= 1
