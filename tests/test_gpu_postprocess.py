"""GPU: the --dedup-dist tree medoid (rtc_tree_medoids) on the GPU against the host path and the Python restatement of the
reference (tests/refpost.py), and clust-mst --fast --dedup-dist / --reps-per-cluster end to end."""
import os
import struct
import subprocess

import numpy as np
import pytest

import refpost as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "rabbittclust_amd", "bin")
EDGE = np.dtype([("preNode", "<i4"), ("sufNode", "<i4"), ("dist", "<f8")])


def _group_edges(rng, nodes, shape, weights):
    """a tree over `nodes` (chain, star or random), weights from `weights` ('tie': few values incl. 0, 'rand': continuous)"""
    e = []
    for i in range(1, len(nodes)):
        p = i - 1 if shape == "chain" else 0 if shape == "star" else int(rng.integers(0, i))
        w = float(rng.choice([0.0, 0.001, 0.002])) if weights == "tie" else float(rng.random() * 0.01)
        e.append((int(nodes[i]), int(nodes[p]), w))
    return e


def _forest(seed, sizes, shape, weights, link=0.5):
    """groups of the given sizes over shuffled ids, joined by a few edges above the dedup distance (0.01)"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    ids = rng.permutation(n)
    edges, at, heads = [], 0, []
    for s in sizes:
        nodes = ids[at:at + s]
        edges += _group_edges(rng, nodes, shape, weights)
        heads.append(int(nodes[0]))
        at += s
    for i in range(1, len(heads)):
        if rng.random() < link:
            edges.append((heads[i], heads[int(rng.integers(0, i))], 0.02 + 0.01 * float(rng.random())))
    rng.shuffle(edges)
    lens = rng.choice([1000, 1000, 2000], size=n).astype(np.uint64) if weights == "tie" else rng.integers(1000, 10**6, size=n).astype(np.uint64)
    return n, edges, lens


def _medoids(ctx, n, edges, lens, mode, dedup=0.01):
    arr = np.array(edges, dtype=EDGE) if edges else np.zeros(0, dtype=EDGE)
    with ctx.env(RTC_DEDUP_GPU=mode):
        rep = ctx.tree_medoids(n, arr, dedup, lens, threads=8)
        return rep, ctx.dedup_last_path()


CASES = [(2, [2, 2, 2, 1], "rand", "tie"), (3, [3, 5, 17, 1, 1], "random", "tie"), (4, [64, 65, 63], "star", "tie"),
         (5, [200, 33], "chain", "rand"), (6, [300, 2, 2], "random", "rand"), (7, [1000], "random", "tie"),
         (8, [700, 129], "star", "rand"), (9, [600], "chain", "tie")]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,sizes,shape,weights", CASES)
def test_tree_medoids_gpu_equals_host_and_restatement(ctx, seed, sizes, shape, weights):
    n, edges, lens = _forest(seed, sizes, shape, weights)
    gpu, p_gpu = _medoids(ctx, n, edges, lens, 2)
    host, p_host = _medoids(ctx, n, edges, lens, 0)
    assert p_gpu == 2 and p_host == 1
    want = R.tree_medoids(n, [e for e in edges], 0.01, [int(x) for x in lens])
    assert host.tolist() == want
    assert gpu.tolist() == want


@pytest.mark.gpu
@pytest.mark.parametrize("shape,weights", [("chain", "rand"), ("star", "tie"), ("random", "tie"), ("random", "rand")])
def test_tree_medoids_gpu_equals_host_on_ten_thousand_members(ctx, shape, weights):
    """groups of 10^4 members (deep chains, stars, exact ties): GPU against the host path, which the test above pins to the
    restatement; the default switch sends a group this large to the GPU"""
    n, edges, lens = _forest(11, [10_000, 3000, 40, 2], shape, weights)
    gpu, p_gpu = _medoids(ctx, n, edges, lens, 2)
    host, p_host = _medoids(ctx, n, edges, lens, 0)
    auto, p_auto = _medoids(ctx, n, edges, lens, 1)
    assert (p_gpu, p_host, p_auto) == (2, 1, 3)
    assert np.array_equal(gpu, host) and np.array_equal(auto, host)


@pytest.mark.gpu
def test_tree_medoids_no_groups_and_refusals(ctx):
    rep, path = _medoids(ctx, 5, [(0, 1, 0.5), (2, 3, 0.7)], np.ones(5, dtype=np.uint64), 2)
    assert rep.tolist() == [0, 1, 2, 3, 4] and path == 0
    rep, path = _medoids(ctx, 3, [(0, 1, 0.0)], np.ones(3, dtype=np.uint64), 2, dedup=-1.0)
    assert rep.tolist() == [0, 1, 2] and path == 0
    from rabbittclust_amd import _lib
    with pytest.raises(_lib.RtcError):  # a cycle among the dedup edges: not a forest
        _medoids(ctx, 3, [(0, 1, 0.0), (1, 2, 0.0), (2, 0, 0.0)], np.ones(3, dtype=np.uint64), 2)


# ---- the command line ----
def _write_genomes(oracle, tmp, n_fam, per, L, seed):
    from rabbittclust_amd import api
    desc = api.synth_family_descs(n_fam, per, global_seed=seed, max_rate=0.02)
    paths = []
    for g, d in enumerate(desc):
        s = oracle.synth_genome(int(d["fam_seed"]), int(d["mut_seed"]), int(d["mut_thr"]), L - 997 * (g % 3))
        p = os.path.join(tmp, f"g{g:03d}.fna")
        with open(p, "wb") as f:
            f.write(f">g{g} synthetic family {g // per}\n".encode())
            f.write(s.tobytes() + b"\n")
        paths.append(p)
    lst = os.path.join(tmp, "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst, len(paths)


def _run(args, cwd, env=None):
    r = subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _edges(folder):
    raw = open(os.path.join(folder, "edge.mst"), "rb").read()
    (m,) = struct.unpack_from("<Q", raw, 0)
    a = np.frombuffer(raw, dtype=EDGE, count=m, offset=8)
    return [(int(x["preNode"]), int(x["sufNode"]), float(x["dist"])) for x in a]


def _lines(path):
    """cluster text -> (clusters, {id: the line's text after the index column})"""
    cl, rest = [], {}
    for ln in open(path):
        if ln.startswith("the cluster"):
            cl.append([])
        elif ln.startswith("\t"):
            f = ln.rstrip("\n").split("\t", 2)
            cl[-1].append(int(f[2].split("\t")[0]))
            rest[cl[-1][-1]] = f[2]
    return cl, rest


def _text(clusters, rest):
    out = []
    for i, c in enumerate(clusters):
        out.append("the cluster %d is: \n" % i)
        out += ["\t%5d\t%s\n" % (j, rest[g]) for j, g in enumerate(c)]
        out.append("\n")
    return "".join(out)


def _check_post(out, forest, n, dedup, k):
    """the .dedup / .reps files beside `out` against the restatement applied to `forest` (also checks out's own clusters)"""
    cl, rest = _lines(out)
    lens = [int(rest[i].split("\t")[1].strip()[:-2]) for i in range(n)]
    rep, cl_want, cd, reps = R.dedup_and_reps(n, forest, lens, dedup, k)
    assert cl == cl_want
    assert open(out + ".dedup").read() == _text(cd, rest)
    assert open(out + ".reps").read() == _text(reps, rest)
    return cd, reps


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True])
def test_clust_mst_fast_dedup_and_reps_end_to_end(oracle, tmp_path, dense):
    tmp = str(tmp_path)
    lst, n = _write_genomes(oracle, tmp, 4, 6, 400_000, seed=21)
    mst_bin = os.path.join(BIN, "clust-mst")
    base = [mst_bin, "--fast", "-l", "-i", lst, "-k", "21", "-d", "0.05", "-t", "4"] + (["--dense"] if dense else [])
    plain = os.path.join(tmp, "plain.out")
    _run(base + ["-e", "-o", plain], tmp)
    out = os.path.join(tmp, "post.out")
    # the medoids of the first run on the GPU whatever the group sizes
    _run(base + ["--dedup-dist", "0.004", "--reps-per-cluster", "2", "-o", out], tmp, env={"RTC_DEDUP_GPU": "2"})
    assert open(out, "rb").read() == open(plain, "rb").read()  # the clustering is untouched
    folder = [os.path.join(tmp, d) for d in os.listdir(tmp) if os.path.isdir(os.path.join(tmp, d)) and d[:2] == "20"][0]
    mst = _edges(folder)
    forest = R.forest(mst, 0.05)
    cd, _ = _check_post(out, forest, n, 0.004, 2)
    assert sum(len(c) for c in cd) < n, "the dedup distance collapses nothing: the test shows nothing"
    if dense:
        assert open(out + ".removeNoise", "rb").read() == open(plain + ".removeNoise", "rb").read()
        cl_new, _ = _lines(out + ".removeNoise")
        where = {g: i for i, c in enumerate(cl_new) for g in c}
        f2 = [e for e in forest if where[e[0]] == where[e[1]]]  # modifyForest's result: the forest edges inside the new clusters
        _check_post(out + ".removeNoise", f2, n, 0.004, 2)
    else:
        assert not os.path.exists(out + ".removeNoise.dedup")
    # from the stored sketches, host medoids, K at 1 and above every cluster's size, dedup above the threshold
    for k, dd in ((1, 0.004), (50, 0.2)):
        out2 = os.path.join(tmp, "pre%d.out" % k)
        pre = [mst_bin, "--fast", "--presketched", folder, "-d", "0.05", "-t", "4", "--dedup-dist", str(dd), "--reps-per-cluster", str(k)]
        _run(pre + (["--dense"] if dense else []) + ["-o", out2], tmp, env={"RTC_DEDUP_GPU": "0"})
        assert open(out2, "rb").read() == open(plain, "rb").read()
        _check_post(out2, forest, n, dd, k)


@pytest.mark.gpu
def test_clust_mst_minhash_accepts_dedup_without_output(oracle, tmp_path):
    tmp = str(tmp_path)
    lst, n = _write_genomes(oracle, tmp, 2, 3, 300_000, seed=3)
    out = os.path.join(tmp, "mh.out")
    plain = os.path.join(tmp, "plain.out")
    args = [os.path.join(BIN, "clust-mst"), "-l", "-i", lst, "-k", "21", "-s", "1000", "-d", "0.05", "-t", "4", "-e"]
    _run(args + ["-o", plain], tmp)
    _run(args + ["--dedup-dist", "0.01", "--reps-per-cluster", "2", "--auto-threshold", "-o", out], tmp)
    assert open(out, "rb").read() == open(plain, "rb").read()
    for ext in (".dedup", ".reps", ".threshold_analysis.txt"):  # compute_clusters honours none of them
        assert not os.path.exists(out + ext)
