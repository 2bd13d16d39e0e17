"""CPU suite: rtc_graph_weight (host only) against tests/refgraph.py bit for bit, and the Louvain definition's restatement
(tests/reflouvain.py) on planted partitions."""
import numpy as np

import refgraph
import reflouvain


def test_graph_weight_equals_the_restatement():
    from rabbittclust_amd import api
    cases = [(0, 100, 100), (0, 0, 0), (100, 100, 100), (1, 1, 1), (1, 1000, 1000), (1, 2_000_000, 2_000_000), (999, 1000, 1000),
             (50, 100, 50), (3, 7, 11), (2_000_000_000, 2_100_000_000, 2_050_000_000)]
    rng = np.random.default_rng(5)
    for _ in range(400):
        a, b = (int(x) for x in rng.integers(1, 5000, size=2))
        cases.append((int(rng.integers(0, min(a, b) + 1)), a, b))
    clamps = set()
    for common, a, b in cases:
        for k in (1, 11, 19, 21, 31):
            want = refgraph.weight(common, a, b, k)
            assert api.graph_weight(common, a, b, k) == want, (common, a, b, k)
            clamps.add(want)
    # distance clamped at 1 (common 0, and a tiny jaccard at k = 1), and 0 at jaccard 1
    assert 0.0 in clamps and 1.0 in clamps
    assert refgraph.distance(1, 2_000_000, 2_000_000, 1) == 1.0 and refgraph.distance(100, 100, 100, 21) == 0.0


def _clique(vs, q):
    vs = list(vs)
    return [(a, b, q) for i, a in enumerate(vs) for b in vs[i + 1:]]


def test_two_cliques_and_a_bridge():
    one = 1 << 20
    labels, ncl, levels, rounds, mod = reflouvain.louvain(12, _clique(range(6), one) + _clique(range(6, 12), one) + [(5, 6, one)], 1.0)
    assert labels == [0] * 6 + [1] * 6 and ncl == 2
    assert levels == 2 and abs(mod - (30 / 31 - 0.5)) < 1e-12


def test_ring_of_cliques_merges_in_pairs():
    """A ring of 30 5-cliques with unit bridges at resolution 1.0.  The first level finds the 30 cliques; the second merges
    neighbouring cliques in pairs, which is Louvain's resolution limit (the pairs have the higher modularity: 0.8857 against
    0.8758 for the cliques alone), so the definition's own output is what is recorded here: 15 clusters of two adjacent
    cliques, but for one clique left alone and one group of three where the synchronous rounds close the ring.  At resolution 2.0 the cliques stay apart."""
    one = 1 << 20
    ring = []
    for c in range(30):
        ring += _clique(range(5 * c, 5 * c + 5), one) + [(5 * c + 4, (5 * c + 5) % 150, one)]
    labels, ncl, levels, rounds, mod = reflouvain.louvain(150, ring, 1.0)
    members = reflouvain.clusters_of(labels)
    cliques = [sorted({x // 5 for x in m}) for m in members]
    assert all(len(m) == 5 * len(c) for m, c in zip(members, cliques))  # no clique is split
    assert ncl == 15 and cliques == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11], [12, 13], [14], [15, 16], [17, 18], [19, 20],
                                     [21, 22], [23, 24], [25, 26], [27, 28, 29]]
    assert (levels, rounds) == (4, 85) and abs(mod - 0.8856565656565657) < 1e-12
    labels, ncl, _, _, _ = reflouvain.louvain(150, ring, 2.0)
    assert ncl == 30 and labels == [x // 5 for x in range(150)]


def test_restatement_input_rules():
    # duplicates are summed, a self loop counts 2q, the record's orientation does not matter
    a = reflouvain.louvain(4, [(0, 1, 5), (1, 0, 5), (2, 3, 4), (1, 2, 1), (3, 3, 2)], 1.0)
    b = reflouvain.louvain(4, [(1, 0, 10), (3, 2, 4), (2, 1, 1), (3, 3, 1), (3, 3, 1)], 1.0)
    assert a == b and a[0] == [0, 0, 1, 1]
    assert reflouvain.louvain(3, [], 1.0)[:4] == ([0, 1, 2], 3, 0, 0)
    assert reflouvain.quantise(1.0) == 1 << 20 and reflouvain.quantise(1e-9) == 1 and reflouvain.quantise(0.5 + 2.0 ** -21) == (1 << 19) + 1


# ---- the command line's flag errors: exit 1 before any GPU context exists ----
import os  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEIDEN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-leiden")


def _leiden(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([LEIDEN] + args, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=60)


def test_cli_flag_errors_need_no_gpu(tmp_path):
    out = ["-o", str(tmp_path / "x.out")]
    lst = ["-l", "-i", str(tmp_path / "none.list")]
    r = _leiden(["--louvain"] + lst + out, tmp_path)
    assert r.returncode == 1 and "ERROR: clust-leiden requires --fast option" in r.stderr
    r = _leiden(["--louvain", "--presketched", str(tmp_path)] + out, tmp_path)
    assert r.returncode == 1 and "ERROR: clust-leiden requires --fast option" in r.stderr
    r = _leiden(["--fast"] + lst + out, tmp_path)
    assert r.returncode == 1 and "Leiden refinement is not in this build; run with --louvain" in r.stderr
    r = _leiden(["--fast", "--louvain", "--drlevel", "9"] + lst + out, tmp_path)
    assert r.returncode == 1 and "ERROR: invalid drlevel 9, should be in [0, 8]" in r.stderr
    r = _leiden(["--louvain", "--pregraph", str(tmp_path)] + out, tmp_path)
    assert r.returncode == 1 and "leiden.graph" in r.stderr and "no MI355X context" not in r.stderr
    for r in (_leiden(["--fast", "--louvain", "--eps", "0.1"] + lst + out, tmp_path), _leiden(["--fast", "--louvain", "--resolution", "0"] + lst + out, tmp_path)):
        assert r.returncode == 1 and "ERROR" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.out"))


def test_cli_knn_defaulting_and_help(tmp_path):
    out = ["-o", str(tmp_path / "x.out"), "--drlevel", "9", "-l", "-i", "none"]  # ends at the drlevel check, after the defaulting
    r = _leiden(["--fast", "--louvain"] + out, tmp_path)
    assert "knn=1000" in r.stderr and "(k=1000)" in r.stderr
    r = _leiden(["--fast", "--louvain", "--knn", "0"] + out, tmp_path)
    assert "(k=1000)" in r.stderr
    r = _leiden(["--fast", "--louvain", "--knn", "3"] + out, tmp_path)
    assert "WARNING: --knn value too small (3), recommend at least 50. Using 50." in r.stderr and "(k=50)" in r.stderr
    r = _leiden(["--fast", "--louvain", "--knn", "70"] + out, tmp_path)
    assert "(k=70)" in r.stderr
    r = _leiden(["-h"], tmp_path)
    assert r.returncode == 0 and "--louvain" in r.stdout and "--save-graph" in r.stdout and "--pregraph" in r.stdout
