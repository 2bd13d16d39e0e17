"""CPU suite: rtc_leiden's definition through its restatement (tests/refleiden.py) on graphs small enough to check on paper,
the host's weight normalisation and quantisation against a few lines of Python, and clust-leiden --leiden's flag errors."""
import os
import subprocess

import numpy as np

import leiden_sets
import refleiden
from refleiden import CPM, MODULARITY

ONE = leiden_sets.ONE


def test_two_cliques_refinement_keeps_pieces():
    """Two 4-cliques and a light edge between vertices 3 and 4, modularity.  At resolution 1.0 the move phase of level 0 ends
    with the two cliques as coarse communities; in the refinement's round 0 every vertex of the second clique proposes vertex
    4 but vertex 4 proposes too, so they are rejected, and the clique is left in two connected pieces that the next level
    joins.  No refined community ever spans the light edge.  At resolution 0.002 the move phase of the level at which the
    cliques are single vertices merges them, and one cluster results: there the refinement merges them too, because for two
    single vertices the move's condition e A > g B nu_x N_d is the eligibility condition with > for >=."""
    n, edges = leiden_sets.two_cliques()
    stats = {"trace": []}
    labels, ncl, C = refleiden.leiden(n, edges, 1.0, MODULARITY, stats)
    assert labels == [0] * 4 + [1] * 4 and ncl == 2
    iteration, level, coarse, refined = stats["trace"][0]
    assert (iteration, level) == (0, 0)
    assert len(set(coarse[:4])) == 1 and len(set(coarse[4:])) == 1 and coarse[0] != coarse[4]
    assert refined == [0, 0, 0, 0, 4, 4, 7, 7]
    assert stats["split"] >= 1 and C[6] > 0
    for _, _, coarse, refined in stats["trace"]:
        for a, b in zip(coarse, refined):
            assert [c for c, r in zip(coarse, refined) if r == b].count(a) == refined.count(b)  # a refined community lies in one coarse one
    assert C[0] == 2 and C[1] == 6  # the second iteration returns the first one's labels
    labels, ncl, _ = refleiden.leiden(n, edges, 0.002, MODULARITY)
    assert labels == [0] * 8 and ncl == 1


def test_path_proposals_chain():
    """A path of nine unit edges: on an even round every vertex but vertex 0 proposes its lower neighbour, so every proposal but
    the one into vertex 0 meets a target that proposes itself and is rejected; the restatement asserts that every round with a
    proposal accepts one."""
    n, edges = leiden_sets.path()
    stats = {}
    labels, ncl, C = refleiden.leiden(n, edges, 1.0, MODULARITY, stats)
    assert C[6] > 0 and C[5] > 0 and stats["ineligible"] > 0
    assert labels == [0, 0, 0, 0, 1, 1, 1, 1, 1] and ncl == 2
    labels, ncl, C = refleiden.leiden(n, edges, 0.5, CPM, stats)
    assert labels == [0, 0, 1, 1, 2, 3, 3, 4, 4] and C[6] == 0


def test_pendant_vertex_fails_eligibility():
    """leiden_sets.pendant, CPM at 0.25: the move phase puts all six vertices into community 0; vertex 5 holds 0.5 towards a
    community of 5 others, below 0.25 * 5, so it is not eligible and the refinement merges the clique without it"""
    n, edges = leiden_sets.pendant()
    stats = {"trace": []}
    labels, ncl, C = refleiden.leiden(n, edges, 0.25, CPM, stats)
    iteration, level, coarse, refined = stats["trace"][0]
    assert coarse == [0] * 6 and refined == [0, 0, 0, 0, 0, 5]
    assert stats["ineligible"] >= 1 and stats["split"] >= 1
    assert labels == [0] * 6 and ncl == 1  # a move never opens an empty community, so vertex 5 stays in the coarse one


def test_cpm_at_resolution_one_or_more_moves_nothing():
    n, edges = leiden_sets.random_graph()
    assert max(q for _, _, q in edges) <= ONE and len({(u, v) for u, v, _ in edges}) == len(edges)
    for resolution in (1.0, 2.0):
        labels, ncl, C = refleiden.leiden(n, edges, resolution, CPM)
        assert labels == list(range(n)) and ncl == n
        assert C[:7] == [1, 1, 2, 0, 2, 0, 0]
    assert refleiden.leiden(n, edges, 0.5, CPM)[1] < n


def test_restatement_input_rules():
    # duplicates are summed, a self record counts 2q, the record's orientation does not matter
    for objective, resolution, s in ((MODULARITY, 1.0, 1), (CPM, 0.25, 1 << 17)):  # CPM: weights of 1.25, 0.5 and 0.125 units
        a = refleiden.leiden(4, [(0, 1, 5 * s), (1, 0, 5 * s), (2, 3, 4 * s), (1, 2, s), (3, 3, 2 * s)], resolution, objective)
        b = refleiden.leiden(4, [(1, 0, 10 * s), (3, 2, 4 * s), (2, 1, s), (3, 3, s), (3, 3, s)], resolution, objective)
        assert a == b and a[0] == [0, 0, 1, 1], (objective, a, b)
    assert refleiden.leiden(3, [], 1.0, CPM) == ([0, 1, 2], 3, [0] * 10)
    # the self record adds to k_3 and so to modularity's node weight, not to any e_d
    with_loop = refleiden.quality(4, [(0, 1, 5), (2, 3, 4), (3, 3, 2)], [0, 0, 1, 1], 1.0, MODULARITY)
    assert abs(with_loop - (10 / 22 + 12 / 22 - (10 * 10 + 12 * 12) / (22 * 22))) < 1e-12


def _quantise_in_python(records, objective):
    """the few lines the host function is held to"""
    if objective == MODULARITY:
        return [(u, v, max(1, refleiden._llround(w * 2.0 ** 20))) for u, v, w in records]
    lo = min([1.0] + [w for _, _, w in records])
    hi = max([0.0] + [w for _, _, w in records])
    if hi - lo < 0.5 and hi - lo > 1e-6:
        records = [(u, v, (w - lo) / (hi - lo)) for u, v, w in records]
    return [(u, v, q) for u, v, q in ((u, v, refleiden._llround(w * 2.0 ** 20)) for u, v, w in records) if q >= 1]


def test_host_quantise_equals_python():
    from rabbittclust_amd import host
    rng = np.random.default_rng(3)
    narrow = [(int(a), int(b), float(w)) for a, b, w in zip(rng.integers(0, 50, 200), rng.integers(0, 50, 200), 0.9 + 0.1 * rng.random(200))]
    cases = {
        "narrow": (narrow, True, True),  # normalised; the lightest record drops out
        "wide": ([(0, 1, 0.2), (1, 2, 0.95), (2, 3, 0.5), (3, 4, 1e-9)], False, True),  # range >= 0.5: as they are; 1e-9 rounds to 0
        "flat": ([(0, 1, 0.75), (1, 2, 0.75), (2, 3, 0.75 + 5e-7)], True, False),  # range <= 1e-6: as they are, the line still printed
        "half": ([(0, 1, 0.5), (1, 2, 1.0)], False, False),  # range exactly 0.5 is not below it
        "empty": ([], True, False),
    }
    for name, (records, narrow_flag, drops) in cases.items():
        u, v, w = ([r[i] for r in records] for i in range(3))
        for objective in (CPM, MODULARITY):
            got, flag = host.leiden_quantise(u, v, w, objective)
            want = _quantise_in_python(records, objective)
            assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in got] == want, (name, objective)
            assert want == refleiden.normalise_and_quantise(records, objective)[0]
            assert flag == (narrow_flag and objective == CPM), (name, objective)
            assert (len(want) < len(records)) == (drops and objective == CPM), (name, objective)
    got, _ = host.leiden_quantise([0, 1], [1, 2], [0.9, 1.0], CPM)
    assert [(int(r["u"]), int(r["v"]), int(r["q"])) for r in got] == [(1, 2, ONE)]


# ---- the command line's flag errors: exit 1 before any GPU context exists ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEIDEN = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-leiden")


def _leiden(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([LEIDEN] + args, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=60)


def test_cli_leiden_flag_errors_need_no_gpu(tmp_path):
    out = ["-o", str(tmp_path / "x.out")]
    lst = ["-l", "-i", str(tmp_path / "none.list")]
    r = _leiden(["--fast", "--leiden", "--louvain"] + lst + out, tmp_path)
    assert r.returncode == 1 and "ERROR: --leiden and --louvain exclude each other" in r.stderr and "no MI355X context" not in r.stderr
    r = _leiden(["--fast", "--leiden", "--objective", "bogus"] + lst + out, tmp_path)
    assert r.returncode == 1 and "ERROR: --objective must be cpm or modularity, got bogus" in r.stderr
    r = _leiden(["--fast"] + lst + out, tmp_path)
    assert r.returncode == 1 and "Leiden refinement is not in this build; run with --louvain" in r.stderr and "--leiden" in r.stderr
    r = _leiden(["--leiden"] + lst + out, tmp_path)
    assert r.returncode == 1 and "ERROR: clust-leiden requires --fast option" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.out"))


def test_cli_leiden_knn_defaulting_and_help(tmp_path):
    out = ["-o", str(tmp_path / "x.out"), "--drlevel", "9", "-l", "-i", "none"]  # ends at the drlevel check, after the defaulting
    r = _leiden(["--fast", "--leiden"] + out, tmp_path)
    assert r.returncode == 1 and "ERROR: invalid drlevel 9" in r.stderr
    assert "-----Auto-selecting k-NN: k=500 (use --knn 0 to disable)" in r.stderr and "-----Algorithm: Leiden" in r.stderr and "(k=500)" in r.stderr
    assert "knn=1000" not in r.stderr
    r = _leiden(["--fast", "--leiden", "--knn", "3", "--objective", "modularity"] + out, tmp_path)
    assert "WARNING: --knn value too small (3), recommend at least 50. Using 50." in r.stderr and "(k=50)" in r.stderr
    r = _leiden(["--fast", "--leiden", "--knn", "70"] + out, tmp_path)
    assert "(k=70)" in r.stderr
    r = _leiden(["-h"], tmp_path)
    assert r.returncode == 0 and "--leiden" in r.stdout and "--objective cpm|modularity" in r.stdout and "--resolution below 1" in r.stdout
