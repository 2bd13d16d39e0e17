"""CPU suite: clust-mst --db without a GPU -- the --stats report against tests/refmstdb.py on states written by
tests/refmststate.py, and the command line's validation of the --db actions (src/main.cpp:213-262, :525-600)."""
import os
import random
import subprocess

import pytest

import refmstdb as D
import refmststate as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MST = os.path.join(ROOT, "rabbittclust_amd", "bin", "clust-mst")

EDGE_SIZES = [1, 2, 5, 6, 10, 11, 100, 101, 1000, 1001]  # both sides of every histogram edge


def _bin():
    if not os.path.exists(MST):
        pytest.fail("clust-mst missing: run __graft_entry__.build()")
    return MST


def _state(kssd, use64, containment=False, seed=5):
    rng = random.Random(seed)
    st = M.State(kssd)
    st.use64 = use64
    st.threshold, st.kmer_size = 0.0375, 22 if kssd else 21
    if kssd:
        st.half_k, st.half_subk, st.drlevel = 11, 6, 3
    else:
        st.sketch_size, st.is_containment, st.contain_compress = 1000, containment, (500 if containment else 0)
    sizes = EDGE_SIZES + [0, 3]  # one retired slot (an empty cluster)
    hmax = (1 << 40) if use64 else (1 << 31)
    g = 0
    for r, sz in enumerate(sizes):
        members = list(range(g, g + sz))
        g += sz
        st.rep_ids.append(members[0] if members else 0)
        st.rep_lens.append(1_000_000 + r)
        st.rep_names.append("/db/rep%d.fna" % r)
        st.rep_hashes.append(sorted(rng.sample(range(1, min(hmax, 4000)), 60)))  # a small range: hashes shared across slots
        st.clusters.append(members)
    st.N = g
    st.member_names = ["/db/g%d.fna" % i for i in range(g)]
    st.member_lens = [100_000 + i for i in range(g)]
    return st


@pytest.mark.parametrize("kssd,use64,containment", [(True, False, False), (True, True, False), (False, True, False),
                                                     (False, True, True)])
def test_stats_prints_the_reference_report(tmp_path, kssd, use64, containment):
    st = _state(kssd, use64, containment)
    db = tmp_path / "rep.mstdb"
    db.write_bytes(M.save(st))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no GPU: --stats must not need one
    r = subprocess.run([_bin()] + (["--fast"] if kssd else []) + ["--db", str(db), "--stats"], capture_output=True, text=True,
                       timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == D.stats_text(st)
    assert "Live clusters:    11\n" in r.stdout and "Total reps slots: 12\n" in r.stdout


@pytest.mark.parametrize("kssd", [True, False])
def test_stats_refuses_truncated_and_foreign_files(tmp_path, kssd):
    raw = M.save(_state(kssd, not kssd))
    fl = ["--fast"] if kssd else []
    cut = tmp_path / "cut.mstdb"
    cut.write_bytes(raw[: len(raw) // 2])
    other = tmp_path / "other.mstdb"
    other.write_bytes(M.save(_state(not kssd, True)))  # the other magic
    for p in (cut, other, tmp_path / "missing.mstdb"):
        r = subprocess.run([_bin()] + fl + ["--db", str(p), "--stats"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "failed to load MST RepDB" in r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--db", "x.db", "--build", "-o", "o.txt"], "ERROR: --build requires --presketched <folder> or -i <genome_list> -l"),
    (["--db", "x.db", "--query", "-o", "o.txt"], "ERROR: --query requires -i <input_file>"),
    (["--db", "x.db", "--assign", "-o", "o.txt"], "ERROR: --assign requires -i <input_file>"),
    (["--db", "x.db", "-o", "o.txt"], "ERROR: --db requires one of: --build, --query, --assign, --append, --stats"),
    (["--db", "x.db", "--query", "-i", "q.txt", "-l"], "ERROR: option -o/--output is required"),
    (["--db", "x.db", "--assign", "-i", "q.txt", "--top-k", "3", "-o", "o.txt"], "ERROR: --top-k requires --query"),
    (["--db", "x.db", "--query", "--stats", "-i", "q.txt", "-o", "o.txt"], "exclude each other"),
    (["--build", "-i", "q.txt", "-l", "-o", "o.txt"], "require --db"),
])
def test_db_validation(tmp_path, args, msg):
    for fl in ([], ["--fast"]):
        r = subprocess.run([_bin()] + fl + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode != 0
        assert msg in r.stderr, r.stderr[-1000:]
