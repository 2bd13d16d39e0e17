"""bench.py's output protocol, host logic only (no GPU): the compact headline the driver parses stays a valid, bounded JSON
line whatever the extra workloads return -- round 5 lost its evidence to a numpy array formatted into a string."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _strings(o, path=""):
    if isinstance(o, dict):
        for k, v in o.items():
            yield from _strings(v, f"{path}.{k}")
    elif isinstance(o, list):
        for i, v in enumerate(o):
            yield from _strings(v, f"{path}[{i}]")
    elif isinstance(o, str):
        yield path, o


def test_compact_line_fits_whatever_the_extras_hold():
    """host logic only: the compact line stays below the limit and valid when the extras are huge, broken or absent"""
    import numpy as np
    import bench
    line = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": 1.0, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": {"workload": "w" * 250, "genomes_total": 1, "staging": "packed"}, "sketch_gbp_per_sec": 1.0, "dist_pairs_per_sec": 1.0,
            "mst_edges": 1, "clusters": 1, "phase_ms": {"sketch_ms": 1.0, "pair_ms": float("nan")},
            "roofline": {"bound": "hbm", "kernel": "k", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.1, "traffic": None},
            "cpu_baseline": {"value": 1.0, "unit": "u", "cores": 1, "kind": "port", "sample": "s" * 1000}}
    huge = {"dense_pairs": {"workload": f"{np.arange(2000)}", "pair_kernel_ms": np.float32(1.5)}, "cli": {"error": "x" * 5000},
            "junk": {str(i): "y" * 300 for i in range(200)}}
    c = bench.compact_line(line, huge)
    s = json.dumps(c)
    assert len(s) < 4096 and json.loads(s)["cpu_baseline"]["sample"] == "s" * 200
    assert c["extra_scalars"]["dense_pair_kernel_ms"] == 1.5 and "cli" in c["extra_errors"]
    assert c["phase_ms"]["pair_ms"] is None  # NaN never reaches the line
    full = bench.sanitize({"extra": huge})
    assert all(len(sv) <= 400 for _, sv in _strings(full))
    assert len(json.dumps(bench.compact_line(line))) < 4096


def test_north_star_genomes_do_not_depend_on_the_rank_count():
    """the strong-scaling job is the same 100 000 genomes at every N: a rank's descriptors are a slice of the job's"""
    import numpy as np
    import bench
    from rabbittclust_amd import api
    whole = bench.north_star_descs(api, "minhash", 0, 7500)
    assert len(whole) == 7500
    for world in (2, 3, 4):
        n_local = 7500 // world
        parts = [bench.north_star_descs(api, "minhash", r * n_local, (r + 1) * n_local) for r in range(world)]
        assert np.array_equal(np.concatenate(parts), whole[: n_local * world])
    assert not np.array_equal(bench.north_star_descs(api, "kssd", 0, 10), whole[:10])


def test_dump_outputs_writes_the_last_step_exactly(tmp_path):
    """--dump-outputs, host logic only: the forest and the sketches of a stand-in pipeline come back from the float64 .npy
    files bit for bit (64-bit hashes as two 32-bit halves), the sampled rows are the same from run to run, and the
    sample stays inside its byte budget"""
    import types
    import numpy as np
    import bench
    from rabbittclust_amd import api
    rng = np.random.default_rng(3)
    for width, n in ((8, 3000), (4, 50)):
        dt = np.uint64 if width == 8 else np.uint32
        sketches = [np.sort(rng.integers(0, np.iinfo(dt).max, size=int(rng.integers(0, 40)), dtype=dt, endpoint=True))
                    for _ in range(n)]
        mst = np.zeros(n - 1, dtype=api.EDGE_DT)
        mst["preNode"], mst["sufNode"] = rng.integers(0, n, size=n - 1), rng.integers(0, n, size=n - 1)
        mst["dist"] = rng.random(n - 1) / 3
        pipe = types.SimpleNamespace(last_mst=mst, last_sketches=api.SketchSet.from_host(sketches, "cpu", width=width))
        outs = []
        for run in range(2):
            d = tmp_path / f"w{width}_{run}"
            bench.dump_outputs(str(d), pipe)
            got = {f.stem: np.load(f) for f in d.glob("*.npy")}
            assert all(a.dtype == np.float64 for a in got.values())
            outs.append(got)
        a, b = outs
        assert set(a) == {"mst_pre_node", "mst_suf_node", "mst_dist", "sketch_len", "sketch_sample_rows",
                          "sketch_sample_hash_hi", "sketch_sample_hash_lo"}
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert np.array_equal(a["mst_pre_node"], mst["preNode"]) and np.array_equal(a["mst_suf_node"], mst["sufNode"])
        assert np.array_equal(a["mst_dist"], mst["dist"])
        assert np.array_equal(a["sketch_len"], [len(s) for s in sketches])
        rows = a["sketch_sample_rows"].astype(np.int64)
        assert len(rows) == min(n, bench.DUMP_SAMPLE_ROWS) and np.all(np.diff(rows) > 0)
        h = a["sketch_sample_hash_hi"].astype(np.uint64) << np.uint64(32) | a["sketch_sample_hash_lo"].astype(np.uint64)
        assert np.array_equal(h, np.concatenate([sketches[r] for r in rows]).astype(np.uint64))
    big = types.SimpleNamespace(last_mst=np.zeros(0, dtype=api.EDGE_DT),
                                last_sketches=api.SketchSet.from_host([np.arange(40_000, dtype=np.uint64)] * 200, "cpu"))
    bench.dump_outputs(str(tmp_path / "big"), big)
    rows = np.load(tmp_path / "big" / "sketch_sample_rows.npy")
    assert 0 < len(rows) < 200 and len(rows) * 40_000 * 16 <= bench.DUMP_SAMPLE_BYTES


def test_full_is_off_by_default(monkeypatch):
    """a plain `bench.py --gpus 1 --steps N --warmup W` runs no CPU baseline and no extra workload: both wait for --full"""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert not a.full and (a.gpus, a.steps, a.warmup) == (1, 20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse().full
