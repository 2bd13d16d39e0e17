"""GPU suite: rtc_louvain and rtc_leiden on the sets of tests/community_sets.py, each run held to its restatement exactly (labels,
cluster count, levels and rounds or the seven counters that are no times; the quality within the other files' tolerances).
tests/test_cpu_community_sets.py shows what the sets reach: a workgroup's second turn on the wave and the workgroup path, long
rows that propose under both objectives, rows of 128, 129, 2 048 and 2 049 entries, probe chains that wrap round the end of each
table, every cap, self loops with repeated and reversed records, and M2 within 2^20 of 2^46.  Every case prints its time and the
restatement's share of it."""
import time

import numpy as np
import pytest

import community_sets as S
import refleiden
import reflouvain
from refleiden import CPM, MODULARITY

pytestmark = pytest.mark.gpu

LIMIT_RESOLUTIONS = (0.25, 1.0, 2.0, 16384.0, 65535.0)

_BUILD = {
    "short": S.many_short_rows,  # these two take the device's compute units
    "long": S.many_long_rows,
    "heavy": lambda _: S.heavy_star(),
    "light": lambda _: S.heavy_star(1),
    "cycling": lambda _: S.cycling_star(),
    "nontarget": lambda _: S.nontarget_star(),
    "loops": lambda _: S.loops_and_duplicates(),
    "loops_large": lambda _: S.loops_and_duplicates_large(),
    "limit": lambda _: S.near_limit(),
}
_BUILD.update({"chain_%d" % m: (lambda _, m=m: S.chain(m)) for m in (8, 40, 70)})
_BUILD.update({"colliding_%d" % b: (lambda _, b=b: S.colliding_star(b)) for b in S.COLLIDING})
_BUILD.update({"star_%d%s" % (length, "_self" if loop else ""): (lambda _, length=length, loop=loop: S.boundary_star(length, loop))
               for length in S.BOUNDARY_LENGTHS for loop in (False, True)})

# (set, resolution, objective); objective None: rtc_louvain
_CASES = [(name, 1.0, None) for name in sorted(_BUILD)]
_CASES += [(name, r, o) for name in sorted(_BUILD) for r, o in ((0.25, CPM), (1.0, MODULARITY))]
_CASES += [("light", 1 / 4096, CPM), ("chain_70", 1 / 65536, CPM)]
_CASES += [("limit", r, o) for r in LIMIT_RESOLUTIONS for o in (None, CPM, MODULARITY) if (r, o) not in ((1.0, None), (0.25, CPM), (1.0, MODULARITY))]

_ARRAYS = {}


def _set(ctx, name):
    """(n, edges, records) of a set, built once"""
    if name not in _ARRAYS:
        from rabbittclust_amd import api
        n, edges = _BUILD[name](ctx.num_cu())
        rec = np.array(edges, dtype=np.int64).reshape(-1, 3)
        arr = np.zeros(len(edges), dtype=api.WEDGE_DT)
        arr["u"], arr["v"], arr["q"] = rec[:, 0], rec[:, 1], rec[:, 2]
        _ARRAYS[name] = (n, edges, arr)
    return _ARRAYS[name]


def _case_id(case):
    name, resolution, objective = case
    return "%s-%s-%g" % (name, {None: "louvain", CPM: "cpm", MODULARITY: "modularity"}[objective], resolution)


@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_equals_the_restatement(ctx, case):
    name, resolution, objective = case
    n, edges, arr = _set(ctx, name)
    t0 = time.perf_counter()
    if objective is None:
        labels, ncl, levels, rounds, quality = reflouvain.louvain(n, edges, resolution)
        want = (levels, rounds)
    else:
        labels, ncl, counters = refleiden.leiden(n, edges, resolution, objective)
        quality = refleiden.quality(n, edges, labels, resolution, objective)
        want = tuple(counters[:7])
    t1 = time.perf_counter()
    if objective is None:
        got, got_quality = ctx.louvain(n, arr, resolution, return_modularity=True)
        c = ctx.louvain_counters()
        got_counters, got_ncl, tolerance = (c["levels"], c["rounds"]), ctx.louvain_clusters, 1e-12
    else:
        got, got_quality = ctx.leiden(n, arr, resolution, objective, return_quality=True)
        c = ctx.leiden_counters()
        got_counters = tuple(c[k] for k in ("iterations", "levels", "move_rounds", "moves", "refine_rounds", "merges", "rejected"))
        got_ncl, tolerance = ctx.leiden_clusters, 1e-9
    t2 = time.perf_counter()
    print("%s: n %d, %d records, restatement %.2f s, GPU call %.3f s; clusters %d / %d, counters %s / %s, quality %.12g / %.12g"
          % (_case_id(case), n, len(edges), t1 - t0, t2 - t1, got_ncl, ncl, got_counters, want, got_quality, quality))
    assert got.tolist() == labels
    assert got_ncl == ncl
    assert got_counters == want
    assert abs(got_quality - quality) <= tolerance
    if objective is None:
        _check_paths(ctx, name, n, c)


def _check_paths(ctx, name, n, c):
    """which row-length paths the Louvain call took (rtc_louvain_counters: rows per round on the two long paths, and on the
    global one alone)"""
    if name.startswith("star_128"):
        assert c["long_rows"] == 0
    if name.startswith("star_129") or name.startswith("star_2048"):
        assert c["long_rows"] > 0 and c["global_rows"] == 0
    if name.startswith("star_2049"):
        assert c["global_rows"] > 0
    if name == "long":
        assert c["long_rows"] > 0 and c["global_rows"] == 0 and n > 3 * ctx.num_cu()  # more rows than the launch has workgroups
    if name == "short":
        assert n > 32 * ctx.num_cu() and c["long_rows"] == 0
    if name in ("colliding_8", "colliding_12"):
        assert c["global_rows"] == 0 and (c["long_rows"] > 0) == (name == "colliding_12")
    if name in ("colliding_13", "heavy", "light"):
        assert c["global_rows"] > 0
    if name == "chain_40":
        assert (c["levels"], c["rounds"]) == (32, 2048)  # both caps
