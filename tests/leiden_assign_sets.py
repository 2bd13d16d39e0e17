"""Inputs the clust-leiden --db --assign tests share (tests/test_cpu_leiden_assign.py proves on the restatement that they hold
the cases they are meant to hold, tests/test_gpu_leiden_assign.py runs them on the device).  Sketches are sorted arrays of
distinct integers below 2^31, so every set serves both hash widths."""
import numpy as np

K = 21
THRESHOLD = 0.05


def _tools(seed):
    rng = np.random.default_rng(seed)

    def fresh(m):
        return rng.choice((1 << 31) - 2, size=m, replace=False).astype(np.int64) + 1

    def mutate(base, rate):
        s = base.copy()
        flip = rng.random(len(s)) < rate
        s[flip] = fresh(int(flip.sum()))
        return np.unique(s)
    return rng, fresh, mutate


_QUERY = {}


def query_case():
    """301 model genomes -- 30 families x 10 at three substitution rates, and a second copy of genome 3 -- and 40 queries:
    34 mutated family members at four rates, a copy of model genome 3 (two model genomes tie at the top of its rank), an empty
    sketch, two unrelated ones, one that holds a whole family base inside more than twice as many hashes of its own (only the
    size ratio fails), one built from two families"""
    if not _QUERY:
        rng, fresh, mutate = _tools(5)
        bases, model = [], []
        for f in range(30):
            base = fresh(200 + 7 * (f % 5))
            bases.append(base)
            model += [mutate(base, (0.02, 0.1, 0.3)[f % 3]) for _ in range(10)]
        model.append(model[3].copy())
        queries = [mutate(bases[f % 30], (0.02, 0.1, 0.3, 0.5)[f % 4]) for f in range(34)]
        queries += [model[3].copy(), np.zeros(0, dtype=np.int64), fresh(180), fresh(90), np.unique(np.concatenate([bases[7], fresh(520)])),
                    np.unique(np.concatenate([bases[0][:100], bases[3][:100]]))]
        assert len(model) == 301 and len(queries) == 40
        _QUERY.update(model=model, queries=queries)
    return _QUERY["model"], _QUERY["queries"]


COPY, EMPTY, UNRELATED, RATIO, STRADDLE = 34, 35, (36, 37), 38, 39

_LONG = {}


def long_case():
    """4 300 model sketches of 12 to 16 hashes, 4 200 of them around one core of 8 hashes; query 0 holds the core and query 3 one
    hash of it (their segments are longer than TK_LONG = 4 096), queries 1 and 2 are short ones beside them: a copy of one of
    the other 100 and an unrelated one"""
    if not _LONG:
        rng, fresh, _ = _tools(11)
        core = fresh(8)
        model = [np.unique(np.concatenate([core, fresh(4 + g % 5)])) for g in range(4200)] + [fresh(12 + g % 5) for g in range(100)]
        queries = [np.unique(np.concatenate([core, fresh(6)])), model[4250].copy(), fresh(14), np.unique(np.concatenate([core[:1], fresh(13)]))]
        _LONG.update(model=model, queries=queries)
    return _LONG["model"], _LONG["queries"]


_FAMILIES = {}


def holdout_case():
    """10 families x 7 genomes of about 150 hashes at substitution rates 0, 0.02, .. 0.12; the member at 0.04 of every family
    is held out as a query (under CPM the run scales its weights from their own range, and the member at 0.12 would be left
    with too little weight to pay for a community of six), and an unrelated sketch is the eleventh query -> (model of 60,
    queries of 11, family of every model genome)"""
    if not _FAMILIES:
        rng, fresh, mutate = _tools(23)
        model, queries, fam = [], [], []
        for f in range(10):
            base = fresh(140 + 3 * f)
            members = [mutate(base, 0.02 * (m % 7)) for m in range(7)]
            model += members[:2] + members[3:]
            fam += [f] * 6
            queries.append(members[2])
        queries.append(fresh(150))
        _FAMILIES.update(model=model, queries=queries, fam=fam)
    return _FAMILIES["model"], _FAMILIES["queries"], _FAMILIES["fam"]


def place_case(lv_wave_row=128, lv_block_row=2048, lv_wave_slots=256):
    """rtc_leiden_place alone: 3 000 model genomes in 700 communities and ten queries whose rows have 0, 1, LV_WAVE_ROW,
    LV_WAVE_ROW + 1, LV_BLOCK_ROW, LV_BLOCK_ROW + 1 and 2 200 distinct model genomes, one row of 400 entries in 300 communities
    (more than LV_WAVE_SLOTS / 2), one row whose two communities tie, one row of heavy records; some records are given twice
    (summed) and all are shuffled -> (labels, n_clusters, n_queries, records (u, v, q))"""
    rng = np.random.default_rng(31)
    n_db, ncl = 3000, 700
    labels = np.concatenate([np.arange(ncl), rng.integers(0, ncl, n_db - ncl)]).astype(np.int32)
    rows = [0, 1, lv_wave_row, lv_wave_row + 1, lv_block_row, lv_block_row + 1, 2200]
    records = []
    for u, m in enumerate(rows):
        for v in rng.choice(n_db, size=m, replace=False).tolist():
            records.append((u, int(v), int(rng.integers(1, 1 << 21))))
    assert lv_wave_slots // 2 < 300
    records += [(7, d, int(rng.integers(1 << 19, 1 << 20))) for d in range(300)] + [(7, int(v), 1 << 18) for v in rng.choice(np.arange(ncl, n_db), 100, replace=False)]
    a, b = int(np.flatnonzero(labels == 650)[0]), int(np.flatnonzero(labels == 12)[0])
    labels[[v for v in np.flatnonzero((labels == 650) | (labels == 12)) if v not in (a, b)]] = 1  # both communities: one member
    records += [(8, a, 1 << 20), (8, b, 1 << 20)]
    records += [(9, int(v), 0xFFFFFFFF) for v in range(40)]
    records += [records[i] for i in rng.choice(len(records), 500, replace=False)]  # duplicates: summed
    order = rng.permutation(len(records))
    return labels, ncl, 10, [records[i] for i in order]
