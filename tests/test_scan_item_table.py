"""The shadow list scan with the plan's item tables (option h16_items: one record per work item, the tile filled for its valid rows
only, pieces and constants requested together; 2 = whatever the plan, 1 = the default: where the plan takes three launches) against
the search over work_off and the padded tile fill (h16_items = 0): the same search run with each must return the oracle's ids and
distances bit for bit and leave, per query, the same number of candidates and the same set of approximate keys (the order inside a buffer is the order of the appends: it may differ).

The index: n = 4096 rows in 8 lists of CHOSEN lengths -- an empty list (a centroid far from every row: no items), 20 rows (block 0
only: a sample item and no main item), 33 rows (one row in block 1), 64, 65, and three long lists (1000, 1414, 1500 rows).  With the
pruning off and nprobe = 8 every query probes every list, so a list holds exactly nq pairs: nq = 1 / 31 / 32 / 33 / 97 / 130 against
tiles of 32 (h16_ncb = 1) and 96 (h16_ncb = 3) queries give short tiles, exactly full column blocks, one pair in the next block, two
tiles of a list and a last tile of one pair.  d = 768 (6 i8r chunks, 12 fp16 chunks) and d = 100 (a padded last chunk)."""
import ctypes as C

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o
from test_i8r_shadow import blobs, build_ivf, last_keys, oracle, same, shadow_form  # noqa: F401  (blobs: the row model)

LENGTHS = [0, 20, 33, 64, 65, 1000, 1414, 1500]
N, NLIST, K, CAP = sum(LENGTHS), len(LENGTHS), 10, 8192
NQS = [1, 31, 32, 33, 97, 130]
NQ_MAX = 1100
assert N == 4096

_cache = {}


def index_and_queries(d, form, metric, opt):
    """One index per (d, shadow form, metric), shared by the cases; queries: the first nq of one seeded set."""
    key = (d, form, metric)
    if key not in _cache:
        rng = np.random.default_rng(9000 + d)
        cents = rng.standard_normal((NLIST, d), dtype=np.float32)
        labels = np.repeat(np.arange(NLIST), LENGTHS)
        rng.shuffle(labels)
        x = (cents[labels] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
        q = (cents[rng.integers(1, NLIST, NQ_MAX)] + 0.3 * rng.standard_normal((NQ_MAX, d), dtype=np.float32)).astype(np.float32)
        # the centroid no row is assigned to: far from every row (L2), without a product with any (inner product)
        cents[0] = 50.0 * rng.standard_normal(d, dtype=np.float32) if metric == capi.METRIC_L2 else 0.0
        opt("h16_form", form)
        if metric == capi.METRIC_L2:
            ix = build_ivf(x, NLIST, centroids=cents)
        else:
            ix = capi.Index(capi.INDEX_IVFFLAT, metric, d, "ncentroids=%d" % NLIST)
            ix.set_centroids(cents)
            ix.add(x)
            ix.build()
        assert shadow_form(ix) == int(form)
        off = np.asarray(ix.export()[1], np.int64)
        assert np.diff(off).tolist() == LENGTHS, "the lists have the chosen lengths"
        _cache[key] = (ix, q)
    return _cache[key]


def reference(ix, q, nprobe, metric):
    if metric == capi.METRIC_L2:
        oi, od, _ = oracle(ix, q, nprobe, K)
    else:
        cent, off, vecs, lids = ix.export()
        oi, od, _ = o.ivf_search(cent, off, vecs, lids, q, nprobe, K, o.METRIC_IP)
    return oi, od


def item_tables():
    """msvs_debug_h16_items: (given, capacity, work items) of the main and the sample launch's table of the last list scan, the
    blocks per segment the plan chose, and the records that do not fit the plan (checked on the host against work_off / pair_off)."""
    out = np.zeros(9, np.uint32)
    rc = capi.lib().msvs_debug_h16_items(out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, capi.lib().msvs_last_error()
    return {"main": out[0:3].tolist(), "seg_blocks": int(out[3]), "main_misfits": int(out[4]), "sample": out[5:8].tolist(),
            "sample_misfits": int(out[8])}


FUSED_PAIRS = 8192  # scan_kernels.hpp: PLAN_FUSED_PAIRS
_plan_fused = {"on": True}


def tables_expected(items, pairs):
    """h16_items = 2: always; 1 (the default): where the plan takes three launches; 0: never."""
    return items == "2" or (items == "1" and (pairs > FUSED_PAIRS or not _plan_fused["on"]))


def scan(ix, q, nprobe, opt, items):
    opt("h16_items", items)
    p0 = capi.prefilter_stats()
    ids, dis = ix.search(q, K, "nprobe=%d" % nprobe)
    assert capi.prefilter_stats()[0] - p0[0] == len(q), "the shadow list scan did not run"
    tables = item_tables()  # (before the keys: reading them retires the record of the pass)
    if tables_expected(items, len(q) * nprobe):
        # both launches were given a table, no larger than its capacity (the kernels read it then), every record fits the plan
        assert tables["main"][0] == 1 and tables["main"][2] <= tables["main"][1] and tables["main_misfits"] == 0, tables
        assert tables["sample"][0] == 1 and tables["sample"][2] <= tables["sample"][1] and tables["sample_misfits"] == 0, tables
    else:
        assert tables["main"][0] == 0 and tables["sample"][0] == 0, tables
    keys, cnt = last_keys(len(q), CAP)
    for qi in range(len(q)):
        keys[qi, : cnt[qi]].sort()
        keys[qi, cnt[qi]:] = 0
    return ids, dis, keys, cnt, tables


def check(ix, q, nprobe, opt, metric=capi.METRIC_L2):
    """h16_items = 0, 2 (tables whatever the plan) and 1 (the default): the oracle's results from all, the same counts and the same
    sorted keys."""
    oi, od = reference(ix, q, nprobe, metric)
    old = scan(ix, q, nprobe, opt, "0")
    same(old[0], old[1], oi, od)
    for items in ("2", "1"):
        new = scan(ix, q, nprobe, opt, items)
        same(new[0], new[1], oi, od)
        assert np.array_equal(old[3], new[3]), "candidate counts differ (h16_items = %s)" % items
        assert (new[3] <= CAP).all()
        assert np.array_equal(old[2], new[2]), "candidate keys differ (h16_items = %s)" % items
        if items == "2":
            forced = new
    return forced


def knobs(opt, prune=False):
    opt("ivf_pass", "2")
    opt("lat_path", "0")
    opt("cand_cap", str(CAP))
    if not prune:
        opt("h16_preprune", "0")
        opt("h16_prune", "0")


CONFIGS = [(768, "3", capi.METRIC_L2), (100, "3", capi.METRIC_L2), (768, "2", capi.METRIC_L2), (100, "2", capi.METRIC_L2),
           (768, "2", capi.METRIC_IP)]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d,form,metric", CONFIGS, ids=["i8r-768", "i8r-100", "fp16-768", "fp16-100", "fp16-ip-768"])
def test_every_list_probed_by_every_query(d, form, metric, nq, opt):
    ix, q = index_and_queries(d, form, metric, opt)
    knobs(opt)
    for ncb in ("1", "3"):
        opt("h16_ncb", ncb)
        check(ix, q[:nq], NLIST, opt, metric)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("d,form", [(768, "3"), (100, "2")])
def test_segments_chosen_on_the_device(d, form, fused, opt):
    """h16_segs = 2: segments of at least 8 blocks, so the long lists (32, 45 and 47 blocks) are cut in several; the table is written
    by the fused plan's one launch (fused = 1) and by the scatter launch of the three-launch plan."""
    ix, q = index_and_queries(d, form, capi.METRIC_L2, opt)
    knobs(opt)
    opt("h16_segs", "2")
    opt("h16_ncb", "1")
    opt("plan_fused", fused)
    _plan_fused["on"] = fused == "1"
    try:
        for nq in (33, 130):
            new = check(ix, q[:nq], NLIST, opt)
            tiles = 6 * ((nq + 31) // 32)  # six lists reach beyond block 0; tiles of 32 queries
            assert new[4]["seg_blocks"] >= 8 and new[4]["main"][2] > tiles, "no list was cut into segments: %s" % new[4]
    finally:
        _plan_fused["on"] = True


@pytest.mark.gpu
@pytest.mark.parametrize("d,form", [(768, "3"), (100, "2")])
def test_few_workgroups_walk_many_items(d, form, opt):
    """h16_grid = 3: three workgroups share the 7 lists x 5 tiles of 130 queries at 32 per tile -- a dozen items each, one after the
    other over the tile rows the item before left behind."""
    ix, q = index_and_queries(d, form, capi.METRIC_L2, opt)
    knobs(opt)
    opt("h16_grid", "3")
    opt("h16_ncb", "1")
    check(ix, q[:130], NLIST, opt)
    check(ix, q[:97], NLIST, opt)


@pytest.mark.gpu
@pytest.mark.parametrize("d,form", [(768, "3"), (100, "2")])
def test_three_launch_plan_writes_the_tables(d, form, opt):
    """nq = 1100: 8800 pairs, above the fused plan's limit."""
    ix, q = index_and_queries(d, form, capi.METRIC_L2, opt)
    knobs(opt)
    check(ix, q[:NQ_MAX], NLIST, opt)


@pytest.mark.gpu
@pytest.mark.parametrize("d,form", [(768, "3"), (100, "2")])
def test_second_stage_plan_has_its_own_table(d, form, opt):
    """Default pruning, the second stage forced (h16_prune = 2): the main launch reads the table of the plan over the surviving
    pairs.  The pruning counters show that the stage ran."""
    ix, q = index_and_queries(d, form, capi.METRIC_L2, opt)
    knobs(opt, prune=True)
    opt("h16_prune", "2")
    opt("rerank_stats", "1")
    s0 = capi.debug_prune_stats()
    check(ix, q[:300], NLIST, opt)
    assert capi.debug_prune_stats()[1] > s0[1], "the second pruning stage did not run"
    opt("h16_prune", None)
    check(ix, q[:300], NLIST, opt)
