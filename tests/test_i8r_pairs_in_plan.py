"""The pair images of the int8 residual list scan built INSIDE the plan's launches (option h8_pairs_plan = 1, the default: extra
workgroups of the histogram and scatter launches of the three-launch plan find the surviving pairs by a sweep over the probe words --
ivf_hist_pairs_kernel, ivf_scatter_pairs_kernel) against the stand-alone launch after the plan (h8_pairs_plan = 0:
h8_pairs_wave_kernel over the plan's pair list).  The same search run with both must leave the same candidate counts, the same
sorted approximate keys and the same per-query bounds BIT FOR BIT, and both must return the oracle's ids and distances.  Every run
asserts from the profile families which form ran: `ivf_prep_pairs` is recorded by the stand-alone launch alone.

Shapes: n = 4096 rows in 8 lists, h16_form = 3, h8_pairs = 2 and plan_fused = 0, so that a batch of a few hundred probe words takes
the wavefront-per-pair form and the three-launch plan.  d = 100 (a padded last chunk, one held piece per lane), 768 (48 of 64 lanes
own a piece, one held piece), 1100 (72 pieces: two held pieces), 2100 once (pieces loaded a second time)."""
import numpy as np
import pytest

import myscaledb_amd.capi as capi
from test_i8r_pair_images import CAP, DIMS, K, N, NLIST, i8r_index, knobs, lists_of_keys
from test_i8r_shadow import blobs, i8r_bound, last_keys, oracle, same
from test_scan_item_table import NLIST as T_NLIST
from test_scan_item_table import index_and_queries, item_tables
from test_scan_item_table import knobs as table_knobs


def scan(ix, q, d, nprobe, opt, plan, grid=None, split=None, forced=True, tables=False):
    """One search with the pairs built in the plan's launches (plan = "1" / None: the default) or after them ("0")."""
    if forced:
        opt("h8_pairs", "2")
        opt("plan_fused", "0")
    opt("h8_pairs_plan", plan)
    opt("h8_pairs_grid", grid)
    opt("h8_pairs_split", split)
    capi.profile_reset()
    capi.profile_enable(True)
    try:
        ids, dis = ix.search(q, K, "nprobe=%d" % nprobe)
    finally:
        capi.profile_enable(False)
    alone, plans = capi.profile_get("ivf_prep_pairs")[0], capi.profile_get("ivf_plan")[0]
    capi.profile_reset()
    assert plans >= 1, "no plan was launched"
    if plan == "0":
        assert alone >= 1, "h8_pairs_plan = 0 did not take the stand-alone pair launch"
    else:
        assert alone == 0, "the stand-alone pair launch ran although the plan's launches carry the pairs"
    tab = item_tables() if tables else None  # (before the bound and the keys: reading those retires the record of the pass)
    bound, _ = i8r_bound(d, len(q))
    keys, cnt = last_keys(len(q), CAP)
    for qi in range(len(q)):
        keys[qi, : cnt[qi]].sort()
        keys[qi, cnt[qi]:] = 0
    return ids, dis, keys, cnt, bound, tab


def equal(old, new, what):
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1].view(np.uint32), new[1].view(np.uint32)), "results differ (%s)" % what
    assert np.array_equal(old[3], new[3]), "candidate counts differ (%s)" % what
    assert np.array_equal(old[2], new[2]), "approximate keys differ (%s)" % what
    assert np.array_equal(old[4].view(np.uint64), new[4].view(np.uint64)), "per-query bounds differ (%s)" % what


def check(ix, q, d, nprobe, opt, grids=(None,), splits=(None,), forced=True):
    """h8_pairs_plan = 0 against the two-role launches, once per (grid, split): everything bit for bit, results = the oracle's."""
    oi, od, _ = oracle(ix, q, nprobe, K)
    old = scan(ix, q, d, nprobe, opt, "0", forced=forced)
    same(old[0], old[1], oi, od)
    for grid in grids:
        for split in splits:
            new = scan(ix, q, d, nprobe, opt, "1" if forced else None, grid, split, forced=forced)
            same(new[0], new[1], oi, od)
            equal(old, new, "grid %s, split %s" % (grid, split))
    return old


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS + [2100])
def test_every_pair_survives(d, opt):
    """No pruning: 64 x 8 = 512 probe words, every one a pair, eight per query through the atomics; a chunk of the sweep is 24 words
    (three queries' worth), six pairs for each wavefront of its workgroup.  The default grid has a workgroup per chunk; a grid of 3
    workgroups and of 1 walk the 11 chunks of either launch's share in several rounds of the stride loop, the last chunk short."""
    rng = np.random.default_rng(d)
    x, q = blobs(rng, NLIST, N, 64, d)
    ix = i8r_index(x, opt)
    knobs(opt, prune=False)
    old = check(ix, q, d, NLIST, opt, grids=(None, "1", "3"))
    assert (old[3] == N).all(), "every row of every list is a candidate"
    assert np.isfinite(old[4]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_pre_pruning_leaves_one_to_three_pairs(d, opt):
    """Default pruning, the geometry of test_i8r_pair_images' test of this name: most probe words are -1 when the sweep reads them,
    the queries keep one pair (blobs 5, 6, 7) or two or three (blobs 0, 1 and 2, 3, 4)."""
    rng = np.random.default_rng(1000 + d)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    for l in (1, 3, 4):
        cents[l] = cents[l - 1] + 0.15 * rng.standard_normal(d, dtype=np.float32)
    x = (cents[rng.integers(0, NLIST, N)] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    q = (cents[np.arange(64) % NLIST] + 0.3 * rng.standard_normal((64, d), dtype=np.float32)).astype(np.float32)
    ix = i8r_index(x, opt, centroids=cents)
    knobs(opt, prune=True)
    old = check(ix, q, d, NLIST, opt)
    npairs = lists_of_keys(ix, old[2], old[3])
    print("pairs per query:", npairs.tolist())
    assert (npairs == 1).sum() >= 16, "queries with exactly one pair"
    assert ((npairs == 2) | (npairs == 3)).sum() >= 16, "queries with two or three pairs"
    assert (npairs <= 3).all(), "the pre-pruning dropped the far lists of every query"
    # the second pruning stage forced: a second plan (without a pair role) follows the sample launch
    opt("h16_prune", "2")
    opt("rerank_stats", "1")
    s0 = capi.debug_prune_stats()
    check(ix, q, d, NLIST, opt)
    assert capi.debug_prune_stats()[1] > s0[1], "the second pruning stage did not run"


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [5, 63, 64, 65])
@pytest.mark.parametrize("d", [100, 1100])
def test_split_between_the_two_launches(d, nq, opt):
    """The histogram launch takes the queries below the split, the scatter launch the rest: the default (nq / 2: 2 | 3, 31 | 32,
    32 | 32, 32 | 33 queries -- shares that are no multiple of the three queries of a chunk: a short last chunk, a chunk of one query),
    0 (everything beside the scatter, the histogram launch is the plan's own kernel) and nq (the reverse)."""
    rng = np.random.default_rng(5000 + d)
    x, q = blobs(rng, NLIST, N, 65, d)
    ix = i8r_index(x, opt)
    knobs(opt, prune=False)
    check(ix, q[:nq], d, NLIST, opt, splits=(None, "0", str(nq), "1"))


@pytest.mark.gpu
@pytest.mark.parametrize("far", [3.0, 50.0])
@pytest.mark.parametrize("d", DIMS)
def test_empty_list_among_the_probed(d, far, opt):
    """One centroid far from every row: its list is empty and the plan drops its pairs; the sweep takes them like every other word
    with l >= 0, once.  Their C_p is 0 (far = 3) or +inf (far = 50: |r_q| / |q| leaves the model) in every query's minimum / maximum."""
    rng = np.random.default_rng(4000 + d)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    x = (cents[rng.integers(0, NLIST - 1, N)] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    q = (cents[rng.integers(0, NLIST - 1, 24)] + 0.3 * rng.standard_normal((24, d), dtype=np.float32)).astype(np.float32)
    cents[NLIST - 1] = far * rng.standard_normal(d, dtype=np.float32)
    ix = i8r_index(x, opt, centroids=cents)
    off = np.asarray(ix.export()[1], np.int64)
    assert off[NLIST] - off[NLIST - 1] == 0, "the far centroid's list is empty"
    knobs(opt, prune=False)
    old = check(ix, q, d, NLIST, opt)
    assert (np.isinf(old[4]) == (far == 50.0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_degenerate_queries_among_normal_ones(d, opt):
    """A query equal to a centroid, an all-zero query, a tiny one and one 50 times farther out than the rows share a batch with
    normal ones: the bound is +inf exactly where the stand-alone launch says so."""
    rng = np.random.default_rng(3000 + d)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    x = (cents[rng.integers(0, NLIST, N)] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    q = (cents[rng.integers(0, NLIST, 16)] + 0.3 * rng.standard_normal((16, d), dtype=np.float32)).astype(np.float32)
    q[2] = cents[4]
    q[5] = 0.0
    q[9] = 1e-3 * rng.standard_normal(d, dtype=np.float32)
    q[12] = 50.0 * q[12]
    ix = i8r_index(x, opt, centroids=cents)
    knobs(opt, prune=False)
    old = check(ix, q, d, NLIST, opt)
    inf = np.isinf(old[4])
    assert inf[5] and inf[9], "queries outside the model's range"
    normal = np.ones(16, bool)
    normal[[5, 9, 12]] = False
    assert np.isfinite(old[4][normal]).all()


@pytest.mark.gpu
def test_default_options_on_a_batch_past_the_threshold(opt):
    """1100 queries x 8 probes = 8800 probe words, default pruning: past the fused plan's limit and the pair kernel's threshold, so
    the DEFAULTS (h8_pairs, plan_fused, h8_pairs_plan, grid and split unset) must choose the two-role launches -- scan() asserts it
    from the profile.  Forced: the index's shadow form, and what routes this small index to the shadow list scan and sizes the
    buffer its keys are read from (ivf_pass, cand_cap)."""
    d = 100
    rng = np.random.default_rng(77)
    x, q = blobs(rng, NLIST, N, 1100, d)
    ix = i8r_index(x, opt)
    opt("ivf_pass", "2")
    opt("cand_cap", "16384")
    check(ix, q, d, NLIST, opt, forced=False)


@pytest.mark.gpu
def test_scatter_launch_with_pair_workgroups_writes_the_same_item_tables(opt):
    """test_scan_item_table's index (lists of 0, 20, 33, 64, 65, 1000, 1414 and 1500 rows), 64 queries probing every list, d = 768,
    h16_items = 1 under the three-launch plan: the scatter launch writes the item tables with a grid-stride loop over the lists, which
    must see the plan's workgroups alone when pair workgroups share its grid -- the same record counts, every record fits the plan
    (msvs_debug_h16_items), and the scans that read the tables leave the same keys."""
    d, nq = 768, 64
    ix, q = index_and_queries(d, "3", capi.METRIC_L2, opt)
    table_knobs(opt)
    opt("h16_items", "1")
    oi, od, _ = oracle(ix, q[:nq], T_NLIST, K)
    old = scan(ix, q[:nq], d, T_NLIST, opt, "0", tables=True)
    new = scan(ix, q[:nq], d, T_NLIST, opt, "1", tables=True)
    same(old[0], old[1], oi, od)
    same(new[0], new[1], oi, od)
    equal(old, new, "item tables")
    for t in (old[5], new[5]):
        assert t["main"][0] == 1 and t["main"][2] <= t["main"][1] and t["main_misfits"] == 0, t
        assert t["sample"][0] == 1 and t["sample"][2] <= t["sample"][1] and t["sample_misfits"] == 0, t
    assert old[5] == new[5], "the tables differ: %s against %s" % (old[5], new[5])
    assert new[5]["main"][2] > 0 and new[5]["sample"][2] > 0
