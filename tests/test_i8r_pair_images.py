"""The pair images of the int8 residual list scan by one wavefront per surviving pair (h8_pairs_wave_kernel, the default) against
the workgroup-per-query kernel (h8_prep_pairs_kernel, option h8_pairs = 0; small batches keep it by default, h8_pairs = 2 forces
the new kernel at any size): the same search run with both must leave
the same approximate keys, the same counts and the same per-query bound BIT FOR BIT -- images, the pairs' constants after their
offset, qbound -- and both must return the oracle's ids and distances.

Shapes are the smallest that reach every path: n = 4096 rows in 8 lists; d = 100 (a padded last chunk), 768 (48 of 64 lanes hold a
piece), 1100 (72 pieces per pair: the second piece of a lane, up to d = 2048 still held in registers) -- and d = 2100 once, where
the pieces past the held ones are loaded a second time."""
import numpy as np
import pytest

from test_i8r_shadow import blobs, build_ivf, i8r_bound, last_keys, oracle, same, shadow_form

DIMS = [100, 768, 1100]
N, NLIST, K = 4096, 8, 10
CAP = 8192


def scan(ix, q, d, nprobe, opt, pairs, grid=None):
    """One search with the given pair kernel; what it returned and what its kernels left behind."""
    opt("h8_pairs", pairs)
    opt("h8_pairs_grid", grid)
    ids, dis = ix.search(q, K, "nprobe=%d" % nprobe)
    bound, _ = i8r_bound(d, len(q))  # (before the keys: reading them retires the record of the pass)
    keys, cnt = last_keys(len(q), CAP)
    for qi in range(len(q)):
        keys[qi, : cnt[qi]].sort()
        keys[qi, cnt[qi]:] = 0
    return ids, dis, keys, cnt, bound


def check_pair(ix, q, d, nprobe, opt, grids=(None,), new_form="2"):
    """h8_pairs = 0 against the wavefront-per-pair kernel (once per grid): keys, counts and bounds bit for bit, results = the
    oracle's."""
    oi, od, _ = oracle(ix, q, nprobe, K)
    old = scan(ix, q, d, nprobe, opt, "0")
    same(old[0], old[1], oi, od)
    for grid in grids:
        new = scan(ix, q, d, nprobe, opt, new_form, grid)
        same(new[0], new[1], oi, od)
        assert np.array_equal(old[3], new[3]), "candidate counts differ (grid %s)" % grid
        assert np.array_equal(old[2], new[2]), "approximate keys differ (grid %s)" % grid
        assert np.array_equal(old[4].view(np.uint64), new[4].view(np.uint64)), "per-query bounds differ (grid %s)" % grid
    return old


def knobs(opt, prune):
    opt("ivf_pass", "2")
    opt("h16_nocut", "1")
    opt("cand_cap", "16384")
    if not prune:
        opt("h16_preprune", "0")
        opt("h16_prune", "0")


def i8r_index(x, opt, centroids=None):
    opt("h16_form", "3")
    ix = build_ivf(x, NLIST, centroids=centroids)
    assert shadow_form(ix) == 3
    return ix


def lists_of_keys(ix, keys, cnt):
    """Per query the number of lists its keys' rows sit in: the pairs that reached the sample launch."""
    off = np.asarray(ix.export()[1], np.int64)
    out = []
    for qi in range(len(cnt)):
        pos = (keys[qi, : cnt[qi]] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        out.append(len(np.unique(np.searchsorted(off, pos, side="right"))))
    return np.array(out)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS + [2100, 2432])
def test_every_pair_survives(d, opt):
    """No pruning: 64 x 8 = 512 pairs, eight per query through the atomics.  A grid of 8 workgroups (32 wavefronts) walks them in 16
    rounds of its grid-stride loop; the default grid has more wavefronts than pairs.  d = 2432 (19 chunks a pair, 152 pieces): the
    largest dimension the i8r list scan serves."""
    rng = np.random.default_rng(d)
    x, q = blobs(rng, NLIST, N, 64, d)
    ix = i8r_index(x, opt)
    knobs(opt, prune=False)
    old = check_pair(ix, q, d, NLIST, opt, grids=(None, "8", "1"))
    assert (old[3] == N).all(), "every row of every list is a candidate"
    assert np.isfinite(old[4]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_pre_pruning_leaves_one_to_three_pairs(d, opt):
    """Default pruning: most probes are -1 when the pair kernel runs.  Blobs 5, 6, 7 stand alone: their queries keep one pair
    (minimum = maximum, no offset).  The centres of blobs 0, 1 and of blobs 2, 3, 4 lie half a blob radius apart: a query of such a
    blob keeps the two or three lists of its group, whose offsets and bound meet through the atomics; every other list is far
    beyond the pre-pruning's bound."""
    rng = np.random.default_rng(1000 + d)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    for l in (1, 3, 4):
        cents[l] = cents[l - 1] + 0.15 * rng.standard_normal(d, dtype=np.float32)
    x = (cents[rng.integers(0, NLIST, N)] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    q = (cents[np.arange(64) % NLIST] + 0.3 * rng.standard_normal((64, d), dtype=np.float32)).astype(np.float32)
    ix = i8r_index(x, opt, centroids=cents)
    knobs(opt, prune=True)
    old = check_pair(ix, q, d, NLIST, opt)
    npairs = lists_of_keys(ix, old[2], old[3])
    print("pairs per query:", npairs.tolist())
    assert (npairs == 1).sum() >= 16, "queries with exactly one pair"
    assert ((npairs == 2) | (npairs == 3)).sum() >= 16, "queries with two or three pairs"
    assert (npairs <= 3).all(), "the pre-pruning dropped the far lists of every query"


@pytest.mark.gpu
def test_default_options_on_a_batch_past_the_threshold(opt):
    """1100 queries x 8 probes = 8800 probe words: the default (h8_pairs unset) takes the wavefront-per-pair kernel there; default
    pruning, so the grid-stride loop and the sweep over the probe words both run over thousands of entries."""
    d = 100
    rng = np.random.default_rng(77)
    x, q = blobs(rng, NLIST, N, 1100, d)
    ix = i8r_index(x, opt)
    knobs(opt, prune=True)
    check_pair(ix, q, d, NLIST, opt, new_form=None)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_five_queries(d, opt):
    """nq = 5: not a multiple of the four wavefronts of a workgroup, 40 pairs in a grid of thousands of wavefronts."""
    rng = np.random.default_rng(2000 + d)
    x, q = blobs(rng, NLIST, N, 5, d)
    ix = i8r_index(x, opt)
    knobs(opt, prune=False)
    check_pair(ix, q, d, NLIST, opt, grids=(None, "3"))
    knobs(opt, prune=True)
    opt("h16_preprune", None)
    opt("h16_prune", None)
    check_pair(ix, q, d, NLIST, opt)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_degenerate_queries_among_normal_ones(d, opt):
    """In one batch: a query equal to a centroid (s_q = 0 for that pair), an all-zero query (|q| = 0: no pair is inside the model), a
    query so small that |r_q| / |q| is beyond the model's limit, a query 50 times farther out than the rows.  The bound is +inf
    exactly where the old kernel says so; the canonical fallback serves those queries."""
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
    old = check_pair(ix, q, d, NLIST, opt)
    inf = np.isinf(old[4])
    assert inf[5] and inf[9], "queries outside the model's range"
    normal = np.ones(16, bool)
    normal[[5, 9, 12]] = False
    assert np.isfinite(old[4][normal]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("far", [3.0, 50.0])
@pytest.mark.parametrize("d", DIMS)
def test_empty_list_among_the_probed(d, far, opt):
    """One centroid far from every row: its list is empty, the plan drops its pairs, and the old kernel still counts their C_p (0: no
    row contributes an alpha or beta; +inf at far = 50, where |r_q| / |q| leaves the model) in every query's minimum and maximum.  The
    new kernel finds those pairs in the probe words."""
    rng = np.random.default_rng(4000 + d)
    cents = rng.standard_normal((NLIST, d), dtype=np.float32)
    x = (cents[rng.integers(0, NLIST - 1, N)] + 0.3 * rng.standard_normal((N, d), dtype=np.float32)).astype(np.float32)
    q = (cents[rng.integers(0, NLIST - 1, 24)] + 0.3 * rng.standard_normal((24, d), dtype=np.float32)).astype(np.float32)
    cents[NLIST - 1] = far * rng.standard_normal(d, dtype=np.float32)
    ix = i8r_index(x, opt, centroids=cents)
    off = np.asarray(ix.export()[1], np.int64)
    assert off[NLIST] - off[NLIST - 1] == 0, "the far centroid's list is empty"
    knobs(opt, prune=False)
    old = check_pair(ix, q, d, NLIST, opt)
    assert (np.isinf(old[4]) == (far == 50.0)).all()
