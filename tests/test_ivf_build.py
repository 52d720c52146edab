"""The build feed of the partitioned float indexes (ivf_build_kernels.hpp, msvs_index_train / add / build) against a numpy reference in
int64 / float64 (ivf_build_ref.py): which list every row goes to, what the seeds are, what one and two Lloyd steps give, that device
memory and host memory build the same index, and that a cancelled build stops with ERR_ABORTED.  The list-scan parity tests compare
a search with an oracle on the EXPORTED structure; a row in the wrong list is invisible to them."""
import numpy as np
import pytest

import ivf_build_ref as R
import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
SEED = 77


def chunks(n):
    """add() calls that cross the assignment kernel's 128-row tile"""
    return [(a, min(b, n)) for a, b in ((0, 127), (127, 128), (128, n)) if a < min(b, n)]


def ivf_lists(metric, cent, x):
    """IVFFLAT index over given centroids -> (list of every row, rows as stored in id order)"""
    n, d = x.shape
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, d, "ncentroids=%d" % cent.shape[0])
    ix.set_centroids(cent)
    for a, b in chunks(n):
        ix.add(x[a:b])
    ix.build()
    c, off, vecs, ids = ix.export()
    ix.close()
    assert (c.view(np.uint32) == np.asarray(cent, np.float32).view(np.uint32)).all()
    stored = np.empty_like(vecs)
    stored[ids] = vecs
    return R.lists_of_ids(off, ids, n), stored


# ---------------------------------------------------------------------------------------- 1. exact assignment on integer data

EXACT = [(1, 1, 1), (2, 3, 127), (2, 16, 1), (127, 16, 129), (128, 17, 300), (128, 20, 129), (129, 20, 300), (129, 100, 1),
         (257, 3, 300), (257, 100, 300), (300, 1, 127), (300, 17, 129), (300, 100, 300)]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nlist,d,n", EXACT)
def test_exact_assignment(metric, nlist, d, n):
    rng = np.random.default_rng(1000 * nlist + 10 * d + n)
    cent = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    want = R.exact_assign(x, cent, metric == IP)
    got, stored = ivf_lists(metric, cent, x)
    assert (stored == x).all()
    R.check_exact(got, want)


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("nlist,copies", [(130, (69, 129)), (257, (69, 133, 200))])
def test_ties_go_to_the_lowest_centroid(metric, nlist, copies):
    """d = 3 with components in [-2, 2]: 125 distinct points for 130 or more centroids, so most rows tie for the minimum.  Centroid 5
    is repeated in the other half of its tile (69: the other pair of wavefronts) and beyond the tile boundary (129, 133, 200)."""
    rng = np.random.default_rng(nlist)
    n, d = 300, 3
    cent = rng.integers(-2, 3, (nlist, d)).astype(np.float32)
    cent[5] = (2, -2, 2)
    cent[:5] = rng.integers(-1, 2, (5, d))  # nothing below 5 equals it
    for j in copies:
        cent[j] = cent[5]
    x = rng.integers(-2, 3, (n, d)).astype(np.float32)
    x[::7] = cent[5]
    s = R.int_scores(x, cent, metric == IP)
    want = np.argmin(s, axis=1)
    tied = (s == s.min(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied.mean() > 0.4 and (want == 5).sum() >= 10 and tied[want == 5].all()
    got, _ = ivf_lists(metric, cent, x)
    R.check_exact(got, want)


@pytest.mark.parametrize("metric", [L2, IP])
def test_nan_and_overflowing_rows_go_to_list_0_and_a_nan_centroid_gets_nothing(metric):
    rng = np.random.default_rng(5)
    n, d, nlist = 300, 20, 129
    cent = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
    cent[:, 0] = rng.integers(-8, -1, nlist)  # <= -2: the product with 3e38 overflows to -inf, every score of that row is +inf
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    x[10:15] = cent[7]  # rows that centroid 7 would win ...
    clean = cent.copy()
    cent[7, 3] = np.nan  # ... if it were a number
    special = [5, 70, 127, 128, 200]
    x[5, 2] = np.nan
    x[200] = np.nan
    for r in (70, 127, 128):
        x[r] = 0
        x[r, 0] = 3e38
    x[128, 0] = np.inf
    assert (R.exact_assign(x[10:15], clean, metric == IP) == 7).all()
    ok = np.ones(n, bool)
    ok[special] = False
    want = np.zeros(n, np.int64)
    want[ok] = R.exact_assign(x[ok], cent, metric == IP)
    assert (want != 7).all() and (want[ok] != 0).any()
    got, _ = ivf_lists(metric, cent, x)
    R.check_exact(got, want)


@pytest.mark.parametrize("metric", [L2, IP])
def test_exact_assignment_of_the_sq_and_pq_indexes(metric):
    rng = np.random.default_rng(6)
    n, nlist = 300, 129
    for kind, d in (("sq", 17), ("pq", 20)):
        cent = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
        x = rng.integers(-8, 9, (n, d)).astype(np.float32)
        if kind == "sq":
            ix = capi.SqIndex(metric, d, "ncentroids=%d" % nlist)
            ix.set_codebook(cent, np.full(d, -20, np.float32), np.full(d, 20, np.float32))
        else:
            ix = capi.PqIndex(metric, d, "ncentroids=%d,m=5" % nlist)
            ix.set_codebook(cent, rng.integers(-4, 5, (5, 256, d // 5)).astype(np.float32))
        for a, b in chunks(n):
            ix.add(x[a:b])
        ix.build()
        exp = ix.export()
        ix.close()
        off, labels = (exp[3], exp[5]) if kind == "sq" else (exp[2], exp[4])
        R.check_exact(R.lists_of_ids(off, labels, n), R.exact_assign(x, cent, metric == IP))


# ---------------------------------------------------------------------------------------- 2. float data: the ambiguity rule

@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("n,d,nlist", [(1500, 20, 129), (1500, 100, 257), (1500, 17, 300), (1500, 3, 130)])
def test_float_assignment_within_the_error_bound(metric, n, d, nlist):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, d), dtype=np.float32)
    cent = rng.standard_normal((nlist, d), dtype=np.float32)
    got, stored = ivf_lists(metric, cent, x)
    if metric != COS:
        assert (stored == x).all()
    # (cosine: the rows as the index normalised them, so that the normalisation is not part of the comparison)
    R.check_float_assign(got, stored, cent, metric != L2)


# ---------------------------------------------------------------------------------------- 3. training

def trained(metric, x, nlist, iters, seed=SEED, extra=""):
    """train on all rows, add them, build -> (centroids, stored rows in id order, list of every row, the index)"""
    n, d = x.shape
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, d, "ncentroids=%d,kmeans_iters=%d,train_sample=%d,seed=%d%s" % (nlist, iters, n, seed, extra))
    ix.train(x)
    ix.add(x)
    ix.build()
    cent, off, vecs, ids = ix.export()
    stored = np.empty_like(vecs)
    stored[ids] = vecs
    return cent, stored, R.lists_of_ids(off, ids, n), ix


TRAIN = [(600, 20, 130, 8), (900, 17, 257, 8), (400, 3, 130, 30), (300, 100, 129, 8)]


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("n,d,nlist,amp", TRAIN)
def test_seeds_and_two_lloyd_steps_by_hand(metric, n, d, nlist, amp):
    """kmeans_iters = 0: the seeds are the first nlist rows of the seeded sample.  1: the means of the exact assignment to the seeds,
    with the kernel's two roundings, to the bit.  2: the same from those centroids, for every cluster no ambiguous row can reach.
    (ns / nlist / 16 == 0 here, so no cluster counts as tiny; forced splits need more than two iterations.)  Cosine trains on the
    normalised rows: their sums are not exact, so the reference adds them in f32 in the kernel's order, the sample's
    (R.train_sample), and the comparison stays bit equality.  A tolerance of (m + 2) 2^-24 relative to each mean would not do: where
    the members' components cancel, a correct f32 sum misses it (by a factor of up to 334 on these inputs in numpy)."""
    x = R.int_rows(np.random.default_rng(1), n, d, -amp, amp)
    c0, stored, _, ix = trained(metric, x, nlist, 0)
    ix.close()
    if metric != COS:
        assert (stored == x).all()
    # the seeds: nlist distinct rows of the input, the same for the same seed, others for another
    have = {r.tobytes(): i for i, r in enumerate(stored)}
    picks = [have.get(c.tobytes(), -1) for c in c0]
    assert min(picks) >= 0 and len(set(picks)) == nlist
    again, _, _, ix = trained(metric, x, nlist, 0)
    ix.close()
    R.check_bit_equal(again, c0)
    other, _, _, ix = trained(metric, x, nlist, 0, seed=SEED + 1)
    ix.close()
    assert (other != c0).any()
    xs = stored[R.train_sample(n, n, SEED)]  # the sample in the trainer's order
    R.check_bit_equal(c0, xs[:nlist])
    # one step
    want1, cnt1, touched1 = R.lloyd_step(xs, c0)
    assert (cnt1 > 0).all()  # no empty cluster: the re-seeding does not interfere
    assert touched1.mean() <= 0.05
    c1, _, _, ix = trained(metric, x, nlist, 1)
    ix.close()
    R.check_bit_equal(c1, want1, rows=~touched1)
    if touched1.any():
        return  # (cosine only, and not at these inputs: the second step has no pinned start then)
    # two steps
    want2, cnt2, touched2 = R.lloyd_step(xs, want1)
    assert (cnt2 > 0).all()
    assert touched2.mean() <= 0.05
    c2, stored2, lists, ix = trained(metric, x, nlist, 2)
    ix.close()
    R.check_bit_equal(c2, want2, rows=~touched2)
    # and the rows of the built index sit in the lists of those centroids (by the index's own metric)
    R.check_float_assign(lists, stored2, c2, metric != L2)


def test_reseeding_of_empty_clusters():
    """40 distinct points, 25 copies of each, 64 centroids: the seeds repeat points, so clusters come out empty and are re-seeded by
    splitting a populated one (both copies moved apart by a relative 1/1024 per component).  At most nlist - 40 = 24 splits stack."""
    rng = np.random.default_rng(3)
    d, nlist = 16, 64
    pts = R.int_rows(rng, 40, d, -50, 50)
    gap = np.sqrt(((pts[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(-1) + 1e18 * np.eye(40)).min()
    assert gap > 40  # well separated: the 24 stacked splits move a centroid by less than 0.024 * 50 * sqrt(16) = 4.8
    x = np.repeat(pts, 25, axis=0)[rng.permutation(1000)]
    c, _, _, ix = trained(L2, x, nlist, 3)
    c_again, _, _, ix2 = trained(L2, x, nlist, 3)
    ix2.close()
    assert np.isfinite(c).all()
    R.check_bit_equal(c_again, c)
    near = np.argmin(((c[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(-1), axis=1)
    assert set(near.tolist()) == set(range(40))
    tol = (1 + 1 / 1024) ** (nlist - 40) - 1
    assert (np.abs(c.astype(np.float64) - pts[near]) <= tol * np.abs(pts[near])).all()
    q = np.concatenate([pts[:5], rng.integers(-50, 51, (4, d)).astype(np.float32)])
    ids, dis = ix.search(q, 10, "nprobe=%d" % nlist)
    ix.close()
    oi, od = o.knn(q, x, 10, o.METRIC_L2)
    assert (ids == oi).all() and (dis.view(np.uint32) == od.view(np.uint32)).all()


def test_sq_and_pq_trainers_take_the_ivfflat_centroids():
    n, d, nlist = 600, 20, 130
    x = R.int_rows(np.random.default_rng(4), n, d, -8, 8)
    params = "ncentroids=%d,kmeans_iters=3,train_sample=%d,seed=%d" % (nlist, n, SEED)
    want, _, _, ix = trained(L2, x, nlist, 3)
    ix.close()
    sq = capi.SqIndex(L2, d, params)
    sq.train(x)
    R.check_bit_equal(sq.export(with_lists=False)[0], want)
    sq.close()
    pq = capi.PqIndex(L2, d, params + ",m=5")
    pq.train(x)
    R.check_bit_equal(pq.export(with_lists=False)[0], want)
    pq.close()


# ---------------------------------------------------------------------------------------- 4. device memory == host memory

@pytest.mark.parametrize("d", [20, 17])  # ld == d: rows gathered on the device; ld != d: copied back and gathered on the host
def test_train_and_add_from_device_memory_equal_host(d):
    import torch
    n, nlist = 600, 130
    x = np.random.default_rng(d).standard_normal((n, d), dtype=np.float32)
    params = "ncentroids=%d,kmeans_iters=3,seed=%d" % (nlist, SEED)
    host = capi.Index(capi.INDEX_IVFFLAT, L2, d, params)
    host.train(x)
    host.add(x[:400])
    host.add(x[400:])
    host.build()
    t = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    dev = capi.Index(capi.INDEX_IVFFLAT, L2, d, params)
    dev.train(t.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    dev.add(t[:400].data_ptr(), n=400, mem=capi.MEM_DEVICE)
    dev.add(t[400:].data_ptr(), n=n - 400, mem=capi.MEM_DEVICE)
    dev.build()
    for a, b in zip(host.export(), dev.export()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    host.close()
    dev.close()


# ---------------------------------------------------------------------------------------- 5. cancellation

def from_call(k):
    """a callback that says 'cancelled' from its k-th call on"""
    calls = [0]

    def fn():
        calls[0] += 1
        return calls[0] >= k

    return fn


def code_of(fn):
    with pytest.raises(capi.MsvsError) as e:
        fn()
    return e.value.code


def test_cancelled_training_leaves_an_untrained_index():
    n, d, nlist, iters = 600, 20, 64, 5
    x = np.random.default_rng(8).standard_normal((n, d), dtype=np.float32)
    want, _, _, ix = trained(L2, x, nlist, iters)
    ix.close()
    params = "ncentroids=%d,kmeans_iters=%d,train_sample=%d,seed=%d" % (nlist, iters, n, SEED)
    for k in (1, 3, iters):  # the first, a middle and the last iteration
        ix = capi.Index(capi.INDEX_IVFFLAT, L2, d, params)
        ix.set_cancel(from_call(k))
        assert code_of(lambda: ix.train(x)) == capi.ERR_ABORTED == 236
        ix.set_cancel(None)
        assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # untrained again
        ix.train(x)
        ix.add(x)
        ix.build()
        R.check_bit_equal(ix.export()[0], want)
        ix.close()


def test_cancelled_add_and_build():
    n, d, nlist = 600, 20, 64
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((7, d), dtype=np.float32)
    oi, od = o.knn(q, x, 10, o.METRIC_L2)
    params = "ncentroids=%d,kmeans_iters=2" % nlist
    # a cancelled add, and the index freed as it stands
    ix = capi.Index(capi.INDEX_IVFFLAT, L2, d, params)
    ix.train(x)
    ix.add(x[:300])
    ix.set_cancel(from_call(1))
    assert code_of(lambda: ix.add(x[300:])) == capi.ERR_ABORTED
    ix.close()
    # a cancelled add and a cancelled build, then the build goes on where it stopped
    ix = capi.Index(capi.INDEX_IVFFLAT, L2, d, params)
    ix.train(x)
    ix.add(x[:300])
    ix.set_cancel(from_call(1))
    assert code_of(lambda: ix.add(x[300:])) == capi.ERR_ABORTED
    ix.set_cancel(from_call(2))
    ix.add(x[300:])
    assert code_of(ix.build) == capi.ERR_ABORTED
    assert not ix.ready
    ix.set_cancel(None)
    ix.build()
    assert ix.ready and ix.num_data == n
    ids, dis = ix.search(q, 10, "nprobe=%d" % nlist)
    assert (ids == oi).all() and (dis.view(np.uint32) == od.view(np.uint32)).all()
    ix.close()
