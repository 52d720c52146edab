"""The IVFSQ index (msvs_sq_index_*, capi.SqIndex): 8-bit residual codes only, searched with the canonical arithmetic.

The reference is composed here from the semantics in include/msvs.h alone: a numpy encode / decode (every step rounded to f32),
the rows' lists from the export, X^ = decode(exported codes), oracle.ivf_search over X^.  Every comparison is == on ids and on
the uint32 view of the distances."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
FLT_MAX = np.finfo(np.float32).max
NLIST = 8


def step_of(vmin, vmax):
    return ((vmax - vmin).astype(F) / F(255)).astype(F)


def encode(x, c, vmin, vmax):
    """x: stored rows, c: the centroid of each row's list"""
    step = step_of(vmin, vmax)
    r = (x - c).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((r - vmin).astype(F) / step).astype(F)
    code = np.clip(np.rint(t), 0, 255)
    code[:, step == 0] = 0
    return code.astype(np.uint8)


def decode(codes, c, vmin, vmax):
    step = step_of(vmin, vmax)
    return (c + (vmin + (codes.astype(F) * step).astype(F)).astype(F)).astype(F)


def stored(x, metric):
    return o.normalize_rows(x) if metric == COS else np.ascontiguousarray(x, F)


def lists_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def decoded(exp):
    cent, lo, hi, off, codes, labels = exp
    return decode(codes, cent[lists_of(off)], lo, hi)


def ref_search(exp, xh, q, nprobe, k, metric, alive=None):
    cent, lo, hi, off, codes, labels = exp
    if metric == COS:
        oi, od, _ = o.ivf_search(cent, off, xh, labels, o.normalize_rows(q), nprobe, k, o.METRIC_IP, alive=alive)
        return oi, (F(1) - od).astype(F)
    oi, od, _ = o.ivf_search(cent, off, xh, labels, q, nprobe, k, o.METRIC_L2 if metric == L2 else o.METRIC_IP, alive=alive)
    return oi, od


def same(got, exp):
    (gi, gd), (ei, ed) = got, exp
    assert gi.shape == ei.shape
    assert (gi == ei).all(), np.argwhere(gi != ei)[:5]
    assert (gd.view(np.uint32) == ed.view(np.uint32)).all(), np.argwhere(gd.view(np.uint32) != ed.view(np.uint32))[:5]


def device_search(ix, q, k, nprobe, alive=None):
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    di = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    dd = torch.empty((len(q), k), device=dev, dtype=torch.float32)
    bits, nbits = 0, 0
    if alive is not None:
        db = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).to(dev)
        bits, nbits = db.data_ptr(), len(alive)
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream, d_alive=bits,
                     nbits=nbits)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


def blobs(rng, n, d, ncentres, sigma=0.3):
    centres = rng.standard_normal((ncentres, d), dtype=F)
    x = (centres[rng.integers(0, ncentres, n)] + F(sigma) * rng.standard_normal((n, d), dtype=F)).astype(F)
    return centres, x


@functools.lru_cache(maxsize=None)
def case(metric, dim, data):
    """A trained and built index of 3000 rows in three chunks, its export, the decoded matrix and 300 queries; computed once."""
    rng = np.random.default_rng(dim * 13 + metric * 5 + len(data))
    n = 3000
    centres, x = blobs(rng, n, dim, NLIST)
    if data == "ties":  # 40 distinct vectors: equal distances everywhere, ordered by label
        x = np.ascontiguousarray(x[:40][rng.integers(0, 40, n)])
    labels = rng.permutation(3 * n)[:n].astype(np.int64)  # shuffled, not contiguous
    q = (centres[rng.integers(0, NLIST, 300)] + F(0.3) * rng.standard_normal((300, dim), dtype=F)).astype(F)
    ix = capi.SqIndex(metric, dim, "ncentroids=%d,kmeans_iters=4" % NLIST)
    ix.train(x)
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        ix.add(x[a:b], labels[a:b])
    ix.build()
    exp = ix.export()
    return ix, exp, decoded(exp), x, labels, q


# ---------------------------------------------------------------------------------------- 1. structure and codes

@pytest.mark.parametrize("dim", [5, 64, 100, 768])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_structure_codes_and_trained_range(metric, dim):
    ix, exp, _, x, labels, _ = case(metric, dim, "clustered")
    cent, lo, hi, off, codes, elab = exp
    n = len(x)
    assert ix.ready and ix.num_data == n and ix.num_lists == NLIST
    assert len(off) == NLIST + 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert sorted(elab.tolist()) == sorted(labels.tolist())
    for l in range(NLIST):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    where = {int(l): i for i, l in enumerate(labels)}
    xs = stored(x, metric)[[where[int(l)] for l in elab]]  # the fed rows in export order
    lists = lists_of(off)
    assert (codes == encode(xs, cent[lists], lo, hi)).all()
    # the rows fed ARE the training rows: their residuals against their exported lists' centroids give the trained range
    r = (xs - cent[lists]).astype(F)
    assert (lo == r.min(axis=0)).all() and (hi == r.max(axis=0)).all()


# ---------------------------------------------------------------------------------------- 2. search parity

PARITY = [
    (L2, 5, "clustered", 1, 1, 1, "host"),
    (L2, 64, "clustered", 9, 10, 4, "device"),
    (L2, 100, "ties", 3, 100, NLIST, "host"),
    (L2, 768, "clustered", 300, 10, 4, "host"),
    (L2, 768, "clustered", 9, 256, 10 * NLIST, "device"),
    (L2, 64, "ties", 300, 256, NLIST, "host"),
    (IP, 5, "ties", 300, 10, NLIST, "device"),
    (IP, 64, "clustered", 3, 256, 4, "host"),
    (IP, 100, "clustered", 300, 100, 1, "host"),
    (IP, 768, "ties", 1, 10, 10 * NLIST, "device"),
    (COS, 5, "clustered", 9, 100, 4, "host"),
    (COS, 64, "ties", 300, 1, NLIST, "host"),
    (COS, 100, "clustered", 1, 256, 10 * NLIST, "device"),
    (COS, 768, "clustered", 3, 10, 1, "host"),
    # the two (query tile, k class) pairs of the list scan the rows above do not reach: tile 2 (< 2 pairs per list) with 64 < k <= 128,
    # and tile 8 (>= 16 pairs per list) with k > 128, where k = 256 no longer fits the tile's LDS and falls back to tile 4
    (L2, 64, "clustered", 1, 100, 4, "host"),
    (IP, 5, "ties", 16, 150, NLIST, "device"),
]


@pytest.mark.parametrize("metric,dim,data,nq,k,nprobe,entry", PARITY)
def test_search_parity(metric, dim, data, nq, k, nprobe, entry):
    ix, exp, xh, _, _, q = case(metric, dim, data)
    q = q[:nq]
    got = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else device_search(ix, q, k, nprobe)
    same(got, ref_search(exp, xh, q, nprobe, k, metric))


# ---------------------------------------------------------------------------------------- 3. edge lists

def test_empty_short_and_segmented_lists(opt):
    rng = np.random.default_rng(3)
    dim, nlist = 20, 6
    cent = np.zeros((nlist, dim), F)
    cent[:, 0] = 10.0 * np.arange(nlist)
    sizes = [1000, 3, 1, 0, 0, 50]  # two empty lists, one shorter than a 16-row step, one single row, one of many segments
    home = np.repeat(np.arange(nlist), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    labels = rng.permutation(5000)[:len(home)].astype(np.int64)
    ix = capi.SqIndex(L2, dim)
    ix.set_codebook(cent, np.full(dim, -2, F), np.full(dim, 2, F))
    ix.add(x, labels)
    ix.build()
    exp = ix.export()
    assert np.diff(exp[3]).tolist() == sizes
    xh = decoded(exp)
    opt("sq_ivf_rpb", "64")  # the 1000-row list spans 16 segments
    q = (cent[[0, 1, 2, 3, 5, 1]] + F(0.5) * rng.standard_normal((6, dim), dtype=F)).astype(F)
    for nprobe, k in ((nlist, 100), (2, 10), (1, 256), (3, 1)):
        got = ix.search(q, k, "nprobe=%d" % nprobe)
        same(got, ref_search(exp, xh, q, nprobe, k, L2))
    ids, dis = ix.search(q[1:2], 10, "nprobe=2")  # lists 1 and 2: four rows for ten slots
    assert (ids[0, :4] >= 0).all() and (ids[0, 4:] == -1).all() and (dis[0, 4:] == FLT_MAX).all()
    ids, dis = ix.search(q[3:4], 5, "nprobe=1")  # an empty list
    assert (ids == -1).all() and (dis == FLT_MAX).all()
    same(device_search(ix, q, 100, nlist), ref_search(exp, xh, q, nlist, 100, L2))


# ---------------------------------------------------------------------------------------- 4. quantiser edges

def test_constant_dimension_and_rows_outside_the_range():
    rng = np.random.default_rng(4)
    dim, n = 24, 2000
    centres, x = blobs(rng, n, dim, NLIST)
    x[:, 7] = 0  # constant over the training rows (and so over the centroids: every residual there is 0)
    ix = capi.SqIndex(L2, dim, "ncentroids=%d,kmeans_iters=4" % NLIST)
    ix.train(x)
    far = x[:6].copy()
    far[:3] += F(100)  # outside the trained range in both directions
    far[3:] -= F(100)
    allx = np.concatenate([x, far])
    ix.add(allx, np.arange(len(allx), dtype=np.int64) * 2)
    ix.build()
    exp = ix.export()
    cent, lo, hi, off, codes, labels = exp
    lists = lists_of(off)
    # step == 0 in column 7: all codes 0 there, decoded to c + vmin
    assert step_of(lo, hi)[7] == 0 and lo[7] == hi[7]
    where = labels // 2
    assert (codes == encode(allx[where], cent[lists], lo, hi)).all()
    xh = decoded(exp)
    zero_step = step_of(lo, hi) == 0
    assert (codes[:, zero_step] == 0).all()
    assert (xh[:, zero_step] == (cent[lists] + lo).astype(F)[:, zero_step]).all()
    out = where >= n
    assert out.sum() == 6
    moving = ~zero_step
    assert (codes[out][labels[out] < 2 * (n + 3)][:, moving] == 255).all() and (codes[out][labels[out] >= 2 * (n + 3)][:, moving] == 0).all()
    q = np.concatenate([far, x[:10]])
    same(ix.search(q, 10, "nprobe=%d" % NLIST), ref_search(exp, xh, q, NLIST, 10, L2))


def test_step_zero_by_hand():
    """A codebook whose range is empty in one dimension: codes 0 there, decoded to c + vmin exactly."""
    rng = np.random.default_rng(5)
    dim = 16
    cent = rng.standard_normal((3, dim), dtype=F)
    lo, hi = np.full(dim, -1, F), np.full(dim, 1, F)
    lo[5] = hi[5] = F(0.375)
    x = (cent[rng.integers(0, 3, 200)] + F(0.2) * rng.standard_normal((200, dim), dtype=F)).astype(F)
    ix = capi.SqIndex(IP, dim)
    ix.set_codebook(cent, lo, hi)
    ix.add(x)
    ix.build()
    exp = ix.export()
    xh = decoded(exp)
    assert (exp[4][:, 5] == 0).all() and (xh[:, 5] == (exp[0][lists_of(exp[3])][:, 5] + F(0.375)).astype(F)).all()
    same(ix.search(x[:5], 20, "nprobe=3"), ref_search(exp, xh, x[:5], 3, 20, IP))


# ---------------------------------------------------------------------------------------- 5. filter by label

@pytest.mark.parametrize("metric", [L2, COS])
def test_filter_by_label(metric):
    ix, exp, xh, _, labels, q = case(metric, 64, "clustered")
    q = q[:20]
    rng = np.random.default_rng(6)
    top = int(labels.max()) + 1
    half = rng.random(top) < 0.5
    one = np.zeros(top, bool)
    one[labels[17]] = True
    none = np.zeros(top, bool)
    for alive in (half, one, none):
        same(ix.search(q, 10, "nprobe=4", alive=alive), ref_search(exp, xh, q, 4, 10, metric, alive=alive))
    same(device_search(ix, q, 10, NLIST, alive=half), ref_search(exp, xh, q, NLIST, 10, metric, alive=half))
    ids, _ = ix.search(q, 10, "nprobe=%d" % NLIST, alive=none)
    assert (ids == -1).all()
    # a bitmap shorter than the label space: labels at or beyond nbits are dead
    nbits = top // 2
    cut = np.ones(top, bool)
    cut[nbits:] = False
    got = ix.search(q, 10, "nprobe=%d" % NLIST, alive=np.ones(nbits, bool), nbits=nbits)
    same(got, ref_search(exp, xh, q, NLIST, 10, metric, alive=cut))
    assert (got[0] < nbits).all()


# ---------------------------------------------------------------------------------------- 6. lifecycle and errors

def code_of(fn):
    with pytest.raises(capi.MsvsError) as e:
        fn()
    return e.value.code


def test_lifecycle_and_errors():
    rng = np.random.default_rng(7)
    dim = 16
    _, x = blobs(rng, 500, dim, 4)
    ix = capi.SqIndex(L2, dim, "ncentroids=4,kmeans_iters=3")
    assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # no codebook yet
    assert code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY
    ix.train(x)
    assert not ix.ready
    assert code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY  # not built yet
    assert code_of(lambda: ix.add(x[:2], np.array([5, 2 ** 32 - 1]))) == capi.ERR_ID_RANGE
    assert code_of(lambda: ix.add(x[:2], np.array([-1, 3]))) == capi.ERR_ID_RANGE
    assert ix.num_data == 0
    ix.add(x[:2], np.array([1000, 2 ** 32 - 2]))  # the largest label
    ix.add(x[2:])
    assert code_of(lambda: ix.train(x)) == capi.ERR_INVALID_ARGUMENT  # the codebook is fixed once rows are staged
    ix.build()
    assert ix.ready and ix.num_data == 500
    assert code_of(lambda: ix.add(x)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ix.search(x[:1], 257)) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search(x[:1], 1, "nprobe=0")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ix.search(x[:1], 1, "efsearch=3")) == capi.ERR_INVALID_ARGUMENT
    ids, dis = ix.search(x[:3], 0)  # k = 0: nothing to return, as everywhere in the library
    assert ids.shape == (3, 0) and dis.shape == (3, 0)
    ids, _ = ix.search(x[:1], 1, "nprobe=4")
    assert ids[0, 0] == 1000
    assert code_of(lambda: capi.SqIndex(capi.METRIC_HAMMING, dim)) == capi.ERR_NOT_IMPLEMENTED
    assert code_of(lambda: capi.SqIndex(L2, 4096)) == capi.ERR_INVALID_ARGUMENT  # beyond the scan's LDS stage
    assert code_of(lambda: capi.SqIndex(L2, 0)) == capi.ERR_INVALID_ARGUMENT
    bad = capi.SqIndex(L2, dim)
    cent, lo, hi = x[:3], np.full(dim, -1, F), np.full(dim, 1, F)
    for j, (a, b) in enumerate(((1.0, -1.0), (np.nan, 1.0), (-1.0, np.inf))):
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j], hi2[j] = a, b
        assert code_of(lambda: bad.set_codebook(cent, lo2, hi2)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # a refused codebook leaves none


def test_largest_dimension_at_the_lds_edge():
    """d = 2240, k = 256: the LDS image of the smallest tile (T = 2) is 65280 of 65536 bytes; a batch that would take T = 8."""
    rng = np.random.default_rng(12)
    dim, nlist, n = 2240, 4, 600
    centres, x = blobs(rng, n, dim, nlist)
    ix = capi.SqIndex(IP, dim)
    ix.set_codebook(centres, np.full(dim, -1.5, F), np.full(dim, 1.5, F))
    ix.add(x, np.arange(n, dtype=np.int64) * 3)
    ix.build()
    exp = ix.export()
    xh = decoded(exp)
    q = x[:40] + F(0.1)
    for k in (256, 10):
        same(ix.search(q, k, "nprobe=%d" % nlist), ref_search(exp, xh, q, nlist, k, IP))
    same(device_search(ix, q[:3], 256, 2), ref_search(exp, xh, q[:3], 2, 256, IP))
    ix.close()


def test_nprobe_beyond_the_coarse_limit():
    dim, nlist = 8, 300
    rng = np.random.default_rng(8)
    cent = rng.standard_normal((nlist, dim), dtype=F)
    ix = capi.SqIndex(L2, dim)
    ix.set_codebook(cent, np.full(dim, -1, F), np.full(dim, 1, F))
    ix.add(cent)
    ix.build()
    assert code_of(lambda: ix.search(cent[:1], 1, "nprobe=257")) == capi.ERR_UNSUPPORTED_K
    exp = ix.export()
    same(ix.search(cent[:4], 5, "nprobe=256"), ref_search(exp, decoded(exp), cent[:4], 256, 5, L2))


def test_training_is_deterministic():
    rng = np.random.default_rng(9)
    _, x = blobs(rng, 2000, 32, NLIST)
    exps = []
    for _ in range(2):
        ix = capi.SqIndex(L2, 32, "ncentroids=%d,kmeans_iters=5" % NLIST)
        ix.train(x)
        ix.train(x)  # (again on the same object: replaces the codebook with the same one)
        ix.add(x)
        ix.build()
        exps.append(ix.export())
        ix.close()
    for a, b in zip(*exps):
        assert a.tobytes() == b.tobytes()


def test_memory_usage_is_codes_plus_labels():
    rng = np.random.default_rng(10)
    n, dim, nlist = 20000, 64, 16
    _, x = blobs(rng, n, dim, nlist)
    ix = capi.SqIndex(L2, dim, "ncentroids=%d,kmeans_iters=2" % nlist)
    ix.train(x[:4000])
    ix.add(x[:12000])
    ix.add(x[12000:])
    ix.build()
    bound = n * (((dim + 15) // 16) * 16 + 8) + nlist * dim * 4 + 2 * dim * 4 + (nlist + 1) * 8 + 4096
    assert n * dim <= ix.memory_usage <= bound
    ix.close()


# ---------------------------------------------------------------------------------------- 7. files

def test_files_round_trip_and_corruption():
    ix, exp, xh, _, _, q = case(IP, 100, "clustered")
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["sq_data", "sq_ids"]
    ld = capi.SqIndex.load_io(store, IP, 100)
    assert ld.ready and ld.num_data == ix.num_data and ld.num_lists == NLIST
    for a, b in zip(exp, ld.export()):
        assert a.tobytes() == b.tobytes()
    same(ld.search(q[:30], 10, "nprobe=3"), ix.search(q[:30], 10, "nprobe=3"))
    same(ld.search(q[:30], 10, "nprobe=3"), ref_search(exp, xh, q[:30], 3, 10, IP))
    ld.close()
    for name in ("sq_data", "sq_ids"):
        full = store[name]
        for cut in (0, 10, len(full) // 2, len(full) - 1):
            bad = dict(store)
            bad[name] = bytearray(full[:cut])
            assert code_of(lambda: capi.SqIndex.load_io(bad, IP, 100)) == capi.ERR_IO, (name, cut)
        header = 56 if name == "sq_data" else 24
        for pos in range(header):
            bad = dict(store)
            bad[name] = bytearray(full)
            bad[name][pos] ^= 0x01
            assert code_of(lambda: capi.SqIndex.load_io(bad, IP, 100)) == capi.ERR_IO, (name, pos)
        bad = dict(store)
        bad[name] = bytearray(full) + b"\0"
        assert code_of(lambda: capi.SqIndex.load_io(bad, IP, 100)) == capi.ERR_IO, name
    missing = {"sq_data": store["sq_data"]}
    assert code_of(lambda: capi.SqIndex.load_io(missing, IP, 100)) == capi.ERR_IO
    fresh = capi.SqIndex(L2, 8)
    assert code_of(lambda: fresh.serialize_io({})) == capi.ERR_NOT_READY


# ---------------------------------------------------------------------------------------- 8. quality of the specification

@pytest.mark.parametrize("metric", [L2, IP])
def test_recall_against_the_original_rows(metric):
    """The semantics, not the kernel: 8192 x 64 rows in 32 blobs (sigma 0.3, centres N(0, 1)), the quantiser trained on every
    second row, every list probed.  Recall@10 against the exact search of the ORIGINAL rows must be >= 0.95 -- first for the numpy
    restatement over the exported codebook (0.976 for L2 and 0.981 for IP in a stand-alone restatement of this set-up), then
    for the index."""
    rng = np.random.default_rng(11)
    n, dim, nlist, nq, k = 8192, 64, 32, 200, 10
    centres, x = blobs(rng, n, dim, nlist)
    q = (centres[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    om = o.METRIC_L2 if metric == L2 else o.METRIC_IP
    truth, _ = o.knn(q, x, k, om)
    ix = capi.SqIndex(metric, dim, "ncentroids=%d,kmeans_iters=6" % nlist)
    ix.train(x[::2])
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent, lo, hi, off, codes, labels = exp
    lists = lists_of(off)
    xh = decode(encode(x[labels], cent[lists], lo, hi), cent[lists], lo, hi)

    def recall(ids):
        return np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, truth)])

    ref_ids, ref_dis, _ = o.ivf_search(cent, off, xh, labels, q, nlist, k, om)
    r_ref = recall(ref_ids)
    print("recall@10 of the reference:", r_ref)
    assert r_ref >= 0.95
    got = ix.search(q, k, "nprobe=%d" % nlist)
    r_ix = recall(got[0])
    print("recall@10 of the index:", r_ix)
    assert r_ix >= 0.95
    same(got, (ref_ids, ref_dis))
    ix.close()
