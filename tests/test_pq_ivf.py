"""The IVFPQ index (msvs_pq_index_*, capi.PqIndex): product-quantised residual codes only, searched through per-(query, list) tables.

The reference is composed here from the semantics in include/msvs.h alone: a numpy sequential sum, the decoded matrix
X^ = fl(c[list of row] + cb[s][code]) from the export, per-(query, row) sub-scores summed over s in f32, the probes of
oracle.ivf_search over X^, a numpy top-k by (distance, label).  Every comparison is == on ids and on the uint32 view of the
distances; codes byte for byte."""
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
SHAPES = [(5, 5), (5, 1), (64, 16), (100, 20), (100, 25), (768, 96)]  # dsub 1, 5 (odd), 4, 5, 4, 8; m not a multiple of 4


def seqsum(p):
    """sum over the last axis, ascending, every addition rounded to f32, starting at +0"""
    s = np.zeros(p.shape[:-1], F)
    for t in range(p.shape[-1]):
        s = (s + p[..., t]).astype(F)
    return s


def ordered(v):
    """the ordered-integer image of f32 values: ascending with the floats, -0 before +0"""
    u = np.ascontiguousarray(v, F).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def lists_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def stored(x, metric):
    return o.normalize_rows(x) if metric == COS else np.ascontiguousarray(x, F)


def encode(x, c, cb):
    """x: stored rows, c: the centroid of each row's list, cb: [m, 256, dsub] -> codes [n, m]"""
    m, _, dsub = cb.shape
    codes = np.empty((len(x), m), np.uint8)
    for s in range(m):
        sub = slice(s * dsub, (s + 1) * dsub)
        with np.errstate(invalid="ignore", over="ignore"):
            xh = (c[:, None, sub] + cb[s][None]).astype(F)
            t = (x[:, None, sub] - xh).astype(F)
            e = seqsum((t * t).astype(F))
        key = ordered(e).astype(np.uint64)
        key[np.isnan(e)] = 1 << 33  # a NaN score never wins; all NaN: argmin gives 0
        codes[:, s] = key.argmin(axis=1)  # the first (lowest j) among equals
    return codes


def decoded(exp):
    cent, cb, off, codes, labels = exp
    m = cb.shape[0]
    c = cent[lists_of(off)]
    return np.concatenate([(c[:, s * cb.shape[2]:(s + 1) * cb.shape[2]] + cb[s][codes[:, s]]).astype(F) for s in range(m)], axis=1)


def adc(xh, q, m, ip):
    """dis[q, row]: +0, then + the sub-score of every sub-space in turn, each a sequential f32 sum"""
    dsub = xh.shape[1] // m
    dis = np.zeros((len(q), len(xh)), F)
    for s in range(m):
        sub = slice(s * dsub, (s + 1) * dsub)
        with np.errstate(invalid="ignore", over="ignore"):
            if ip:
                e = seqsum((q[:, None, sub] * xh[None, :, sub]).astype(F))
            else:
                t = (q[:, None, sub] - xh[None, :, sub]).astype(F)
                e = seqsum((t * t).astype(F))
            dis = (dis + e).astype(F)
    return dis


def ref_search(exp, xh, q, nprobe, k, metric, alive=None):
    cent, cb, off, codes, labels = exp
    ip = metric != L2
    if metric == COS:
        q = o.normalize_rows(q)
    q = np.ascontiguousarray(q, F)
    _, _, probes = o.ivf_search(cent, off, xh, labels, q, nprobe, 1, o.METRIC_IP if ip else o.METRIC_L2)
    dis = adc(xh, q, cb.shape[0], ip)
    lists = lists_of(off)
    ids = np.full((len(q), k), -1, np.int64)
    out = np.full((len(q), k), -FLT_MAX if ip else FLT_MAX, F)
    ok_row = np.ones(len(labels), bool) if alive is None else np.array([l < len(alive) and alive[l] for l in labels], bool)
    for i in range(len(q)):
        d = dis[i]
        better = (d > -FLT_MAX) if ip else (d < FLT_MAX)  # strictly better than the neutral value; NaN never
        cand = np.flatnonzero(np.isin(lists, probes[i]) & ok_row & better)
        key = ordered(d[cand])
        if ip:
            key = ~key
        order = cand[np.lexsort((labels[cand], key))][:k]
        ids[i, :len(order)] = labels[order]
        out[i, :len(order)] = d[order]
    if metric == COS:
        out = (F(1) - out).astype(F)
    return ids, out


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


def random_codebooks(rng, m, dsub, scale=0.5):
    return (F(scale) * rng.standard_normal((m, 256, dsub), dtype=F)).astype(F)


@functools.lru_cache(maxsize=None)
def case(metric, dim, m, data):
    """A trained and built index of 3000 rows in three chunks, its export, the decoded matrix and 300 queries; computed once."""
    rng = np.random.default_rng(dim * 13 + m * 101 + metric * 5 + len(data))
    n = 3000
    centres, x = blobs(rng, n, dim, NLIST)
    if data == "ties":  # 40 distinct vectors: equal distances everywhere, ordered by label
        x = np.ascontiguousarray(x[:40][rng.integers(0, 40, n)])
    labels = rng.permutation(3 * n)[:n].astype(np.int64)  # shuffled, not contiguous
    q = (centres[rng.integers(0, NLIST, 300)] + F(0.3) * rng.standard_normal((300, dim), dtype=F)).astype(F)
    ix = capi.PqIndex(metric, dim, "ncentroids=%d,m=%d,kmeans_iters=4" % (NLIST, m))
    ix.train(x)
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        ix.add(x[a:b], labels[a:b])
    ix.build()
    exp = ix.export()
    return ix, exp, decoded(exp), x, labels, q


# ---------------------------------------------------------------------------------------- 1. structure and codes

@pytest.mark.parametrize("dim,m", SHAPES)
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_structure_and_codes(metric, dim, m):
    ix, exp, _, x, labels, _ = case(metric, dim, m, "clustered")
    cent, cb, off, codes, elab = exp
    n = len(x)
    assert ix.ready and ix.num_data == n and ix.num_lists == NLIST
    assert cent.shape == (NLIST, dim) and cb.shape == (m, 256, dim // m) and codes.shape == (n, m)
    assert np.isfinite(cb).all()
    assert len(off) == NLIST + 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert sorted(elab.tolist()) == sorted(labels.tolist())
    for l in range(NLIST):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    where = {int(l): i for i, l in enumerate(labels)}
    xs = stored(x, metric)[[where[int(l)] for l in elab]]  # the fed rows in export order
    assert (codes == encode(xs, cent[lists_of(off)], cb)).all()


def test_ties_go_to_the_lower_entry_and_an_all_equal_subspace_gives_zero():
    rng = np.random.default_rng(21)
    dim, m, nlist = 12, 3, 3
    dsub = dim // m
    cent = rng.standard_normal((nlist, dim), dtype=F)
    cb = random_codebooks(rng, m, dsub)
    cb[0, 128:] = cb[0, :128]  # every entry of sub-space 0 twice: the lower one wins
    cb[1, :] = cb[1, 77]       # sub-space 1: all entries equal
    cb[2, 5] = cb[2, 200]      # one duplicated pair in an otherwise distinct codebook
    home = rng.integers(0, nlist, 1500)
    x = (cent[home] + F(0.5) * rng.standard_normal((1500, dim), dtype=F)).astype(F)
    x[:300, 2 * dsub:] = (cent[home[:300], 2 * dsub:] + cb[2, 200]).astype(F)  # rows at the duplicated entry
    ix = capi.PqIndex(L2, dim, "m=%d" % m)
    ix.set_codebook(cent, cb)
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent2, cb2, off, codes, labels = exp
    assert cent2.tobytes() == cent.tobytes() and cb2.tobytes() == cb.tobytes()
    assert (codes[:, 0] < 128).all() and (codes[:, 1] == 0).all() and (codes[:, 2] != 200).all() and (codes[:, 2] == 5).any()
    assert (codes == encode(x[labels], cent[lists_of(off)], cb)).all()
    same(ix.search(x[:7], 20, "nprobe=%d" % nlist), ref_search(exp, decoded(exp), x[:7], nlist, 20, L2))


# ---------------------------------------------------------------------------------------- 2. search parity

# The list scan's query tile T: 8 from 16 pairs per list on, 4 from 2, 2 from 1, else 1 (pairs = nq * min(nprobe, nlist), nlist = 8),
# halved until T * m KiB of tables + (T + 1) * 4 * dim + T * 40 * k bytes fit 160 KiB; its top-k class R: 1 / 2 / 4 for k <= 64 /
# <= 128 / <= 256.  The last column names the (T, R) a row reaches; together they reach all twelve.
PARITY = [
    (L2, 5, 5, "clustered", 1, 1, 1, "host", (1, 1)),
    (L2, 5, 1, "ties", 300, 256, NLIST, "device", (8, 4)),
    (IP, 5, 5, "ties", 40, 100, 4, "host", (8, 2)),
    (COS, 5, 1, "clustered", 9, 10, 4, "device", (4, 1)),
    (L2, 64, 16, "clustered", 300, 10, 4, "host", (8, 1)),
    (L2, 64, 16, "ties", 300, 256, NLIST, "host", (4, 4)),  # (tile 8 would need 128 KiB of tables + 80 KiB of merge lists)
    (IP, 64, 16, "clustered", 3, 256, 4, "host", (2, 4)),
    (COS, 64, 16, "ties", 300, 1, NLIST, "host", (8, 1)),
    (L2, 64, 16, "clustered", 1, 100, 4, "device", (1, 2)),
    (L2, 100, 20, "ties", 3, 100, NLIST, "host", (4, 2)),
    (IP, 100, 20, "clustered", 300, 100, 1, "host", (4, 2)),
    (COS, 100, 25, "clustered", 1, 256, 10 * NLIST, "device", (2, 4)),
    (L2, 100, 25, "clustered", 40, 10, NLIST, "device", (4, 1)),
    (IP, 100, 25, "ties", 9, 1, 1, "host", (2, 1)),
    (L2, 768, 96, "clustered", 40, 10, 4, "host", (1, 1)),
    (L2, 768, 96, "clustered", 9, 256, 10 * NLIST, "device", (1, 4)),
    (IP, 768, 96, "ties", 1, 10, 10 * NLIST, "device", (1, 1)),
    (COS, 768, 96, "clustered", 3, 100, 1, "host", (1, 2)),
    (IP, 5, 5, "ties", 16, 150, NLIST, "device", (8, 4)),
    (COS, 5, 5, "clustered", 9, 100, 4, "host", (4, 2)),
    (IP, 5, 1, "clustered", 3, 10, 4, "host", (2, 1)),
    (L2, 100, 20, "clustered", 1, 100, NLIST, "host", (2, 2)),
    (COS, 64, 16, "clustered", 40, 256, 1, "device", (4, 4)),
    (IP, 100, 25, "clustered", 300, 256, NLIST, "host", (4, 4)),
    (L2, 5, 1, "clustered", 1, 256, 4, "host", (1, 4)),
]


def tile_class(dim, m, nq, k, nprobe):
    pairs = nq * min(nprobe, NLIST)
    t = 8 if pairs >= 16 * NLIST else 4 if pairs >= 2 * NLIST else 2 if pairs >= NLIST else 1
    while t > 1 and t * m * 1024 + (t + 1) * ((dim + 3) // 4 * 4) * 4 + t * 40 * k > 160 * 1024:
        t //= 2
    return t, 1 if k <= 64 else 2 if k <= 128 else 4


def test_parity_table_reaches_every_tile_and_k_class():
    reached = set()
    for metric, dim, m, data, nq, k, nprobe, entry, cls in PARITY:
        assert tile_class(dim, m, nq, k, nprobe) == cls
        reached.add(cls)
    assert reached == {(t, r) for t in (1, 2, 4, 8) for r in (1, 2, 4)}


@pytest.mark.parametrize("metric,dim,m,data,nq,k,nprobe,entry,cls", PARITY)
def test_search_parity(metric, dim, m, data, nq, k, nprobe, entry, cls):
    ix, exp, xh, _, _, q = case(metric, dim, m, data)
    q = q[:nq]
    got = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else device_search(ix, q, k, nprobe)
    same(got, ref_search(exp, xh, q, nprobe, k, metric))


def by_hand(rng, metric, dim, m, nlist, n, scale=0.5):
    centres, x = blobs(rng, n, dim, nlist)
    ix = capi.PqIndex(metric, dim, "m=%d" % m)
    ix.set_codebook(centres, random_codebooks(rng, m, dim // m, scale))
    ix.add(x, np.arange(n, dtype=np.int64) * 3)
    ix.build()
    exp = ix.export()
    return ix, exp, decoded(exp), x


def test_most_subquantisers_only_the_single_query_tile_fits():
    """dim 768, m 128 (dsub 6), k 256: 128 KiB of tables + 6 KiB of staging + 10 KiB of merge lists; a batch that would take T = 8."""
    ix, exp, xh, x = by_hand(np.random.default_rng(12), IP, 768, 128, 4, 600)
    q = x[:40] + F(0.1)
    for k in (256, 10):
        same(ix.search(q, k, "nprobe=4"), ref_search(exp, xh, q, 4, k, IP))
    same(device_search(ix, q[:3], 256, 2), ref_search(exp, xh, q[:3], 2, 256, IP))
    ix.close()


def test_one_subquantiser():
    ix, exp, xh, x = by_hand(np.random.default_rng(13), L2, 48, 1, 5, 900)
    q = x[:33] + F(0.05)
    assert exp[3].shape == (900, 1)
    same(ix.search(q, 100, "nprobe=5"), ref_search(exp, xh, q, 5, 100, L2))
    same(device_search(ix, q[:2], 7, 2), ref_search(exp, xh, q[:2], 2, 7, L2))
    ix.close()


# ---------------------------------------------------------------------------------------- 3. edge lists

def test_empty_short_and_segmented_lists(opt):
    rng = np.random.default_rng(3)
    dim, m, nlist = 20, 5, 6
    cent = np.zeros((nlist, dim), F)
    cent[:, 0] = 10.0 * np.arange(nlist)
    sizes = [1000, 3, 1, 0, 0, 50]  # two empty lists, one shorter than a wavefront, one single row, one of several segments
    home = np.repeat(np.arange(nlist), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    labels = rng.permutation(5000)[:len(home)].astype(np.int64)
    ix = capi.PqIndex(L2, dim, "m=%d" % m)
    ix.set_codebook(cent, random_codebooks(rng, m, dim // m, 0.4))
    ix.add(x, labels)
    ix.build()
    exp = ix.export()
    assert np.diff(exp[2]).tolist() == sizes
    xh = decoded(exp)
    opt("pq_ivf_rpb", "64")  # rounded up to one 256-row step: the 1000-row list spans 4 segments, each with tables of its own
    q = (cent[[0, 1, 2, 3, 5, 1]] + F(0.5) * rng.standard_normal((6, dim), dtype=F)).astype(F)
    for nprobe, k in ((nlist, 100), (2, 10), (1, 256), (3, 1)):
        got = ix.search(q, k, "nprobe=%d" % nprobe)
        same(got, ref_search(exp, xh, q, nprobe, k, L2))
    ids, dis = ix.search(q[1:2], 10, "nprobe=2")  # lists 1 and 2: four rows for ten slots
    assert (ids[0, :4] >= 0).all() and (ids[0, 4:] == -1).all() and (dis[0, 4:] == FLT_MAX).all()
    ids, dis = ix.search(q[3:4], 5, "nprobe=1")  # an empty list
    assert (ids == -1).all() and (dis == FLT_MAX).all()
    same(device_search(ix, q, 100, nlist), ref_search(exp, xh, q, nlist, 100, L2))


def test_twelve_segments(opt):
    """A 3000-row list in 256-row segments: eleven whole ones and one of 184 rows, every one with tables of its own, and the merge over
    twelve partial lists per (query, list) pair (the 1000-row list above reaches four)."""
    rng = np.random.default_rng(31)
    dim, m, sizes = 20, 5, [3000, 70]
    cent = np.zeros((2, dim), F)
    cent[1, 0] = 10.0
    home = np.repeat(np.arange(2), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    ix = capi.PqIndex(L2, dim, "m=%d" % m)
    ix.set_codebook(cent, random_codebooks(rng, m, dim // m, 0.4))
    ix.add(x, rng.permutation(9000)[:len(home)].astype(np.int64))
    ix.build()
    exp = ix.export()
    assert np.diff(exp[2]).tolist() == sizes
    xh = decoded(exp)
    opt("pq_ivf_rpb", "64")  # rounded up to one 256-row step
    q = (cent[[0, 1, 0, 0, 1]] + F(0.5) * rng.standard_normal((5, dim), dtype=F)).astype(F)
    for nprobe, k in ((2, 100), (1, 256), (2, 1)):
        same(ix.search(q, k, "nprobe=%d" % nprobe), ref_search(exp, xh, q, nprobe, k, L2))
    same(device_search(ix, q, 256, 2), ref_search(exp, xh, q, 2, 256, L2))
    ix.close()


# ---------------------------------------------------------------------------------------- 4. filter by label

@pytest.mark.parametrize("metric", [L2, COS])
def test_filter_by_label(metric):
    ix, exp, xh, _, labels, q = case(metric, 64, 16, "clustered")
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


# ---------------------------------------------------------------------------------------- 5. lifecycle and errors

def code_of(fn):
    with pytest.raises(capi.MsvsError) as e:
        fn()
    return e.value.code


def test_lifecycle_and_errors():
    rng = np.random.default_rng(7)
    dim, m = 16, 4
    _, x = blobs(rng, 500, dim, 4)
    ix = capi.PqIndex(L2, dim, "ncentroids=4,m=%d,kmeans_iters=3" % m)
    assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # no codebook yet
    assert code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY
    assert code_of(lambda: ix.train(x[:255])) == capi.ERR_INVALID_ARGUMENT  # fewer rows than entries of a sub-codebook
    assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY
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
    exp = ix.export()
    same(ix.search(x[:4], 3, "nprobe=4"), ref_search(exp, decoded(exp), x[:4], 4, 3, L2))
    assert 1000 in exp[4] and 2 ** 32 - 2 in exp[4]
    assert code_of(lambda: capi.PqIndex(capi.METRIC_HAMMING, dim, "m=4")) == capi.ERR_NOT_IMPLEMENTED
    assert code_of(lambda: capi.PqIndex(L2, dim)) == capi.ERR_INVALID_ARGUMENT  # m missing
    assert code_of(lambda: capi.PqIndex(L2, dim, "m=3")) == capi.ERR_INVALID_ARGUMENT  # m does not divide dim
    assert code_of(lambda: capi.PqIndex(L2, dim, "m=0")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.PqIndex(L2, 258, "m=129")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.PqIndex(L2, 0, "m=1")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.PqIndex(L2, 8192, "m=128")) == capi.ERR_INVALID_ARGUMENT  # 128 + 64 + 10 KiB of LDS
    bad = capi.PqIndex(L2, dim, "m=%d" % m)
    cb = random_codebooks(rng, m, dim // m)
    for v in (np.nan, np.inf):
        cb2 = cb.copy()
        cb2[2, 99, 1] = v
        assert code_of(lambda: bad.set_codebook(x[:3], cb2)) == capi.ERR_INVALID_ARGUMENT
        assert code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # a refused codebook leaves none
    bad.set_codebook(x[:3], cb)
    cb2 = cb.copy()
    cb2[0, 0, 0] = np.nan
    assert code_of(lambda: bad.set_codebook(x[:3], cb2)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # ... not even the one it had


def test_nprobe_beyond_the_coarse_limit():
    dim, m, nlist = 8, 2, 300
    rng = np.random.default_rng(8)
    cent = rng.standard_normal((nlist, dim), dtype=F)
    ix = capi.PqIndex(L2, dim, "m=%d" % m)
    ix.set_codebook(cent, random_codebooks(rng, m, dim // m, 0.2))
    ix.add(cent)
    ix.build()
    assert code_of(lambda: ix.search(cent[:1], 1, "nprobe=257")) == capi.ERR_UNSUPPORTED_K
    exp = ix.export()
    same(ix.search(cent[:4], 5, "nprobe=256"), ref_search(exp, decoded(exp), cent[:4], 256, 5, L2))


# ---------------------------------------------------------------------------------------- 6. determinism

def test_training_is_deterministic():
    rng = np.random.default_rng(9)
    _, x = blobs(rng, 2000, 32, NLIST)
    exps = []
    for _ in range(2):
        ix = capi.PqIndex(L2, 32, "ncentroids=%d,m=8,kmeans_iters=5" % NLIST)
        ix.train(x)
        if exps:
            ix.train(x)  # (again on the same object: replaces the codebook with the same one)
        ix.add(x)
        ix.build()
        exps.append(ix.export())
        ix.close()
    for a, b in zip(*exps):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------- 7. memory

def test_memory_usage_is_codes_plus_labels():
    rng = np.random.default_rng(10)
    n, dim, m, nlist = 20000, 64, 16, 16
    _, x = blobs(rng, n, dim, nlist)
    ix = capi.PqIndex(L2, dim, "ncentroids=%d,m=%d,kmeans_iters=2" % (nlist, m))
    ix.train(x[:4000])
    ix.add(x[:12000])
    ix.add(x[12000:])
    ix.build()
    tables = nlist * dim * 4 + 256 * dim * 4 + (nlist + 1) * 8
    assert n * m <= ix.memory_usage <= n * ((m + 15) // 16 * 16 + 8) + tables + 4096
    ix.close()


# ---------------------------------------------------------------------------------------- 8. files

def test_files_round_trip_and_corruption():
    ix, exp, xh, _, _, q = case(IP, 100, 25, "clustered")
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["pq_data", "pq_ids"]
    assert bytes(store["pq_data"][:8]) == b"MSVSPQ01"
    ld = capi.PqIndex.load_io(store, IP, 100, 25)
    assert ld.ready and ld.num_data == ix.num_data and ld.num_lists == NLIST
    for a, b in zip(exp, ld.export()):
        assert a.tobytes() == b.tobytes()
    same(ld.search(q[:30], 10, "nprobe=3"), ix.search(q[:30], 10, "nprobe=3"))
    same(ld.search(q[:30], 10, "nprobe=3"), ref_search(exp, xh, q[:30], 3, 10, IP))
    ld.close()
    for name in ("pq_data", "pq_ids"):
        full = store[name]
        for cut in (0, 10, len(full) // 2, len(full) - 1):
            bad = dict(store)
            bad[name] = bytearray(full[:cut])
            assert code_of(lambda: capi.PqIndex.load_io(bad, IP, 100, 25)) == capi.ERR_IO, (name, cut)
        header = 64 if name == "pq_data" else 24
        for pos in range(header):
            bad = dict(store)
            bad[name] = bytearray(full)
            bad[name][pos] ^= 0x01
            assert code_of(lambda: capi.PqIndex.load_io(bad, IP, 100, 25)) == capi.ERR_IO, (name, pos)
        bad = dict(store)
        bad[name] = bytearray(full) + b"\0"
        assert code_of(lambda: capi.PqIndex.load_io(bad, IP, 100, 25)) == capi.ERR_IO, name
    missing = {"pq_data": store["pq_data"]}
    assert code_of(lambda: capi.PqIndex.load_io(missing, IP, 100, 25)) == capi.ERR_IO
    fresh = capi.PqIndex(L2, 8, "m=2")
    assert code_of(lambda: fresh.serialize_io({})) == capi.ERR_NOT_READY


def test_loaded_geometry_comes_from_the_file():
    ix, exp, _, _, _, _ = case(IP, 100, 25, "clustered")
    store = {}
    ix.serialize_io(store)
    ld = capi.PqIndex.load_io(store)  # nothing repeated by the caller
    assert (ld.metric, ld.dim, ld.m) == (IP, 100, 25)
    for a, b in zip(exp, ld.export()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    ld.close()
    for wrong in ((L2, 100, 25), (IP, 50, 25), (IP, 100, 20)):  # a caller's mistake is an error, never a wrongly sized export
        with pytest.raises(ValueError):
            capi.PqIndex.load_io(store, *wrong)


# ---------------------------------------------------------------------------------------- 9. recall of the trained index

@pytest.mark.parametrize("metric", [L2, IP])
def test_recall_against_the_original_rows(metric):
    """4000 x 64 rows in 8 blobs (sigma 0.3, centres N(0, 1)), 8 lists, m = 16, every list probed, 100 queries.  The share of the
    exact top-10 of the ORIGINAL rows found in the top-100 must be >= 0.95 -- first for the numpy restatement over the exported
    codebook, then for the index (a numpy restatement with a 5-iteration Lloyd codebook gives 0.992 / 0.998 / 1.000 over three
    seeds for L2 and 1.000 for IP).  Top-10 in top-10 is the quantiser's loss (0.58 - 0.65 there): printed, not asserted."""
    rng = np.random.default_rng(11)
    n, dim, m, nlist, nq = 4000, 64, 16, 8, 100
    centres, x = blobs(rng, n, dim, nlist)
    q = (centres[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    if metric == L2:
        exact = ((q[:, None, :].astype(np.float64) - x[None]) ** 2).sum(-1)
    else:
        exact = -(q.astype(np.float64) @ x.T.astype(np.float64))
    truth = np.argsort(exact, axis=1, kind="stable")[:, :10]
    ix = capi.PqIndex(metric, dim, "ncentroids=%d,m=%d,kmeans_iters=5" % (nlist, m))
    ix.train(x)
    ix.add(x)
    ix.build()
    exp = ix.export()

    def share(ids, width):
        return np.mean([len(set(t.tolist()) & set(g[:width].tolist())) / 10 for t, g in zip(truth, ids)])

    ref = ref_search(exp, decoded(exp), q, nlist, 100, metric)
    print("reference: 10 in 100 %.3f, 10 in 10 %.3f" % (share(ref[0], 100), share(ref[0], 10)))
    assert share(ref[0], 100) >= 0.95
    got = ix.search(q, 100, "nprobe=%d" % nlist)
    print("index: 10 in 100 %.3f, 10 in 10 %.3f" % (share(got[0], 100), share(got[0], 10)))
    assert share(got[0], 100) >= 0.95
    same(got, ref)
    ix.close()
