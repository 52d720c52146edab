"""The two-stage search: the row store (msvs_rows_*, capi.Rows), the exact re-rank of candidate labels (msvs_refine[_device]) and
the composed entries of the coded indexes (search_refine[_device]).

The reference is per query oracle.knn(q, rows[valid cand], k, metric, labels=valid cand) -- for cosine over oracle.normalize_rows of
both sides with IP, then fl(1 - x) in every slot -- padded with -1 and the metric's neutral value.  Every comparison is == on ids
and on the uint32 view of the distances."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o
from test_pq_ivf import blobs, code_of, decoded, ref_search, same

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
DEV, PIN = capi.ROWS_DEVICE, capi.ROWS_HOST_PINNED
FLT_MAX = np.finfo(np.float32).max
N = 3000


def ref_refine(x, q, cand, k, metric, num=None):
    """x: the rows as fed to the store (row i is label i); cand [nq, kc] labels"""
    num = len(x) if num is None else num
    ip = metric != L2
    xs = o.normalize_rows(x) if metric == COS else np.ascontiguousarray(x, F)
    qs = o.normalize_rows(q) if metric == COS else np.ascontiguousarray(q, F)
    ids = np.full((len(qs), k), -1, np.int64)
    dis = np.full((len(qs), k), -FLT_MAX if ip else FLT_MAX, F)
    for i, c in enumerate(np.asarray(cand, np.int64)):
        valid = c[(c >= 0) & (c < num)]
        if len(valid):
            ids[i], dis[i] = o.knn(qs[i], xs[valid], k, o.METRIC_IP if ip else o.METRIC_L2, labels=valid)
    if metric == COS:
        dis = (F(1) - dis).astype(F)
    return ids, dis


def store_of(x, metric, placement=DEV, capacity=None):
    rows = capi.Rows(x.shape[1], len(x) if capacity is None else capacity, normalize=metric == COS, placement=placement)
    rows.append(x)
    return rows


def device_refine(rows, metric, q, cand, k):
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    dc = torch.from_numpy(np.ascontiguousarray(cand, np.int64)).to(dev)
    di = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    dd = torch.empty((len(q), k), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    capi.refine_device(rows, metric, dq.data_ptr(), len(q), dc.data_ptr(), cand.shape[1], k, di.data_ptr(), dd.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


# ---------------------------------------------------------------------------------------- 1. parity table

# the pad (3), no pad (4), the tail group (67: 17 pieces), exactly one batch of twelve pieces a lane (768), one batch plus a tail
# (772), the four-at-a-time remainder (256: 4 pieces; 1000: 15 full + 10 of 16 lanes), two batches (1536), beyond (2052: 32 + 1 lane),
# the limit of the row store (8192: 32 KiB of query in LDS, ten batches and a remainder of eight) and the last ld below it (8188)
DIMS = [3, 4, 67, 256, 768, 772, 1000, 1536, 2052, 8188, 8192]
NQS = [1, 3, 65]
KCK = [(1, 1), (10, 10), (100, 10), (256, 256), (257, 100), (1024, 256), (5, 20)]  # one key a thread / four; k < = > kc; the limits


def parity_table():
    """four of the seven (kc, k) classes per dimension, the other axes rotating beside them"""
    table = []
    for i, dim in enumerate(DIMS):
        for j in range(4):
            c = i * 4 + j
            table.append(((L2, IP, COS)[(i + j) % 3], dim, NQS[(i + 2 * j) % 3], KCK[c % 7], ("host", "device")[c % 2], (DEV, PIN)[(c // 2) % 2]))
    return table


PARITY = parity_table()


def test_parity_table_reaches_every_axis():
    assert {r[1] for r in PARITY} == set(DIMS)
    assert {r[3] for r in PARITY} == set(KCK)
    assert {r[0] for r in PARITY} == {L2, IP, COS} and {r[2] for r in PARITY} == set(NQS)
    assert {r[4] for r in PARITY} == {"host", "device"} and {r[5] for r in PARITY} == {DEV, PIN}
    assert {(r[4], r[5]) for r in PARITY} == {(e, p) for e in ("host", "device") for p in (DEV, PIN)}
    for p in (DEV, PIN):  # both ranking paths (kc <= 256, kc > 256) and k > kc in both placements
        assert {r[3][0] > 256 for r in PARITY if r[5] == p} == {False, True}


@functools.lru_cache(maxsize=None)
def data(dim):
    rng = np.random.default_rng(1000 + dim)
    x = rng.standard_normal((N, dim), dtype=F)
    q = rng.standard_normal((65, dim), dtype=F)
    cand = np.stack([rng.permutation(N)[:1024] for _ in range(65)]).astype(np.int64)  # distinct labels per query
    return x, q, cand


@functools.lru_cache(maxsize=None)
def store(dim, normalize, placement):
    return store_of(data(dim)[0], COS if normalize else L2, placement)


@pytest.mark.parametrize("metric,dim,nq,kck,entry,placement", PARITY)
def test_refine_parity(metric, dim, nq, kck, entry, placement):
    kc, k = kck
    x, q, cand = data(dim)
    q, cand = q[:nq], np.ascontiguousarray(cand[:nq, :kc])
    rows = store(dim, metric == COS, placement)
    assert rows.num == N and rows.dim == dim and rows.normalized == (metric == COS)
    got = capi.refine(rows, metric, q, cand, k) if entry == "host" else device_refine(rows, metric, q, cand, k)
    same(got, ref_refine(x, q, cand, k, metric))


# ---------------------------------------------------------------------------------------- 2. candidate hygiene

@pytest.mark.parametrize("placement", [DEV, PIN])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_candidate_hygiene(metric, placement):
    x, q, _ = data(67)
    rows = store(67, metric == COS, placement)
    cand = np.array([
        [-1, 5, 9, 2000, 7, 11, 13, 17, 19, 23, 29, 31],            # -1 at the front
        [5, 9, -1, -1, 2000, 7, -7, 11, 13, 17, 19, 23],            # ... in the middle (and another negative label)
        [5, 9, 2000, 7, 11, 13, 17, 19, 23, 29, -1, -1],            # ... at the end
        [N, N + 1, 2 ** 32 + 5, 2 ** 40, 5, 2 ** 63 - 1, 9, 2 ** 32, 2 ** 31, 2999, 0, 2 ** 32 - 1],  # labels >= num (one whose low word is a row)
        [-1] * 12,                                                   # nothing at all
        [41, 8, 41, 3, 41, 8, 100, -1, 101, 102, 103, 104],          # 41 three times, 8 twice
        [-1, -1, -1, 77, -1, -1, N, -1, 78, -1, -1, -1],             # fewer valid candidates than k
    ], np.int64)
    q = q[:len(cand)]
    for k in (8, 12, 20):
        exp = ref_refine(x, q, cand, k, metric)
        same(capi.refine(rows, metric, q, cand, k), exp)
        same(device_refine(rows, metric, q, cand, k), exp)
    ids, dis = capi.refine(rows, metric, q, cand, 12)
    pad = FLT_MAX if metric != IP else -FLT_MAX  # (cosine: fl(1 - -FLT_MAX))
    assert (ids[4] == -1).all() and (dis[4] == pad).all()
    assert sorted(ids[3].tolist()) == [-1] * 8 + [0, 5, 9, 2999]
    assert sorted(ids[5].tolist()) == [-1, 3, 8, 8, 41, 41, 41, 100, 101, 102, 103, 104]
    assert sorted(ids[6].tolist()) == [-1] * 10 + [77, 78] and (ids[6, 2:] == -1).all() and (dis[6, 2:] == pad).all()


# ---------------------------------------------------------------------------------------- 3. order and admission

def special_rows():
    rng = np.random.default_rng(31)
    dim = 8
    x = rng.standard_normal((200, dim), dtype=F)
    copies = rng.permutation(200)[:40]
    x[copies] = x[copies[0]]  # forty copies of one row under different labels
    rest = np.setdiff1d(np.arange(200), copies)
    x[rest[0], 3] = np.nan
    x[rest[1], 0] = np.inf
    x[rest[2], 5] = -np.inf
    x[rest[3], 2] = F(3e19)   # its square overflows
    x[rest[4], 2] = F(-3e19)
    x[rest[5]] = F(3e19)
    x[rest[6], 1], x[rest[6], 4] = np.inf, -np.inf
    q = rng.standard_normal((6, dim), dtype=F)
    q[0] = x[copies[0]]
    q[2] = np.nan             # one query is all NaN
    q[3, 2] = F(3e19)
    q[4, 0] = np.inf
    q[5] = np.abs(q[5])       # (against the all-3e19 row: a huge finite inner product)
    return x, q, copies, rest


@pytest.mark.parametrize("placement", [DEV, PIN])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_order_and_admission(metric, placement):
    x, q, copies, rest = special_rows()
    rows = store_of(x, metric, placement)
    rng = np.random.default_rng(32)
    cand = np.stack([rng.permutation(200) for _ in range(len(q))]).astype(np.int64)  # every row, shuffled
    with np.errstate(all="ignore"):
        for k in (10, 200, 256):
            exp = ref_refine(x, q, cand, k, metric)
            same(capi.refine(rows, metric, q, cand, k), exp)
    ids, dis = capi.refine(rows, metric, q, cand, 200)
    if metric == L2:
        assert ids[0, :40].tolist() == sorted(copies.tolist()) and (dis[0, :40] == 0).all()  # equal distances: label order
        bad = set(rest[:7].tolist())  # NaN, inf and overflowing rows are never strictly better than FLT_MAX
        assert not bad & set(ids[0].tolist()) and (ids[0, 193:] == -1).all() and (ids[0, :193] >= 0).all()
    else:
        at = [ids[0].tolist().index(int(c)) for c in sorted(copies.tolist())]
        assert at == list(range(at[0], at[0] + 40))  # one run, in label order
    assert (ids[2] == -1).all()  # NaN never enters
    assert (dis[2] == (-FLT_MAX if metric == IP else FLT_MAX)).all()
    rows.close()


# ---------------------------------------------------------------------------------------- 4. the store

@pytest.mark.parametrize("placement", [DEV, PIN])
@pytest.mark.parametrize("normalize", [False, True])
def test_chunked_appends_equal_one_append(normalize, placement):
    import torch
    metric = COS if normalize else L2
    dim, n = 67, 2016
    x = data(dim)[0][:n].copy()
    x[5] = 0  # a row below FLT_EPSILON stays as it is
    one = store_of(x, metric, placement)
    many = capi.Rows(dim, n + 3, normalize=normalize, placement=placement)
    dx = torch.from_numpy(x).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    at = 0
    for cnt, mem in ((1, "host"), (7, "host"), (1000, "host"), (1, "device"), (7, "device"), (1000, "device")):
        if mem == "host":
            many.append(x[at:at + cnt])
        else:
            many.append(dx.data_ptr() + at * dim * 4, n=cnt, mem=capi.MEM_DEVICE)
        at += cnt
        assert many.num == at
    assert at == n and one.num == n
    q = np.repeat(data(dim)[1][:1], 8, axis=0)
    cand = np.arange(n, dtype=np.int64).reshape(8, 252)  # every row's distance comes back
    exp = ref_refine(x, q, cand, 252, metric)
    same(capi.refine(one, metric, q, cand, 252), exp)
    same(capi.refine(many, metric, q, cand, 252), exp)
    one.close()
    many.close()


def test_store_limits_and_errors():
    x, q, cand = data(67)
    assert code_of(lambda: capi.Rows(0, 10)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.Rows(8193, 10)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.Rows(8, 10, placement=2)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.Rows(8, 2 ** 32)) == capi.ERR_ID_RANGE
    for placement in (DEV, PIN):
        rows = capi.Rows(67, 10, placement=placement)
        assert rows.memory_usage == (10 * 68 * 4 if placement == DEV else 0)  # device bytes: a pinned store's rows are not
        rows.append(x[:8])
        assert code_of(lambda: rows.append(x[8:11])) == capi.ERR_INVALID_ARGUMENT  # beyond the capacity: nothing is appended
        assert rows.num == 8
        c = np.array([[7, 8, 9, 3]], np.int64)  # labels 8 and 9 are within the capacity, but no row yet
        same(capi.refine(rows, L2, q[:1], c, 4), ref_refine(x[:8], q[:1], c, 4, L2))
        rows.append(x[8:10])
        assert rows.num == 10
        assert code_of(lambda: rows.append(x[:1])) == capi.ERR_INVALID_ARGUMENT
        c = np.array([[9, 10, 3, -1]], np.int64)  # label 10 is the capacity: no such row
        same(capi.refine(rows, L2, q[:1], c, 4), ref_refine(x[:10], q[:1], c, 4, L2))
        rows.close()
    plain, unit = store(67, False, DEV), store(67, True, DEV)
    c = cand[:2, :10]
    assert code_of(lambda: capi.refine(plain, COS, q[:2], c, 5)) == capi.ERR_INVALID_ARGUMENT  # cosine needs normalize=1
    assert code_of(lambda: capi.refine(unit, L2, q[:2], c, 5)) == capi.ERR_INVALID_ARGUMENT    # ... and L2 / IP normalize=0
    assert code_of(lambda: capi.refine(unit, IP, q[:2], c, 5)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.refine(plain, capi.METRIC_HAMMING, q[:2], c, 5)) == capi.ERR_NOT_IMPLEMENTED
    big = np.zeros((2, 1025), np.int64)
    assert code_of(lambda: capi.refine(plain, L2, q[:2], big, 5)) == capi.ERR_UNSUPPORTED_K    # kc = 1025
    assert code_of(lambda: capi.refine(plain, L2, q[:2], c, 257)) == capi.ERR_UNSUPPORTED_K    # k = 257
    assert code_of(lambda: device_refine(plain, L2, q[:2], big, 5)) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: device_refine(plain, L2, q[:2], c, 257)) == capi.ERR_UNSUPPORTED_K
    same(capi.refine(plain, L2, q[:2], big[:, :1024], 256), ref_refine(x, q[:2], big[:, :1024], 256, L2))  # the limits themselves
    ids, dis = capi.refine(plain, L2, q[:0], c[:0], 5)  # nq = 0 and k = 0 are no-ops
    assert ids.shape == (0, 5)
    ids, dis = capi.refine(plain, L2, q[:2], c, 0)
    assert ids.shape == (2, 0)
    assert lib_refine_null(plain) == capi.ERR_INVALID_ARGUMENT


def lib_refine_null(rows):
    import ctypes as C
    one = np.zeros(67, F)
    out_i, out_d = np.zeros(1, np.int64), np.zeros(1, F)
    lib = capi.lib()
    args = lambda r, qq, cc: (r, L2, qq, C.c_size_t(1), cc, C.c_size_t(1), C.c_size_t(1), capi._p(out_i, C.c_int64), capi._p(out_d, C.c_float))
    codes = {lib.msvs_refine(*args(None, capi._p(one, C.c_float), capi._p(out_i, C.c_int64))),
             lib.msvs_refine(*args(rows._h, None, capi._p(out_i, C.c_int64))),
             lib.msvs_refine(*args(rows._h, capi._p(one, C.c_float), None))}
    assert len(codes) == 1
    return codes.pop()


# ---------------------------------------------------------------------------------------- 5. the composed entries

KINDS = [("sq", ""), ("pq", "m=16"), ("pq", "m=16,bit_size=4"), ("pq", "m=16,query_tables=1"), ("pq", "m=16,bit_size=4,query_tables=1")]


@functools.lru_cache(maxsize=None)
def coded_data():
    rng = np.random.default_rng(51)
    centres, x = blobs(rng, 2000, 64, 8)
    q = (centres[rng.integers(0, 8, 20)] + F(0.3) * rng.standard_normal((20, 64), dtype=F)).astype(F)
    return x, q, rng.random(2000) < 0.5


def device_search_refine(ix, rows, q, k, kc, nprobe, alive=None):
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
    ix.search_refine_device(rows, dq.data_ptr(), len(q), k, kc, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream,
                            d_alive=bits, nbits=nbits)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


@pytest.mark.parametrize("kind,params", KINDS)
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_search_refine_is_refine_of_search(metric, kind, params):
    x, q, half = coded_data()
    cls = capi.SqIndex if kind == "sq" else capi.PqIndex
    ix = cls(metric, 64, ",".join(p for p in ("ncentroids=8,kmeans_iters=3", params) if p))
    ix.train(x)
    ix.add(x[:700])  # labels are the staging positions: row i of the store
    ix.add(x[700:])
    ix.build()
    rows = store_of(x, metric)
    for alive in (None, half):
        first, _ = ix.search(q, 100, "nprobe=4", alive=alive)
        assert (first >= 0).sum() > 20 * 50
        got = ix.search_refine(rows, q, 10, 100, "nprobe=4", alive=alive)
        same(got, capi.refine(rows, metric, q, first, 10))
        same(got, ref_refine(x, q, first, 10, metric))
        same(device_search_refine(ix, rows, q, 10, 100, 4, alive=alive), got)
        if alive is not None:
            assert half[got[0][got[0] >= 0]].all()
    # a second call with another shape on the same stream reuses the arenas
    same(ix.search_refine(rows, q[:3], 100, 100, "nprobe=8"), capi.refine(rows, metric, q[:3], ix.search(q[:3], 100, "nprobe=8")[0], 100))
    wrong_dim = capi.Rows(32, 10, normalize=metric == COS)
    wrong_form = capi.Rows(64, 10, normalize=metric != COS)
    assert code_of(lambda: ix.search_refine(wrong_dim, q, 10, 100)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ix.search_refine(wrong_form, q, 10, 100)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ix.search_refine(rows, q, 11, 10)) == capi.ERR_INVALID_ARGUMENT      # k <= kc
    assert code_of(lambda: ix.search_refine(rows, q, 10, 257)) == capi.ERR_UNSUPPORTED_K        # the first stage's limit
    assert code_of(lambda: device_search_refine(ix, wrong_dim, q, 10, 100, 4)) == capi.ERR_INVALID_ARGUMENT
    for h in (wrong_dim, wrong_form, rows, ix):
        h.close()


# ---------------------------------------------------------------------------------------- 6. recall, the point of it all

@pytest.mark.parametrize("metric", [L2, IP])
def test_refined_recall_against_the_original_rows(metric):
    """The data of test_pq_ivf.test_recall_against_the_original_rows exactly (seed 11, 4000 x 64, 8 blobs, m = 16, every list
    probed, 100 queries).  Recall@10 of search_refine(k=10, kc=100) against the f64 truth must be >= 0.95 -- asserted first for the
    reference chain, that test's ref_search(..., 100) followed by oracle.knn over its labels.  By construction it is that test's
    "10 in 100" share (a numpy restatement gives 0.992 - 1.000)."""
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
    rows = store_of(x, metric)

    def recall(ids):
        return np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, ids)])

    first = ref_search(exp, decoded(exp), q, nlist, 100, metric)[0]
    ref = ref_refine(x, q, first, 10, metric)
    print("reference chain: recall@10 %.3f" % recall(ref[0]))
    assert recall(ref[0]) >= 0.95
    got = ix.search_refine(rows, q, 10, 100, "nprobe=%d" % nlist)
    print("search_refine: recall@10 %.3f (the first stage alone: %.3f)" % (recall(got[0]), recall(ix.search(q, 10, "nprobe=%d" % nlist)[0])))
    assert recall(got[0]) >= 0.95
    same(got, ref)
    pinned = store_of(x, metric, PIN)
    same(ix.search_refine(pinned, q, 10, 100, "nprobe=%d" % nlist), ref)
    for h in (pinned, rows, ix):
        h.close()
