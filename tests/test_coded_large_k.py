"""IVFSQ / IVFPQ with more than 256 results: search_rounds[_device] (k <= 4096, the list scan once per 256 ranks for the whole batch,
each round behind the last key a query has returned) and search_refine_rounds[_device] (kc <= 1024).

The references are the numpy ones of the indexes' own test files, which take any k: test_sq_ivf.ref_search, test_pq_ivf.ref_search
(both code widths), test_pq_query_tables.ref_search (query_tables=1) and test_refine.ref_refine.  Every comparison is == on ids
and on the uint32 view of the distances."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_pq4_ivf as pq4
import test_pq_ivf as pq
import test_pq_query_tables as qt
import test_sq_ivf as sq
from oracle import oracle as o
from test_pq_ivf import blobs, code_of, same
from test_refine import ref_refine, store_of

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
DEV, PIN = capi.ROWS_DEVICE, capi.ROWS_HOST_PINNED
FLT_MAX = np.finfo(np.float32).max
N, NLIST, NPROBE, M = 3000, 8, 4, 8
KINDS = ["sq", "sq264", "pq8", "pq4", "qt8", "qt4"]  # sq264: a whole 256-column block plus a tail; qt: query_tables=1
KS = [256, 257, 300, 512, 513, 1000, 4096]
NQS = [1, 5, 70]


def pad_of(metric):
    return -FLT_MAX if metric == IP else FLT_MAX  # (cosine: fl(1 - -FLT_MAX))


def reference(kind, metric, exp):
    """-> f(q, nprobe, k, alive=None): the numpy reference of the index kind over an index's export"""
    if kind.startswith("sq"):
        xh = sq.decoded(exp)
        return lambda q, nprobe, k, alive=None: sq.ref_search(exp, xh, q, nprobe, k, metric, alive)
    if kind.startswith("qt"):
        return lambda q, nprobe, k, alive=None: qt.ref_search(exp, q, nprobe, k, metric, alive)
    xh = pq.decoded(exp)
    return lambda q, nprobe, k, alive=None: pq.ref_search(exp, xh, q, nprobe, k, metric, alive)


def make(kind, metric, cent, x, labels):
    """-> (index, its reference) over the codebook given here: no training"""
    dim = cent.shape[1]
    rng = np.random.default_rng(77)
    if kind.startswith("sq"):
        ix = capi.SqIndex(metric, dim)
        ix.set_codebook(cent, np.full(dim, -1.0, F), np.full(dim, 1.0, F))
    else:
        bits = int(kind[2])
        ix = capi.PqIndex(metric, dim, "m=%d,bit_size=%d%s" % (M, bits, ",query_tables=1" if kind.startswith("qt") else ""))
        ix.set_codebook(cent, (pq.random_codebooks if bits == 8 else pq4.codebooks16)(rng, M, dim // M, 0.4))
    ix.add(x, labels)
    ix.build()
    return ix, reference(kind, metric, ix.export())


@functools.lru_cache(maxsize=None)
def case(kind, metric):
    """3000 rows around 8 centres (about 1500 candidates at nprobe 4), shuffled labels, 70 queries, a filter over half the labels"""
    dim = 264 if kind == "sq264" else 32
    rng = np.random.default_rng(dim + metric)
    cent, x = blobs(rng, N, dim, NLIST)
    labels = rng.permutation(3 * N)[:N].astype(np.int64)
    q = (cent[rng.integers(0, NLIST, 70)] + F(0.3) * rng.standard_normal((70, dim), dtype=F)).astype(F)
    alive = rng.random(3 * N) < 0.5
    ix, ref = make(kind, metric, cent, x, labels)
    return ix, functools.lru_cache(maxsize=None)(lambda nq, k, filtered: ref(q[:nq], NPROBE, k, alive if filtered else None)), q, alive


def device_rounds(ix, q, k, nprobe, alive=None):
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
    ix.search_rounds_device(dq.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream,
                            d_alive=bits, nbits=nbits)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


# ---------------------------------------------------------------------------------------- 1. parity table

def parity_table():
    """every k with three of the six index kinds, the other axes rotating beside them"""
    table = []
    for c in range(21):
        table.append((KINDS[c % 6], (L2, IP, COS)[(c + c // 6) % 3], NQS[(c + c // 3) % 3], KS[c % 7], ("host", "device")[(c + c // 7) % 2],
                      c % 4 == 1, c % 5 == 2))
    return table


PARITY = parity_table()


def test_parity_table_reaches_every_axis():
    assert {r[0] for r in PARITY} == set(KINDS) and {r[1] for r in PARITY} == {L2, IP, COS}
    assert {r[2] for r in PARITY} == set(NQS) and {r[3] for r in PARITY} == set(KS)
    assert {r[4] for r in PARITY} == {"host", "device"} and {r[5] for r in PARITY} == {False, True} and {r[6] for r in PARITY} == {False, True}
    for kind in KINDS:  # every kind beyond one round, with both entries somewhere among the kinds of its family
        assert any(r[0] == kind and r[3] > 256 for r in PARITY)
    for fam in ("sq", "pq", "qt"):
        assert {r[4] for r in PARITY if r[0].startswith(fam)} == {"host", "device"}
        assert {r[1] for r in PARITY if r[0].startswith(fam)} == {L2, IP, COS}


@pytest.mark.parametrize("kind,metric,nq,k,entry,filtered,segmented", PARITY)
def test_search_rounds_parity(kind, metric, nq, k, entry, filtered, segmented, opt):
    ix, ref, q, alive = case(kind, metric)
    if segmented:  # a list of about 375 rows in several row segments
        opt("sq_ivf_rpb", "64")
        opt("pq_ivf_rpb", "256")
    a = alive if filtered else None
    got = ix.search_rounds(q[:nq], k, "nprobe=%d" % NPROBE, a) if entry == "host" else device_rounds(ix, q[:nq], k, NPROBE, a)
    exp = ref(nq, k, filtered)
    same(got, exp)
    if k == 4096:  # more slots than candidates: the tails are pads
        assert (got[0][:, -1] == -1).all() and (got[1][:, -1] == pad_of(metric)).all() and (got[0][:, 0] >= 0).all()
    if k == 256:  # one round: the bits of search
        same(got, ix.search(q[:nq], k, "nprobe=%d" % NPROBE, a))


# ---------------------------------------------------------------------------------------- 2. boundaries

def far_centres(nlist, dim):
    cent = np.zeros((nlist, dim), F)
    cent[np.arange(nlist), np.arange(nlist)] = 10.0
    return cent


@pytest.mark.parametrize("kind,metric", [("sq", L2), ("pq8", IP), ("qt4", L2), ("pq4", COS)])
def test_a_tie_run_across_a_round_boundary(kind, metric):
    """1200 rows drawn from three vectors in two lists: runs of about 400 equal distances cross ranks 256 and 512, the labels are
    shuffled; the next round resumes inside the run, by label."""
    rng = np.random.default_rng(5)
    dim = 32
    cent = far_centres(4, dim)
    vec = (cent[[0, 0, 1]] + F(0.4) * rng.standard_normal((3, dim), dtype=F)).astype(F)
    x = np.ascontiguousarray(vec[rng.integers(0, 3, 1200)])
    labels = rng.permutation(5000)[:1200].astype(np.int64)
    ix, ref = make(kind, metric, cent, x, labels)
    q = (F(0.5) * (cent[0] + cent[1]) + F(0.2) * rng.standard_normal((5, dim), dtype=F)).astype(F)
    for k in (300, 600, 1200):
        got, exp = ix.search_rounds(q, k, "nprobe=2"), ref(q, 2, k)
        same(got, exp)
        runs = [len(np.unique(d)) for d in got[1]]
        assert max(runs) <= 3 and (got[0] >= 0).all()  # three distances at most: the boundaries fall inside runs
    for i in got[0]:  # all 1200 rows, each once
        assert sorted(i.tolist()) == sorted(labels.tolist())
    ix.close()


@pytest.mark.parametrize("kind,metric", [("sq", IP), ("pq8", L2), ("qt8", COS)])
def test_exactly_one_and_two_rounds_of_alive_rows(kind, metric):
    """every list probed and a filter that leaves exactly 256, then exactly 512 rows: the round after returns nothing"""
    ix, _, q, _ = case(kind, metric)
    exp = ix.export()
    ref = reference(kind, metric, exp)  # (case's own is bound to its nprobe and filter)
    labels = np.sort(exp[-1])
    for cnt in (256, 512):
        alive = np.zeros(3 * N, bool)
        alive[labels[::3][:cnt]] = True
        for k in (cnt + 1, 1000):
            got = ix.search_rounds(q[:5], k, "nprobe=%d" % NLIST, alive)
            same(got, ref(q[:5], NLIST, k, alive))
            assert (got[0][:, :cnt] >= 0).all() and (got[0][:, cnt:] == -1).all() and (got[1][:, cnt:] == pad_of(metric)).all()


@pytest.mark.parametrize("kind", ["sq", "pq8", "qt4"])
def test_a_query_that_finishes_early_rides_along(kind):
    """Lists of 10, 1500, 1200 and 300 rows.  Query 0 reaches 10 rows (nprobe 1) or 310 (nprobe 2: lists 0 and 3) at k = 1000 and is
    finished after the first / second round; it shares list 3's tile with queries that go on through all four rounds."""
    rng = np.random.default_rng(9)
    dim, sizes = 32, [10, 1500, 1200, 300]
    cent = far_centres(4, dim)
    home = np.repeat(np.arange(4), sizes)
    x = (cent[home] + F(0.3) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    labels = rng.permutation(9000)[:len(home)].astype(np.int64)
    ix, ref = make(kind, L2, cent, x, labels)
    assert np.diff(ix.export()[-3]).tolist() == sizes
    near = lambda a, b: (F(0.7) * cent[a] + F(0.3) * cent[b]).astype(F)  # nearest list a, then b
    q = np.stack([near(0, 3), near(3, 1), near(1, 3), near(3, 2), near(2, 1), near(0, 3)])
    q = (q + F(0.05) * rng.standard_normal(q.shape, dtype=F)).astype(F)
    for nprobe, reach in ((1, 10), (2, 310)):
        got = ix.search_rounds(q, 1000, "nprobe=%d" % nprobe)
        same(got, ref(q, nprobe, 1000))
        for i in (0, 5):
            assert (got[0][i, :reach] >= 0).all() and (got[0][i, reach:] == -1).all() and (got[1][i, reach:] == FLT_MAX).all()
        assert (got[0][2] >= 0).all()  # 1500 rows and more: full
    ix.close()


@pytest.mark.parametrize("kind,metric", [("sq", L2), ("pq8", COS), ("qt8", IP), ("pq4", COS)])
def test_a_nan_query_and_an_all_dead_filter_give_pads(kind, metric):
    ix, ref, q, alive = case(kind, metric)
    qn = q[:5].copy()
    qn[2] = np.nan
    ids, dis = ix.search_rounds(qn, 600, "nprobe=%d" % NPROBE)
    assert (ids[2] == -1).all() and (dis[2] == pad_of(metric)).all()
    exp = ref(5, 600, False)
    keep = [0, 1, 3, 4]
    same((ids[keep], dis[keep]), (exp[0][keep], exp[1][keep]))
    ids, dis = ix.search_rounds(q[:5], 600, "nprobe=%d" % NPROBE, np.zeros(3 * N, bool))
    assert (ids == -1).all() and (dis == pad_of(metric)).all()
    ids, dis = device_rounds(ix, qn, 300, NPROBE, np.zeros(3 * N, bool))
    assert (ids == -1).all() and (dis == pad_of(metric)).all()


# ---------------------------------------------------------------------------------------- 3. the two-stage search

@functools.lru_cache(maxsize=None)
def refine_case(kind, metric):
    """rows whose label is their position (the row store's rule), 20 queries near the rows"""
    rng = np.random.default_rng(300 + metric)
    dim = 32
    cent, x = blobs(rng, N, dim, NLIST)
    q = (x[rng.integers(0, N, 20)] + F(0.2) * rng.standard_normal((20, dim), dtype=F)).astype(F)
    ix, ref = make(kind, metric, cent, x, None)
    return ix, ref, x, q


@functools.lru_cache(maxsize=None)
def refine_store(kind, metric, placement):
    return store_of(refine_case(kind, metric)[2], metric, placement)


def device_refine_rounds(ix, rows, q, k, kc, nprobe):
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    di = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    dd = torch.empty((len(q), k), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix.search_refine_rounds_device(rows, dq.data_ptr(), len(q), k, kc, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


REFINE = [  # kc, k, kind, metric, store, entry
    (257, 10, "sq", L2, DEV, "host"), (257, 256, "pq8", COS, PIN, "device"), (512, 10, "qt4", IP, DEV, "device"),
    (512, 256, "sq", L2, PIN, "host"), (1024, 10, "pq8", COS, DEV, "host"), (1024, 256, "qt4", IP, PIN, "device"),
]


@pytest.mark.parametrize("kc,k,kind,metric,placement,entry", REFINE)
def test_search_refine_rounds(kc, k, kind, metric, placement, entry):
    ix, ref, x, q = refine_case(kind, metric)
    rows = refine_store(kind, metric, placement)
    got = (ix.search_refine_rounds(rows, q, k, kc, "nprobe=%d" % NPROBE) if entry == "host"
           else device_refine_rounds(ix, rows, q, k, kc, NPROBE))
    cand = ix.search_rounds(q, kc, "nprobe=%d" % NPROBE)[0]
    same(got, capi.refine(rows, metric, q, cand, k))
    same(got, ref_refine(x, q, ref(q, NPROBE, kc)[0], k, metric))


def test_search_refine_rounds_within_one_round_is_search_refine():
    ix, ref, x, q = refine_case("sq", L2)
    rows = refine_store("sq", L2, DEV)
    same(ix.search_refine_rounds(rows, q, 10, 256, "nprobe=%d" % NPROBE), ix.search_refine(rows, q, 10, 256, "nprobe=%d" % NPROBE))


# ---------------------------------------------------------------------------------------- 4. what the larger first stage buys

def recall_data():
    """4000 x 64 in 8 blobs, four sub-quantisers of random entries: a coarse code, whose first 256 candidates miss true neighbours
    that the first 1024 hold.  (Checked on the reference alone, with a numpy assignment and encode, before the seed was fixed:
    recall@10 0.853 at kc = 256, 0.990 at 1024.)"""
    rng = np.random.default_rng(2024)
    cent, x = blobs(rng, 4000, 64, NLIST, sigma=2.0)
    q = (x[rng.integers(0, 4000, 30)] + F(0.25) * rng.standard_normal((30, 64), dtype=F)).astype(F)
    cb = pq.random_codebooks(rng, 4, 16, 1.0)
    return cent, x, q, cb


def recall10(ids, truth):
    return np.mean([len(set(a.tolist()) & set(b.tolist())) / 10.0 for a, b in zip(ids, truth)])


def test_recall_grows_with_the_first_stage():
    cent, x, q, cb = recall_data()
    ix = capi.PqIndex(L2, 64, "m=4")
    ix.set_codebook(cent, cb)
    ix.add(x)
    ix.build()
    exp = ix.export()
    xh = pq.decoded(exp)
    rows = store_of(x, L2)
    truth = o.knn(q, x, 10, o.METRIC_L2)[0]
    rec = {}
    for kc in (256, 1024):
        got = ix.search_refine_rounds(rows, q, 10, kc, "nprobe=%d" % NLIST)
        same(got, ref_refine(x, q, pq.ref_search(exp, xh, q, NLIST, kc, L2)[0], 10, L2))
        rec[kc] = recall10(got[0], truth)
    print("recall@10: kc=256 %.3f, kc=1024 %.3f" % (rec[256], rec[1024]))
    assert rec[1024] > rec[256]
    ix.close()
    rows.close()


# ---------------------------------------------------------------------------------------- 5. errors

@pytest.mark.parametrize("kind", ["sq", "pq8"])
def test_limits_and_errors(kind):
    ix, _, x, q = refine_case(kind, L2)
    rows = refine_store(kind, L2, DEV)
    q = q[:2]
    assert code_of(lambda: ix.search_rounds(q, 4097, "nprobe=2")) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: device_rounds(ix, q, 4097, 2)) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search_refine_rounds(rows, q, 10, 1025, "nprobe=2")) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search_refine_rounds(rows, q, 257, 512, "nprobe=2")) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: device_refine_rounds(ix, rows, q, 257, 512, 2)) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search_refine_rounds(rows, q, 200, 100, "nprobe=2")) == capi.ERR_INVALID_ARGUMENT  # k > kc
    assert code_of(lambda: ix.search_rounds(q, 300, "nprobe=0")) == capi.ERR_INVALID_ARGUMENT
    other = store_of(x[:, :16].copy(), L2)  # a row store of another dimension
    assert code_of(lambda: ix.search_refine_rounds(other, q, 10, 512, "nprobe=2")) == capi.ERR_INVALID_ARGUMENT
    other.close()
    # the one-round entries keep their limits
    assert code_of(lambda: ix.search(q, 257, "nprobe=2")) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search_refine(rows, q, 10, 257, "nprobe=2")) == capi.ERR_UNSUPPORTED_K
    ids, dis = ix.search_rounds(q, 0)  # k = 0: nothing to return
    assert ids.shape == (2, 0)
    new = capi.SqIndex(L2, 32) if kind == "sq" else capi.PqIndex(L2, 32, "m=8")
    assert code_of(lambda: new.search_rounds(q, 300)) == capi.ERR_NOT_READY
    assert code_of(lambda: new.search_refine_rounds(rows, q, 10, 300)) == capi.ERR_NOT_READY
    new.close()
