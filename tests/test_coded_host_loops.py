"""The host code around the coded indexes' kernels (coded_ivf.hpp, sq_index.hip, pq_index.hip, the search loop of binary.hip) at the
sizes where its loops take a second pass, and the one piece of arithmetic that had no reference:

a. the IVFPQ sub-codebooks against the IVFFLAT trainer run on numpy residual slices (test_ivf_build.py pins that trainer by hand);
b. training over more rows than one step (CODED_ADD_ROWS = 65536) and than the trainer's cap (PQ_TRAIN_ROWS = 262144: the evenly
   spaced pick), from host and from device memory; the IVFSQ range accumulated over three steps;
c. one add of more rows than a step against adds of at most 40000 rows (the path the other files pin), from host memory and with
   rows, labels and codebook in device memory;
d. searches whose queries take three rounds (127 + 127 + 1), counted by the profile, for IVFSQ, IVFPQ (8 and 4 bits) and the binary index;
e. the device entry on a stream that is not the current one;
f. four host threads searching one index at once.

The references are the ones of test_pq_ivf.py, test_sq_ivf.py, test_bin_ivf.py and ivf_build_ref.py.  Every comparison is == on ids
and on the uint32 view of floats; codes and exports byte for byte."""
import contextlib
import functools
import threading

import numpy as np
import pytest

import ivf_build_ref as R
import myscaledb_amd.capi as capi
import test_bin_ivf as bi
import test_pq4_ivf as pq4
import test_pq_ivf as pq
import test_sq_ivf as sq

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
HAMMING, JACCARD = capi.METRIC_HAMMING, capi.METRIC_JACCARD
STEP = 65536     # CODED_ADD_ROWS
CAP = 262144     # PQ_TRAIN_ROWS
SEED = 4321


def make(kind, metric, dim, m=None, extra=""):
    """kind: "sq" / "pq8" / "pq4" """
    if kind == "sq":
        return capi.SqIndex(metric, dim, extra)
    own = "m=%d,bit_size=%d" % (m, 8 if kind == "pq8" else 4)
    return capi.PqIndex(metric, dim, extra + "," + own if extra else own)


def lists_part(exp):
    """(list offsets, codes, labels) of an SqIndex or PqIndex export"""
    return exp[-3], exp[-2], exp[-1]


def same_exports(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()


def on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def flat_centroids(metric, x, params):
    """the centroids the IVFFLAT trainer gives for the rows x (an export needs a built index: one row is added)"""
    x = np.ascontiguousarray(x, F)
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, x.shape[1], params)
    ix.train(x)
    ix.add(x[:1])
    ix.build()
    cent = ix.export(with_vecs=False)[0]
    ix.close()
    return cent


# ---------------------------------------------------------------------------------------- a. the PQ trainer

def check_pq_codebooks(ix, x, pick, metric, sub_params):
    """`ix` trained on x: its rows are added and built, the list of every row read from the export; then every sub-codebook must be,
    to the bit, what the IVFFLAT trainer gives for fl(stored(x) - cent[list]) of the rows `pick`, cut to the sub-space's columns."""
    n = len(x)
    cent, cb = ix.export(with_lists=False)[:2]
    ix.add(x)
    ix.build()
    exp = ix.export()
    assert exp[0].tobytes() == cent.tobytes() and exp[1].tobytes() == cb.tobytes()
    lists = R.lists_of_ids(exp[2], exp[4], n)
    res = (pq.stored(x, metric)[pick] - cent[lists[pick]]).astype(F)
    m, ksub, dsub = cb.shape
    assert ksub == 1 << ix.bits and m * dsub == x.shape[1]
    for s in range(m):
        want = flat_centroids(L2, res[:, s * dsub:(s + 1) * dsub], "%s,ncentroids=%d" % (sub_params, ksub))
        assert want.shape == (ksub, dsub)
        R.check_bit_equal(cb[s], want)
    return cent, cb


@pytest.mark.parametrize("dim,m", [(20, 5), (64, 16), (5, 1)])
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_pq_codebooks_are_the_ivfflat_trainer_on_residual_slices(metric, bits, dim, m):
    rng = np.random.default_rng(1000 * metric + 100 * bits + dim)
    _, x = pq.blobs(rng, 3000, dim, 8)
    base = "ncentroids=8,kmeans_iters=3,seed=%d" % SEED
    ix = capi.PqIndex(metric, dim, "%s,m=%d,bit_size=%d" % (base, m, bits))
    ix.train(x)
    cent, _ = check_pq_codebooks(ix, x, np.arange(len(x)), metric, "kmeans_iters=3,seed=%d" % SEED)
    ix.close()
    R.check_bit_equal(cent, flat_centroids(metric, x, base))  # the coarse part: the same trainer with the index's own metric


# ---------------------------------------------------------------------------------------- b. training past one step, past the cap

@functools.lru_cache(maxsize=None)
def steps_in_sample(n, ns, seed):
    """the 65536-row steps the trainer's sample of ns of n rows takes rows from"""
    return frozenset((R.train_sample(n, ns, seed) // STEP).tolist())


@pytest.mark.parametrize("n", [70000, 300000])  # two residual steps and no pick; the cap: four steps of picked rows
@pytest.mark.parametrize("bits", [4, 8])
def test_pq_training_past_one_step_and_past_the_cap(bits, n):
    dim, m, ksub = 4, 2, 1 << bits
    cap = min(n, CAP)
    # a condition of the input, not of the result: the sub-trainer's sample draws from every step of the residual buffer
    assert steps_in_sample(cap, min(cap, 64 * ksub), SEED) == frozenset(range(-(-cap // STEP)))
    pick = np.arange(cap, dtype=np.int64) * n // cap
    assert pick[0] == 0 and pick[-1] < n and (np.diff(pick) >= 1).all() and ((pick != np.arange(cap)).any() == (cap < n))
    _, x = pq.blobs(np.random.default_rng(n + bits), n, dim, 8)
    params = "ncentroids=8,kmeans_iters=2,seed=%d,m=%d,bit_size=%d" % (SEED, m, bits)
    host = capi.PqIndex(L2, dim, params)
    host.train(x)
    dx = on_device(x)
    dev = capi.PqIndex(L2, dim, params)
    dev.train(dx.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    same_exports(host.export(with_lists=False)[:2], dev.export(with_lists=False)[:2])
    dev.close()
    check_pq_codebooks(host, x, pick, L2, "kmeans_iters=2,seed=%d" % SEED)
    host.close()


def test_sq_range_is_accumulated_over_three_steps():
    """Steps of 65536, 65536 and 1 rows: the smallest residual of column 1 is in the first row of the second step, the largest of
    column 3 in the only row of the third."""
    n, dim = 2 * STEP + 1, 5
    low, high = STEP, n - 1
    params = "ncentroids=8,kmeans_iters=2,seed=%d" % SEED
    # a condition of the input: neither row is in the k-means sample (it would pull a centroid towards itself)
    assert not {low, high} & set(R.train_sample(n, 64 * 8, SEED).tolist())
    _, x = sq.blobs(np.random.default_rng(17), n, dim, 8)
    x[low, 1] = F(-50)
    x[high, 3] = F(50)
    host = capi.SqIndex(L2, dim, params)
    host.train(x)
    dx = on_device(x)
    dev = capi.SqIndex(L2, dim, params)
    dev.train(dx.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    same_exports(host.export(with_lists=False)[:3], dev.export(with_lists=False)[:3])
    dev.close()
    host.add(x)
    host.build()
    cent, lo, hi, off, _, labels = host.export()
    host.close()
    r = (x - cent[R.lists_of_ids(off, labels, n)]).astype(F)
    assert r[:, 1].argmin() == low and r[:, 3].argmax() == high
    assert lo.tobytes() == r.min(axis=0).tobytes() and hi.tobytes() == r.max(axis=0).tobytes()


# ---------------------------------------------------------------------------------------- c. adding past one step

N_ADD = 2 * STEP + 1


@pytest.mark.parametrize("kind,metric", [("sq", L2), ("pq8", L2), ("pq4", L2), ("pq8", IP)])
def test_add_of_more_rows_than_a_step(kind, metric):
    rng = np.random.default_rng(len(kind) * 10 + metric + (kind == "pq4"))
    n, dim, m = N_ADD, (5 if kind == "sq" else 6), 3  # IVFSQ: rows of 16 floats on the device, IVFPQ: of 8
    cent = R.int_rows(rng, 8, dim, -8, 8)
    x = rng.integers(-8, 9, (n, dim)).astype(F)
    labels = rng.permutation(3 * n)[:n].astype(np.int64)  # shuffled, not contiguous
    if kind == "sq":
        book = (np.full(dim, -20, F), np.full(dim, 20, F))
    else:
        book = ((pq.random_codebooks if kind == "pq8" else pq4.codebooks16)(rng, m, dim // m, 3.0),)

    def index():
        ix = make(kind, metric, dim, m)
        ix.set_codebook(cent, *book)
        return ix

    def built(ix):
        ix.build()
        assert ix.num_data == n
        exp = ix.export()
        ix.close()
        return exp

    ix = index()  # B: the rows in calls of at most 40000
    for r0 in range(0, n, 40000):
        ix.add(x[r0:r0 + 40000], labels[r0:r0 + 40000])
    exp_b = built(ix)
    ix = index()  # A: in one call
    ix.add(x, labels)
    same_exports(built(ix), exp_b)
    ix = index()  # exactly one step, then one step and a row
    ix.add(x[:STEP], labels[:STEP])
    ix.add(x[STEP:], labels[STEP:])
    same_exports(built(ix), exp_b)
    dx, dl = on_device(x), on_device(labels)
    dbook = [on_device(cent)] + [on_device(b) for b in book]
    ix = make(kind, metric, dim, m)  # A from device memory, the labels and the codebook there too
    ix.set_codebook(*[t.data_ptr() for t in dbook], nlist=len(cent), mem=capi.MEM_DEVICE)
    ix.add(dx.data_ptr(), dl.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    same_exports(built(ix), exp_b)
    ix = index()  # no labels: the staging positions, over two calls
    ix.add(dx.data_ptr(), None, n=STEP + 1, mem=capi.MEM_DEVICE)
    ix.add(dx[STEP + 1:].data_ptr(), n=n - STEP - 1, mem=capi.MEM_DEVICE)
    exp_p = built(ix)

    # B against the references: the list of every row, the codes of the rows around both step boundaries and of a sample
    off, codes, elab = lists_part(exp_b)
    row_of = np.full(3 * n, -1, np.int64)
    row_of[labels] = np.arange(n)
    rows = row_of[elab]  # the fed row of every exported row
    assert sorted(rows.tolist()) == list(range(n))
    lists, codes_of = np.empty(n, np.int64), np.empty((n, codes.shape[1]), np.uint8)
    lists[rows] = sq.lists_of(off)
    codes_of[rows] = codes
    for l in range(8):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    R.check_exact(lists, R.exact_assign(x, cent, metric == IP))
    some = np.unique(np.concatenate([np.arange(64), np.arange(STEP - 64, STEP + 64), np.arange(2 * STEP - 64, n), rng.integers(0, n, 2000)]))
    want = (sq.encode if kind == "sq" else pq.encode)(x[some], cent[lists[some]], *book)
    assert want.shape == codes_of[some].shape and (codes_of[some] == want).all()
    # the index without labels: the same lists and codes under the labels 0 .. n - 1
    off_p, codes_p, elab_p = lists_part(exp_p)
    R.check_exact(R.lists_of_ids(off_p, elab_p, n), lists)
    by_pos = np.empty_like(codes_of)
    by_pos[elab_p] = codes_p
    assert by_pos.tobytes() == codes_of.tobytes()
    for a, b in zip(exp_p[:-3], exp_b[:-3]):  # (the codebook)
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------- d. searches of three rounds

# 64 lists, one of 4000 rows: with 256-row segments seg_max = 16, and with nprobe = 64 and k = 256 a query's partial lists take
# 64 * 16 * 256 * 8 = 2 MiB, so a round of at most 256 MiB holds 127 queries: 255 queries are rounds of 127, 127 and 1.  The tests do
# not trust this arithmetic: the profile must count three scan launches per search.
SIZES = [4000] + [15] * 63
NQ, K, NPROBE = 255, 256, 64
KNOB = {"sq": "sq_ivf_rpb", "pq8": "pq_ivf_rpb", "pq4": "pq_ivf_rpb", "bin": "bin_ivf_rpb"}
SCAN = {"sq": "sq_ivf_scan", "pq8": "pq_ivf_scan", "pq4": "pq_ivf_scan", "bin": "bin_ivf_scan"}


@contextlib.contextmanager
def three_rounds(kind):
    """256-row segments and the profile on; -> run(fn): fn() under a count of the kind's scan launches, which must be 3"""
    def run(fn):
        capi.profile_reset()
        out = fn()
        assert capi.profile_get(SCAN[kind])[0] == 3
        return out

    capi.set_option(KNOB[kind], 256)
    capi.profile_enable(True)
    try:
        yield run
    finally:
        capi.set_option(KNOB[kind])
        capi.profile_enable(False)
        capi.release_scratch()  # (a round's arena is about 256 MB)


def half_alive(rng, labels):
    """-> (a bitmap of about half the labels that ends below the largest label, the same over the whole label range)"""
    top = int(labels.max()) + 1
    nbits = 2 * top // 3
    alive = rng.random(nbits) < 0.5
    whole = np.zeros(top, bool)
    whole[:nbits] = alive
    assert (labels >= nbits).any() and 0 < whole[labels].sum() < (labels < nbits).sum()
    return alive, whole


@functools.lru_cache(maxsize=None)
def rounds_case(kind, metric):
    """An index of the lists SIZES over tight blobs at dim 16 (centres of one norm, so that the nearest centroid of a row is its own
    by L2 and by inner product; norm 1 for cosine, whose rows are stored normalised, else 10), its export, the decoded rows, 255
    queries and the references without and with a filter."""
    rng = np.random.default_rng(len(kind) + 7 * metric + (kind == "pq4"))
    dim, m, nlist = 16, 4, len(SIZES)
    unit = F(0.1 if metric == COS else 1.0)
    cent = rng.standard_normal((nlist, dim), dtype=F)
    cent = (F(10) * unit * cent / np.sqrt((cent * cent).sum(axis=1, keepdims=True))).astype(F)
    home = np.repeat(np.arange(nlist), SIZES)
    x = (cent[home] + F(0.05) * unit * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    order = rng.permutation(len(x))  # fed in no list order
    x, home = x[order], home[order]
    labels = rng.permutation(3 * len(x))[:len(x)].astype(np.int64)
    ix = make(kind, metric, dim, m)
    if kind == "sq":
        ix.set_codebook(cent, np.full(dim, -0.25 * unit, F), np.full(dim, 0.25 * unit, F))
    else:
        ix.set_codebook(cent, (pq.random_codebooks if kind == "pq8" else pq4.codebooks16)(rng, m, dim // m, 0.05 * unit))
    ix.add(x, labels)
    ix.build()
    exp = ix.export()
    assert np.diff(lists_part(exp)[0]).tolist() == SIZES
    mod = sq if kind == "sq" else pq
    xh = mod.decoded(exp)
    qhome = rng.integers(0, nlist, NQ)
    qhome[::3] = 0  # a third of the queries at the long list
    q = (cent[qhome] + F(0.05) * unit * rng.standard_normal((NQ, dim), dtype=F)).astype(F)
    alive, whole = half_alive(rng, labels)
    ref = mod.ref_search(exp, xh, q, NPROBE, K, metric)
    ref_alive = mod.ref_search(exp, xh, q, NPROBE, K, metric, alive=whole)
    assert len({r.tobytes() for r in ref[0]}) > NQ // 2  # the answers differ from query to query
    return ix, mod, exp, xh, q, alive, ref, ref_alive


ROUNDS = [("sq", L2), ("sq", COS), ("pq8", IP), ("pq4", L2)]


@pytest.mark.parametrize("kind,metric", ROUNDS)
def test_search_of_three_rounds(kind, metric):
    ix, mod, _, _, q, alive, ref, ref_alive = rounds_case(kind, metric)
    with three_rounds(kind) as run:
        mod.same(run(lambda: ix.search(q, K, "nprobe=%d" % NPROBE)), ref)
        mod.same(run(lambda: ix.search(q, K, "nprobe=%d" % NPROBE, alive=alive)), ref_alive)
        mod.same(run(lambda: mod.device_search(ix, q, K, NPROBE)), ref)
        mod.same(run(lambda: mod.device_search(ix, q, K, NPROBE, alive=alive)), ref_alive)


@pytest.mark.parametrize("metric", [HAMMING, JACCARD])
def test_binary_search_of_three_rounds(metric):
    rng = np.random.default_rng(40 + metric)
    nbytes, nlist = 16, len(SIZES)
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    rows = np.concatenate([bi.flip_noise(rng, centres[l:l + 1], s, 0.02) for l, s in enumerate(SIZES)])
    n = len(rows)
    labels = rng.permutation(3 * n)[:n].astype(np.int64)
    ix = capi.BinIndex(nbytes, metric, "ncentroids=%d" % nlist)
    ix.set_centroids(centres)
    ix.add(rows, labels)
    assert np.diff(bi.check_structure(ix, rows, labels, centres)).tolist() == SIZES
    rows_s, labels_s, lists_s = bi.by_label(rows, labels, centres)
    q = bi.flip_noise(rng, centres, NQ, 0.05)
    alive, whole = half_alive(rng, labels)
    ref = bi.ref_search(q, centres, rows_s, labels_s, lists_s, NPROBE, K, metric)
    ref_alive = bi.ref_search(q, centres, rows_s, labels_s, lists_s, NPROBE, K, metric, whole[labels_s])
    assert len({r.tobytes() for r in ref[0]}) > NQ // 2
    with three_rounds("bin") as run:
        bi.same(*run(lambda: ix.search(q, K, params="nprobe=%d" % NPROBE)), *ref)
        bi.same(*run(lambda: ix.search(q, K, alive=alive, params="nprobe=%d" % NPROBE)), *ref_alive)
    ix.close()


# ---------------------------------------------------------------------------------------- e. the device entry on a side stream

def side_stream_search(ix, q, k, nprobe):
    """The queries are computed on a stream that is not the current one, the search is enqueued there, and only that stream is waited for."""
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    di = torch.full((len(q), k), -7, device=dev, dtype=torch.int64)
    dd = torch.full((len(q), k), float("nan"), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(s):
        q2 = dq * 1
        ix.search_device(q2.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), s.cuda_stream)
    s.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


@pytest.mark.parametrize("kind,metric", [("sq", L2), ("pq8", IP), ("pq4", L2)])
def test_device_entry_on_a_side_stream(kind, metric):
    ix, mod, exp, xh, q, _, ref, _ = rounds_case(kind, metric)
    with three_rounds(kind) as run:
        mod.same(run(lambda: side_stream_search(ix, q, K, NPROBE)), ref)
    mod.same(side_stream_search(ix, q[:7], 10, 4), mod.ref_search(exp, xh, q[:7], 4, 10, metric))


# ---------------------------------------------------------------------------------------- f. concurrent callers

def float_searcher(ix):
    return lambda q, k, nprobe: ix.search(q, k, "nprobe=%d" % nprobe)


def concurrent_case(kind):
    """-> (search(q, k, nprobe), queries, number of lists) over an index the other files build and pin"""
    if kind == "sq":
        ix, _, _, _, _, q = sq.case(L2, 64, "clustered")
        return float_searcher(ix), q, sq.NLIST
    if kind == "pq8":
        ix, _, _, _, _, q = pq.case(L2, 64, 16, "clustered")
        return float_searcher(ix), q, pq.NLIST
    if kind == "pq4":
        ix, _, _, _, _, q = pq4.case(IP, 64, 16, "clustered")
        return float_searcher(ix), q, pq4.NLIST
    ix, _, q, _ = bi.parity_case(JACCARD, 64, "clustered")
    return (lambda q_, k, nprobe: ix.search(q_, k, params="nprobe=%d" % nprobe)), q, bi.NLIST


@pytest.mark.parametrize("kind", ["sq", "pq8", "pq4", "bin"])
def test_four_threads_search_one_index(kind):
    search, q, nlist = concurrent_case(kind)
    nthreads, per = 4, len(q) // 4
    shapes = [(k, nprobe) for k in (1, 10, 100) for nprobe in (1, 4, nlist)]
    mine = [q[t * per:(t + 1) * per] for t in range(nthreads)]
    want = {(t, s): search(mine[t], *s) for t in range(nthreads) for s in shapes}  # single-threaded, beforehand
    assert len({w[0].tobytes() for (t, s), w in want.items() if s == (10, 4)}) == nthreads
    errors = []

    def worker(t):
        try:
            for rep in range(20):
                s = shapes[(rep + 2 * t) % len(shapes)]
                ids, dis = search(mine[t], *s)
                wi, wd = want[t, s]
                if not ((ids == wi).all() and (dis.view(np.uint32) == wd.view(np.uint32)).all()):
                    errors.append((t, rep, s))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []
