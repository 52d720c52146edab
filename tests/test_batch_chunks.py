"""Batches larger than one chunk through the host loops that cut the queries of a search: every loop offsets queries, scratch and
output rows by q0 and plans the tail chunk again at its own size, and a slip there corrupts every query from q0 on.

1. index_search_device (msvs_capi.hip): sub-batches of 2^21 (query, probe) pairs -- 8192 queries at nprobe = 256 -- through the host
   and the device entry (on a stream that is not the current one), three metrics, no filter / a bitmap / a delete bitmap / the
   compacted view;
2. the same loop at the smaller cut of an index with the int8 residual shadow (384 MiB of pair or query images), one case a metric;
3. the slices of 32768 queries of ivf_scan_kernel (queries on grid.z);
4. more than 65535 query tiles on grid.y of flat_scan_kernel: a FLAT index, the brute-force knn, the coarse step of IVFFLAT and IVFSQ;
5. the BM25 batch entry (bm25.hip): chunks of about 7.2 k queries at k = 256.

Every case restates its loop's cut and asserts nq > cut (a case that stays in one pass fails), and where a ProfileScope counts the
loop's launches, their number.  nq = cut + 37: the tail chunk is small and planned differently.  The queries are a few hundred
distinct vectors repeated in a shuffled order, the ones around the cut and the last one pairwise different with different answers;
the oracle runs once per distinct vector.  Every row is compared: ids ==, distances / scores by their uint32 view; device outputs
are pre-filled with -7 / NaN."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_special_values as sv
import test_sq_ivf as sq
from oracle import oracle as o

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
NAME = {L2: "l2", IP: "ip", COS: "cosine"}
METRICS = [pytest.param(m, id=NAME[m]) for m in (L2, IP, COS)]
TAIL = 37
MAX_PAIRS = 1 << 21  # index_search_device: (query, probe) pairs of one sub-batch


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------- helpers

def straddle(rng, nq, cut, ndist):
    """-> pick[nq]: which of ndist distinct queries sits at every position; positions cut - 2 .. cut + 2 hold the distinct queries
    0 .. 4 and the last two positions 5 and 6, so the neighbours of the cut and the last row differ from one another."""
    assert 2 <= cut and cut + 3 <= nq - 2 and ndist >= 7
    pick = rng.integers(0, ndist, nq)
    pick[cut - 2:cut + 3] = np.arange(5)
    pick[nq - 2:] = (5, 6)
    return pick


def answers_differ(ref):
    """the references of the distinct queries 0 .. 6 (the ones around the cut and at the end) are pairwise different"""
    ri, rd = ref
    assert len({ri[j].tobytes() + rd[j].tobytes() for j in range(7)}) == 7


def check(got, ref, pick, cut, what):
    """every row of got == the reference of its distinct query"""
    (gi, gd), ei, ed = got, ref[0][pick], ref[1][pick]
    assert gi.shape == ei.shape and gd.shape == ed.shape, what
    gu, eu = np.ascontiguousarray(gd).view(np.uint32), ed.view(np.uint32)
    bad = np.flatnonzero((gi != ei).any(axis=1) | (gu != eu).any(axis=1))
    if len(bad):
        r = int(bad[0])
        raise AssertionError("%s: %d of %d rows differ from the reference, %d of them before the cut at %d; first %d, last %d; row %d: "
                             "got %s %s, reference %s %s" % (what, len(bad), len(pick), int((bad < cut).sum()), cut, r, int(bad[-1]), r,
                                                             gi[r].tolist(), gd[r].tolist(), ei[r].tolist(), ed[r].tolist()))


@functools.lru_cache(maxsize=None)
def side_stream():
    import torch
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    return s


def device_search(ix, q, k, nprobe, alive=None, flt=None):
    """msvs_index_search_device / msvs_index_search_filter_device: the queries are computed on a stream that is not the current one,
    the search is enqueued there and only that stream is waited for; outputs pre-filled with -7 / NaN"""
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).cuda()
    di = torch.full((len(q), k), -7, device="cuda", dtype=torch.int64)
    dd = torch.full((len(q), k), float("nan"), device="cuda", dtype=torch.float32)
    bits, nbits = 0, 0
    if alive is not None:
        db = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).cuda()
        bits, nbits = db.data_ptr(), len(alive)
    torch.cuda.synchronize()
    s = side_stream()
    with torch.cuda.stream(s):
        q2 = dq * 1
        if flt is not None:
            ix.search_filter_device(q2.data_ptr(), len(q), k, nprobe, flt, di.data_ptr(), dd.data_ptr(), s.cuda_stream)
        else:
            ix.search_device(q2.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), s.cuda_stream, d_alive=bits, nbits=nbits)
    s.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


@contextlib.contextmanager
def profile():
    """-> run(fn) = (fn(), count(name)): how often a ProfileScope ran inside fn"""
    def run(fn):
        capi.profile_reset()
        res = fn()
        return res, lambda name: capi.profile_get(name)[0]

    capi.profile_enable(True)
    try:
        yield run
    finally:
        capi.profile_enable(False)
        capi.profile_reset()


def shadow_form(ix):
    capi.lib().msvs_debug_shadow_form.restype = C.c_int
    return capi.lib().msvs_debug_shadow_form(ix._h)


def shadow_scan_on_record(nq):
    """msvs_debug_h16_keys: whether this thread's last recorded shadow list scan was one of nq queries (a record that matches is retired
    by the call, one that does not stays)"""
    keys, cnt = np.zeros((nq, 1), np.uint64), np.zeros(nq, np.uint32)
    return capi.lib().msvs_debug_h16_keys(keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(1), cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          C.c_size_t(nq)) == 0


def planned_tiles():
    """msvs_debug_planned_tiles -> (query tile of this thread's last canonical table scan, of its last canonical list scan)"""
    out = np.zeros(2, np.uint32)
    assert capi.lib().msvs_debug_planned_tiles(out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0, capi.lib().msvs_last_error()
    return int(out[0]), int(out[1])


@pytest.fixture(scope="module")
def built():
    """-> get(make, metric): the case make(metric), whose first element is its index, built once for this file and closed after it"""
    made = {}

    def get(make, metric):
        if (make, metric) not in made:
            made[make, metric] = make(metric)
        return made[make, metric]

    yield get
    for case in made.values():
        case[0].close()
    capi.release_scratch()


def int_blobs(rng, nblob, n, ndist, d, spread=20, noise=3):
    """integer-valued rows and distinct queries around integer centres (L2 distances and inner products are exact); the distinct
    queries 0 .. 6 sit at the centres 0 .. 6"""
    centres = rng.integers(-spread, spread + 1, (nblob, d)).astype(F)
    x = (centres[rng.integers(0, nblob, n)] + rng.integers(-noise, noise + 1, (n, d))).astype(F)
    home = rng.integers(0, nblob, ndist)
    home[:7] = np.arange(7)
    dq = (centres[home] + rng.integers(-noise, noise + 1, (ndist, d))).astype(F)
    return centres, x, dq


# ---------------------------------------------------------------------------------------- 1. IVFFLAT: the sub-batch loop

N1, D1, NLIST1, NPROBE1, K1, NDIST1 = 4096, 16, 256, 256, 10, 300
SUB1 = max(256, MAX_PAIRS // NPROBE1)  # index_search_device: sub = max(256, max_pairs / np_eff)
NQ1 = SUB1 + TAIL


def ivf_case(metric):
    """-> (index, distinct queries, pick, bitmap, {variant: reference of the distinct queries})"""
    rng = np.random.default_rng(100 + metric)
    centres, x, dq = int_blobs(rng, NLIST1, N1, NDIST1, D1)
    ix = sv.build_ivf(x, metric, NLIST1, centroids=centres)
    assert ix.num_lists == NLIST1 and ix.num_data == N1
    alive = rng.random(N1) < 0.3
    refs = {None: sv.oracle_on_exported(ix, dq, NPROBE1, K1, metric)[:2], "alive": sv.oracle_on_exported(ix, dq, NPROBE1, K1, metric, alive=alive)[:2]}
    for ref in refs.values():
        answers_differ(ref)
    return ix, dq, straddle(rng, NQ1, SUB1, NDIST1), alive, refs


@pytest.mark.parametrize("variant", ["plain", "alive", "delete_bitmap", "view"])
@pytest.mark.parametrize("metric", METRICS)
def test_ivfflat_batch_beyond_one_sub_batch(metric, variant, built, opt):
    """8192 + 37 queries at nprobe = 256 are two sub-batches; the coarse step of this shape (256 probes: beyond the candidate
    passes of the coarse quantiser) is one canonical table scan a sub-batch, which the profile counts.  The view is built once and
    carried into both sub-batches.
    (k > 256: index_search_rounds runs one query at a time, nq = 1 at every call of index_search_device, so it never reaches this loop:
    no such case here.)"""
    ix, dq, pick, alive, refs = built(ivf_case, metric)
    assert SUB1 == 8192 and NQ1 > SUB1 and NQ1 % SUB1 == TAIL
    q = np.ascontiguousarray(dq[pick])
    params = "nprobe=%d" % NPROBE1
    what = "%s %s" % (NAME[metric], variant)
    flt = None
    try:
        if variant == "plain":
            host, dev, ref = (lambda: ix.search(q, K1, params)), (lambda: device_search(ix, q, K1, NPROBE1)), refs[None]
        elif variant == "alive":
            opt("filter_compact_below", "0")  # the bit test
            host, dev, ref = (lambda: ix.search(q, K1, params, alive=alive)), (lambda: device_search(ix, q, K1, NPROBE1, alive=alive)), refs["alive"]
        elif variant == "delete_bitmap":
            ix.set_delete_bitmap(alive)
            host, dev, ref = (lambda: ix.search(q, K1, params)), (lambda: device_search(ix, q, K1, NPROBE1)), refs["alive"]
        else:
            opt("filter_compact_below", "1")  # always the compacted view
            flt = capi.Filter.from_bool(alive)
            host, dev, ref = (lambda: ix.search(q, K1, params, alive=alive)), (lambda: device_search(ix, q, K1, NPROBE1, flt=flt)), refs["alive"]
        with profile() as run:
            for entry, fn in (("host", host), ("device", dev)):
                got, count = run(fn)
                check(got, ref, pick, SUB1, "%s %s entry" % (what, entry))
                assert count("flat_scan") == 2, "%s %s entry: %d coarse table scans, not one a sub-batch" % (what, entry, count("flat_scan"))
                assert count("filter_view") == (1 if variant == "view" else 0)
    finally:
        ix.set_delete_bitmap(None)
        if flt is not None:
            flt.close()


# ---------------------------------------------------------------------------------------- 2. the cut of an i8r index

H8_CHUNK = 128
I8R_BYTES = 384 << 20


def i8r_sub(metric, d, nprobe):
    """index_search_device for an index with the i8r shadow: the pairs whose images (L2: two a pair; inner product and cosine: two a
    query, and 12 bytes of constants a pair) fill 384 MiB"""
    nch = ceil_div(d, H8_CHUNK)
    pair_bytes = (nch * 256 if metric == L2 else 0) + 12
    query_bytes = 0 if metric == L2 else nch * 256
    max_pairs = min(MAX_PAIRS, I8R_BYTES * nprobe // (nprobe * pair_bytes + query_bytes))
    return max(256, max_pairs // nprobe)


# L2: 16 chunks and 64 probes cut at 1531 queries.  Inner product / cosine: the images are per query, so the cut is ~384 MiB / (256
# nch) queries whatever nprobe -- the fewest at the largest d whose query tile the shadow list scan holds in LDS (2432: 19 chunks)
I8R = {L2: (2048, 64, 64, 2048), IP: (2432, 8, 2, 1024), COS: (2432, 8, 2, 1024)}  # d, nlist, nprobe, n


@pytest.mark.parametrize("metric", METRICS)
def test_i8r_batch_beyond_its_own_cut(metric, opt):
    d, nlist, nprobe, n = I8R[metric]
    sub = i8r_sub(metric, d, nprobe)
    assert sub == (1531 if metric == L2 else 82375) and sub * nprobe < MAX_PAIRS  # the 384 MiB rule cuts, not the 2^21 pairs
    nq, k, ndist = sub + TAIL, 10, 100
    rng = np.random.default_rng(200 + metric)
    centres = rng.standard_normal((nlist, d), dtype=F)
    x = (centres[rng.integers(0, nlist, n)] + F(0.3) * rng.standard_normal((n, d), dtype=F)).astype(F)
    home = rng.integers(0, nlist, ndist)
    home[:7] = np.arange(7)
    dq = (centres[home] + F(0.3) * rng.standard_normal((ndist, d), dtype=F)).astype(F)
    opt("h16_form", "3" if metric == L2 else "4")
    ix = sv.build_ivf(x, metric, nlist, centroids=o.normalize_rows(centres) if metric == COS else centres)
    assert shadow_form(ix) == 3
    ref = sv.oracle_on_exported(ix, dq, nprobe, k, metric)[:2]
    answers_differ(ref)
    pick = straddle(rng, nq, sub, ndist)
    q = np.ascontiguousarray(dq[pick])
    opt("ivf_pass", "2")
    p0 = capi.prefilter_stats()
    try:
        with profile() as run:
            got, count = run(lambda: ix.search(q, k, "nprobe=%d" % nprobe))
            check(got, ref, pick, sub, "i8r %s" % NAME[metric])
            # fewer than 256 lists: the coarse step of the first sub-batch is the canonical table scan; the 37 queries of the tail (at most
            # 128 queries and 64 probes) take the self-merging launch instead (coarse_few_launch)
            assert (count("flat_scan"), count("coarse_few")) == (1, 1)
        assert capi.prefilter_stats()[0] - p0[0] == nq, "the shadow list scan did not serve every query"
        assert shadow_scan_on_record(TAIL), "the last shadow list scan was not the one of the tail sub-batch"
    finally:
        ix.close()
        capi.release_scratch()  # (inner product / cosine: 800 MB of queries and their images)


# ---------------------------------------------------------------------------------------- 3. the slices of ivf_scan_kernel

SLICE = 32768  # queries of one launch of ivf_scan_kernel (grid.z)
N3, D3, NLIST3, NDIST3, KMAX3 = 2000, 8, 8, 200, 100
NQ3 = SLICE + TAIL


def slices_case(metric):
    rng = np.random.default_rng(300 + metric)
    centres, x, dq = int_blobs(rng, NLIST3, N3, NDIST3, D3)
    ix = sv.build_ivf(x, metric, NLIST3, centroids=centres)
    refs = {nprobe: sv.oracle_on_exported(ix, dq, nprobe, KMAX3, metric)[:2] for nprobe in (1, 3)}
    return ix, dq, straddle(rng, NQ3, SLICE, NDIST3), refs


@pytest.mark.parametrize("k", [10, 100])  # R = 1 and 2: the slice's offset into the partial lists scales with k
@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_ivf_scan_kernel_second_slice(metric, nprobe, k, built, opt):
    """One query per block (ivf_t = 1) puts the queries on grid.z, 32768 a launch: 32768 + 37 queries are one sub-batch
    (< 2^21 pairs) and two launches."""
    ix, dq, pick, refs = built(slices_case, metric)
    assert NQ3 > SLICE and NQ3 * nprobe <= MAX_PAIRS and NQ3 <= max(256, MAX_PAIRS // nprobe)
    ref = refs[nprobe][0][:, :k], refs[nprobe][1][:, :k]
    answers_differ(ref)
    q = np.ascontiguousarray(dq[pick])
    opt("ivf_pass", "0")
    opt("lat_path", "0")
    opt("ivf_t", "1")
    with profile() as run:
        for entry, fn in (("host", lambda: ix.search(q, k, "nprobe=%d" % nprobe)), ("device", lambda: device_search(ix, q, k, nprobe))):
            got, count = run(fn)
            check(got, ref, pick, SLICE, "%s nprobe %d k %d %s entry" % (NAME[metric], nprobe, k, entry))
            assert count("ivf_scan") == 2, "%d launches of ivf_scan_kernel" % count("ivf_scan")
            assert planned_tiles()[1] == 1
    capi.release_scratch()


# ---------------------------------------------------------------------------------------- 4. query tiles beyond 65535 on grid.y

GRID_Y = 65535
T_FLAT = 8                      # plan_flat: tiles of 8 queries from 5 queries on (d = 4, k <= 3: far below the LDS budget)
NQ4 = T_FLAT * (GRID_Y + 1) + 5  # 65537 tiles
CUT4 = T_FLAT * GRID_Y           # the first query of tile 65535
N4, D4, NLIST4 = 48, 4, 8


@pytest.fixture(scope="module")
def tiles_data():
    rng = np.random.default_rng(400)
    centres, x, dq = int_blobs(rng, NLIST4, N4, N4, D4, spread=40, noise=4)
    return centres, x, dq, straddle(rng, NQ4, CUT4, N4)


@pytest.mark.parametrize("route", ["flat", "knn", "ivfflat", "ivfsq"])
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_more_query_tiles_than_65535(route, metric, tiles_data, opt):
    """flat_search_device puts ceil(nq / T) query tiles on grid.y: 8 * 65536 + 5 queries are 65537 tiles of 8.  A FLAT index and the
    brute-force knn scan their rows there; IVFFLAT (8 lists: no candidate pass for the coarse quantiser) and IVFSQ find their probes
    there -- plan_segments leaves an IVFSQ search of this size in one chunk (256 MiB / per_q of 160 bytes: 1.6 M queries), so its
    coarse step sees all 65537 tiles.  The profile counts one launch of flat_scan_kernel a search: nothing upstream cut the batch."""
    centres, x, dq, pick = tiles_data
    assert ceil_div(NQ4, T_FLAT) == GRID_Y + 2 and NQ4 <= MAX_PAIRS
    q = np.ascontiguousarray(dq[pick])
    om = sv.OM[metric]
    if route == "flat":
        ix = capi.Index(capi.INDEX_FLAT, metric, D4)
        ix.add(x)
        ix.build()
        search, ref3 = (lambda k: ix.search(q, k)), o.knn(dq, x, 3, om)
    elif route == "knn":
        ix = None
        search, ref3 = (lambda k: capi.knn(q, x, k, metric)), o.knn(dq, x, 3, om)
    elif route == "ivfflat":
        opt("coarse_mfma", "0")
        ix = sv.build_ivf(x, metric, NLIST4, centroids=centres)
        search, ref3 = (lambda k: ix.search(q, k, "nprobe=1")), sv.oracle_on_exported(ix, dq, 1, 3, metric)[:2]
    else:
        ix = capi.SqIndex(metric, D4)
        ix.set_codebook(centres, np.full(D4, -4, F), np.full(D4, 4, F))
        ix.add(x)
        ix.build()
        exp = ix.export()
        per_q = 1 * 1 * 3 * 8 + 16 * 4 + 1 * 8 + 64  # plan_segments: one probe, one segment, k keys; the padded row, the probe and pair, 64
        assert NQ4 <= (256 << 20) // per_q
        search, ref3 = (lambda k: ix.search(q, k, "nprobe=1")), sq.ref_search(exp, sq.decoded(exp), dq, 1, 3, metric)
    try:
        with profile() as run:
            for k in (1, 3):
                ref = ref3[0][:, :k], ref3[1][:, :k]
                answers_differ(ref)
                planned_tiles()
                got, count = run(lambda: search(k))
                check(got, ref, pick, CUT4, "%s %s k %d" % (route, NAME[metric], k))
                assert planned_tiles()[0] == T_FLAT
                assert count("flat_scan") == 1, "%s %s k %d: %d launches of flat_scan_kernel" % (route, NAME[metric], k, count("flat_scan"))
    finally:
        if ix is not None:
            ix.close()
        capi.release_scratch()


# ---------------------------------------------------------------------------------------- 5. BM25: the batch beyond one chunk

N_DOCS, VOCAB, NDIST5 = 20000, 300, 200
BM25_CAND_CAP, BW_DOCS, MAX_K = 2048, 2048, 256
BP_CAP, BP_MIN_DOCS, BP_MAX_DOCS, BM25_SKIP_DOCS = 64 * 8, 512, 8192, 2048


def bm25_chunk(c, queries, k, posting):
    """bm25_batch_device: the queries of one chunk, from the densest query of the batch"""
    rho = max(sum(int(c.df[t]) for t in qt) for qt in queries) / N_DOCS
    s = int(min(BP_MAX_DOCS, max(BP_MIN_DOCS, np.floor(0.75 * BP_CAP / max(rho, 1e-9)))))  # bm25_sub_docs_for
    if s >= BM25_SKIP_DOCS:
        s = s // BM25_SKIP_DOCS * BM25_SKIP_DOCS
    rounds = k > MAX_K
    sub_ub = BW_DOCS if posting == 0 else s if (rho <= 0.125 or posting == 2 or rounds) else min(BW_DOCS, s)
    n_blocks = max(1, ceil_div(N_DOCS, sub_ub))
    kl = min(k, MAX_K)
    per_q = BM25_CAND_CAP * 8 + 4 * 16 * (n_blocks + 1) + 64 * kl * 8 + ((kl + 1) * 8 if rounds else 0) + 64
    return max(1, (1024 << 20) // per_q)


class Corpus:
    """20000 documents of about 12 tokens over a vocabulary of 300 with 1 / (rank + 3) frequencies: the commonest term is in over half
    of the documents, so that an AND query of six of the twelve commonest terms still has hits."""

    def __init__(self):
        rng = np.random.default_rng(500)
        lens = np.maximum(1, rng.poisson(12, N_DOCS))
        p = 1.0 / (np.arange(VOCAB) + 3)
        toks = rng.choice(VOCAB, int(lens.sum()), p=p / p.sum())
        doc_of = np.repeat(np.arange(N_DOCS, dtype=np.int64), lens)
        uk, tf = np.unique(toks.astype(np.int64) * N_DOCS + doc_of, return_counts=True)
        term, self.doc, self.tf = uk // N_DOCS, (uk % N_DOCS).astype(np.uint32), tf.astype(np.uint32)
        self.post_off = np.zeros(VOCAB + 1, np.int64)
        np.cumsum(np.bincount(term, minlength=VOCAB), out=self.post_off[1:])
        self.fn = np.array([o.fieldnorm_id(int(v)) for v in range(int(lens.max()) + 1)], np.uint8)[lens]
        self.total = int(lens.sum())
        self.df = np.diff(self.post_off)
        # distinct queries: 0 is empty, 1 .. 6 have 1 .. 6 of the twelve commonest terms, the others 1 .. 6 terms of the whole
        # vocabulary; no term twice in a query
        nterms = [0, 1, 2, 3, 4, 5, 6] + rng.integers(1, 7, NDIST5 - 7).tolist()
        self.distinct = [rng.choice(12 if j < 7 else VOCAB, m, replace=False).tolist() for j, m in enumerate(nterms)]
        self.short = np.flatnonzero(np.asarray(nterms) <= 4)  # (the lean record scorer takes a chunk of such queries)
        self._ref = {}

    @functools.cached_property
    def ps(self):
        return capi.Postings(self.post_off, self.doc, self.tf, self.fn)

    def dfs(self, queries):
        return [[int(self.df[t]) for t in qt] for qt in queries]

    def oracle(self, j, k, operator_or):
        if (j, k, operator_or) not in self._ref:
            qt = self.distinct[j]
            self._ref[j, k, operator_or] = o.bm25_search_ex(self.post_off, self.doc, self.tf, self.fn, qt, self.dfs([qt])[0], N_DOCS, self.total, k,
                                                            operator_or=operator_or)
        return self._ref[j, k, operator_or]


@pytest.fixture(scope="module")
def corpus():
    c = Corpus()
    yield c
    if "ps" in c.__dict__:
        c.ps.close()
    capi.release_scratch()


def bm25_pick(c, nq, cut):
    """Queries of 5 and 6 terms and the empty one end the first chunk, queries of 1 to 4 terms begin the second, whose queries all
    have at most 4 terms: where the record scorers run, the tail chunk takes the lean one."""
    rng = np.random.default_rng(nq)
    pick = rng.integers(0, NDIST5, nq)
    pick[cut:] = c.short[rng.integers(0, len(c.short), nq - cut)]
    pick[cut - 3:cut + 4] = (5, 6, 0, 1, 2, 3, 4)
    pick[nq - 2:] = (1, 2)
    assert max(len(c.distinct[j]) for j in pick[cut:]) <= 4 < max(len(c.distinct[j]) for j in pick[:cut])
    return pick


@pytest.mark.parametrize("posting", [2, 0])
@pytest.mark.parametrize("k", [256, 300])
def test_bm25_batch_beyond_one_chunk(k, posting, corpus, opt):
    """The batch entry cuts the queries so that per_q * chunk <= 1 GiB and hands every chunk qoff + q0 with absolute term offsets;
    bm25_chunk_device opens the profile scope bm25_score once a chunk (rank rounds included), which must count two for every call.
    Both entries, a batch of OR queries and one of AND queries, under both scorer routings (bm25_chunk_device chooses per chunk).
    k = 300 are rank rounds, which only the record scorers serve: bm25_posting = 0 refuses them by design, so that pair is the error."""
    import torch
    c = corpus
    opt("bm25_posting", str(posting))
    if k > MAX_K and posting == 0:
        with pytest.raises(capi.MsvsError) as e:
            c.ps.bm25_search_batch([[1]], c.dfs([[1]]), N_DOCS, c.total, k)
        assert e.value.code == capi.ERR_UNSUPPORTED_K
        return
    chunk = bm25_chunk(c, c.distinct, k, posting)
    nq = chunk + TAIL
    pick = bm25_pick(c, nq, chunk)
    queries = [c.distinct[j] for j in pick]
    assert 7000 < chunk < 7400 and nq > bm25_chunk(c, queries, k, posting) == chunk
    dfs = c.dfs(queries)
    for operator_or in (True, False):
        refs = [c.oracle(j, k, operator_or) for j in range(NDIST5)]
        assert len({refs[j][0].tobytes() for j in range(1, 7)}) == 6 and len(refs[0][0]) == 0
        what = "k %d bm25_posting %d %s" % (k, posting, "or" if operator_or else "and")
        di = torch.full((nq, k), -7, device="cuda", dtype=torch.int64)
        dd = torch.full((nq, k), float("nan"), device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        with profile() as run:
            got, count = run(lambda: c.ps.bm25_search_batch(queries, dfs, N_DOCS, c.total, k, operator_or=operator_or))
            assert count("bm25_score") == 2, "%s, host entry: %d chunks" % (what, count("bm25_score"))
            _, count = run(lambda: c.ps.bm25_search_batch_device(queries, dfs, N_DOCS, c.total, k, di.data_ptr(), dd.data_ptr(),
                                                                 torch.cuda.current_stream().cuda_stream, operator_or=operator_or))
            assert count("bm25_score") == 2, "%s, device entry: %d chunks" % (what, count("bm25_score"))
        torch.cuda.synchronize()
        di, dd = di.cpu().numpy(), dd.cpu().numpy().view(np.uint32)
        bad = []
        for r, j in enumerate(pick):
            er, es = refs[j]
            n = len(er)
            gr, gs = got[r]
            if not (gr.tolist() == er.tolist() and (gs.view(np.uint32) == es.view(np.uint32)).all() and (di[r, :n] == er.astype(np.int64)).all()
                    and (di[r, n:] == -1).all() and (dd[r, :n] == es.view(np.uint32)).all()):
                bad.append(r)
        assert not bad, "%s: %d of %d queries differ from the oracle, %d of them before the cut at %d; first %d, last %d" % (
            what, len(bad), nq, sum(r < chunk for r in bad), chunk, bad[0], bad[-1])
    capi.release_scratch()
