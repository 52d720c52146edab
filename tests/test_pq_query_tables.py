"""The query-table form of the IVFPQ index (query_tables=1): look-up tables that depend on the query alone, one f32 row term per
stored row of an L2 index, the pair's coarse distance added in the scan.

The reference is a numpy restatement of the definition in include/msvs.h: P[s][j], w, b and the row score, every operation a
separately rounded f32 one.  Probes and b come from oracle.knn over the exported centroids; top-k is taken as
test_pq_ivf.ref_search takes it.  Ids are compared with == and distances by their bits.  Tests that need a GPU are marked one by
one: the table test and the test of the definition itself run anywhere."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_coded_index_files as cf
import test_pq4_ivf as pq4
import test_pq_ivf as pq
import test_special_values as sv
from oracle import oracle as o
from test_pq_ivf import blobs, by_hand, device_search, lists_of, ordered, same, seqsum

gpu = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
FLT_MAX = np.finfo(np.float32).max
NLIST = pq.NLIST
SHAPES = [(5, 5), (5, 1), (64, 16), (100, 25), (768, 96)]


# ---------------------------------------------------------------------------------------- the reference

def row_terms(exp):
    """w[row]: +0, then + g(s) for every sub-space in turn; g(s) the sequential sum of fl(cb_t * fl(fl(c_t + c_t) + cb_t))"""
    cent, cb, off, codes, _ = exp
    m, _, dsub = cb.shape
    c = cent[lists_of(off)]
    w = np.zeros(len(codes), F)
    for s in range(m):
        cs, e = c[:, s * dsub:(s + 1) * dsub], cb[s][codes[:, s]]
        with np.errstate(invalid="ignore", over="ignore"):
            g = seqsum((e * ((cs + cs).astype(F) + e).astype(F)).astype(F))
            w = (w + g).astype(F)
    return w


def code_sums(cb, codes, q):
    """acc[q, row]: +0, then + P[s][code[s]] for every sub-space in turn; P[s][j] the sequential sum of fl(q_t * cb[s][j][t])"""
    m, _, dsub = cb.shape
    acc = np.zeros((len(q), len(codes)), F)
    for s in range(m):
        with np.errstate(invalid="ignore", over="ignore"):
            tab = seqsum((q[:, None, s * dsub:(s + 1) * dsub] * cb[s][None]).astype(F))  # [q, ksub]
            acc = (acc + tab[:, codes[:, s]]).astype(F)
    return acc


def scores(exp, q, nprobe, ip):
    """-> (dis[q, row], probed[q, row]) for prepared (normalised) queries: b from oracle.knn over the centroids, NaN and unprobed
    where the list is not among the query's admitted probes"""
    cent, cb, off, codes, _ = exp
    nlist = len(cent)
    pid, pdis = o.knn(q, cent, min(nprobe, nlist), o.METRIC_IP if ip else o.METRIC_L2)
    b = np.full((len(q), nlist), np.nan, F)
    hit = np.zeros((len(q), nlist), bool)
    for i in range(len(q)):
        ok = pid[i] >= 0
        b[i, pid[i][ok]] = pdis[i][ok]
        hit[i, pid[i][ok]] = True
    lists = lists_of(off)
    acc = code_sums(cb, codes, q)
    with np.errstate(invalid="ignore", over="ignore"):
        if ip:
            dis = (b[:, lists] + acc).astype(F)
        else:
            dis = ((b[:, lists] + row_terms(exp)[None]).astype(F) - (F(2) * acc).astype(F)).astype(F)
    return dis, hit[:, lists]


def ref_search(exp, q, nprobe, k, metric, alive=None):
    labels = exp[4]
    ip = metric != L2
    if metric == COS:
        q = o.normalize_rows(q)
    q = np.ascontiguousarray(q, F)
    dis, probed = scores(exp, q, nprobe, ip)
    ids = np.full((len(q), k), -1, np.int64)
    out = np.full((len(q), k), -FLT_MAX if ip else FLT_MAX, F)
    ok_row = np.ones(len(labels), bool) if alive is None else np.array([l < len(alive) and alive[l] for l in labels], bool)
    for i in range(len(q)):
        d = dis[i]
        with np.errstate(invalid="ignore"):
            better = (d > -FLT_MAX) if ip else (d < FLT_MAX)  # strictly better than the neutral value; NaN never
        cand = np.flatnonzero(probed[i] & ok_row & better)
        key = ordered(d[cand])
        if ip:
            key = ~key
        order = cand[np.lexsort((labels[cand], key))][:k]
        ids[i, :len(order)] = labels[order]
        out[i, :len(order)] = d[order]
    if metric == COS:
        out = (F(1) - out).astype(F)
    return ids, out


def params(m, bits, extra=""):
    return "m=%d,bit_size=%d,query_tables=1%s" % (m, bits, extra)


@functools.lru_cache(maxsize=None)
def case(metric, bits, dim, m, data):
    """test_pq_ivf.case with query_tables=1: a trained and built index of 3000 rows in three chunks, its export and 300 queries"""
    rng = np.random.default_rng(dim * 13 + m * 101 + metric * 5 + len(data) + bits)
    n = 3000
    centres, x = blobs(rng, n, dim, NLIST)
    if data == "ties":  # 40 distinct vectors: equal distances everywhere, ordered by label
        x = np.ascontiguousarray(x[:40][rng.integers(0, 40, n)])
    labels = rng.permutation(3 * n)[:n].astype(np.int64)
    q = (centres[rng.integers(0, NLIST, 300)] + F(0.3) * rng.standard_normal((300, dim), dtype=F)).astype(F)
    ix = capi.PqIndex(metric, dim, params(m, bits, ",ncentroids=%d,kmeans_iters=4" % NLIST))
    assert ix.query_tables == 1 and ix.bits == bits
    ix.train(x)
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        ix.add(x[a:b], labels[a:b])
    ix.build()
    return ix, ix.export(), q


def twin(exp, x, labels, metric, bits):
    """the query-table index over the codebook of `exp` and the rows (x, labels): the same rows and codebook in the other form"""
    cent, cb = exp[0], exp[1]
    ix = capi.PqIndex(metric, cent.shape[1], params(cb.shape[0], bits))
    ix.set_codebook(cent, cb)
    ix.add(x, labels)
    ix.build()
    return ix


def hand_pair(rng, metric, dim, m, nlist, n, bits, scale=0.5):
    """by_hand of the width's test file (the default form) and its twin in the query-table form"""
    ix0, exp0, _, x = (by_hand if bits == 8 else pq4.by_hand)(rng, metric, dim, m, nlist, n, scale)
    ix1 = twin(exp0, x, np.arange(n, dtype=np.int64) * 3, metric, bits)
    exp1 = ix1.export()
    for a, b in zip(exp0, exp1):  # codes are the same bytes in both forms
        assert a.tobytes() == b.tobytes()
    return ix0, ix1, exp1, x


# ---------------------------------------------------------------------------------------- 1. row terms

@gpu
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("dim,m", [(5, 5), (5, 1), (100, 25), (768, 96)])
def test_row_terms(dim, m, bits):
    ix, exp, _ = case(L2, bits, dim, m, "clustered")
    w = ix.export_row_terms()
    assert w.shape == (3000,) and w.dtype == F
    assert (w.view(np.uint32) == row_terms(exp).view(np.uint32)).all()
    store = {}
    ix.serialize_io(store)
    ld = capi.PqIndex.load_io(store)
    assert (ld.export_row_terms().view(np.uint32) == w.view(np.uint32)).all()
    ld.close()


@gpu
@pytest.mark.parametrize("metric", [IP, COS])
def test_no_row_terms_for_inner_product(metric):
    ix, _, _ = case(metric, 8, 5, 5, "clustered" if metric == COS else "ties")
    assert pq.code_of(ix.export_row_terms) == capi.ERR_INVALID_ARGUMENT
    plain = capi.PqIndex(L2, 8, "m=2")
    assert pq.code_of(plain.export_row_terms) == capi.ERR_INVALID_ARGUMENT  # the default form keeps none
    fresh = capi.PqIndex(L2, 8, params(2, 8))
    assert pq.code_of(fresh.export_row_terms) == capi.ERR_NOT_READY


# ---------------------------------------------------------------------------------------- 2. search parity

# The tile T: 8 from 16 pairs per list on, 4 from 2, 2 from 1, else 1 (pairs = nq * min(nprobe, nlist), nlist = 8), halved until
# T * m * (4 << bits) bytes of tables + T * 40 * k of merge lists + 4 * T of pair terms fit 160 KiB; R: 1 / 2 / 4 for k <= 64 /
# <= 128 / <= 256.  The last column names the (T, R) a row reaches; the rows of each width reach all twelve.
PARITY = [
    (L2, 8, 5, 5, "clustered", 1, 1, 1, "host", (1, 1)),
    (L2, 8, 5, 1, "ties", 300, 256, 8, "device", (8, 4)),
    (IP, 8, 5, 5, "ties", 40, 100, 3, "host", (4, 2)),
    (COS, 8, 5, 1, "clustered", 9, 10, 3, "device", (4, 1)),
    (L2, 8, 64, 16, "clustered", 300, 10, 3, "host", (8, 1)),
    (L2, 8, 64, 16, "ties", 300, 100, 8, "host", (8, 2)),  # 131072 + 32000 + 32 = 163104 of 163840 bytes
    (L2, 8, 64, 16, "ties", 300, 256, 8, "device", (4, 4)),
    (IP, 8, 64, 16, "clustered", 3, 256, 3, "host", (2, 4)),
    (COS, 8, 64, 16, "ties", 300, 1, 80, "host", (8, 1)),
    (L2, 8, 64, 16, "clustered", 1, 100, 3, "device", (1, 2)),
    (COS, 8, 100, 25, "clustered", 1, 256, 80, "device", (2, 4)),
    (L2, 8, 100, 25, "clustered", 40, 10, 8, "device", (4, 1)),
    (IP, 8, 100, 25, "ties", 9, 1, 1, "host", (2, 1)),
    (IP, 8, 100, 25, "clustered", 300, 256, 8, "host", (4, 4)),
    (L2, 8, 768, 96, "clustered", 40, 10, 3, "host", (1, 1)),
    (L2, 8, 768, 96, "clustered", 9, 256, 80, "device", (1, 4)),
    (IP, 8, 768, 96, "ties", 1, 10, 80, "device", (1, 1)),
    (COS, 8, 768, 96, "clustered", 3, 100, 1, "host", (1, 2)),
    (L2, 8, 5, 5, "clustered", 1, 100, 8, "host", (2, 2)),
    (IP, 8, 5, 5, "ties", 16, 100, 8, "device", (8, 2)),
    (L2, 8, 5, 1, "clustered", 1, 256, 3, "host", (1, 4)),
    (COS, 8, 5, 5, "clustered", 300, 256, 8, "host", (8, 4)),
    (L2, 4, 5, 5, "clustered", 1, 1, 1, "host", (1, 1)),
    (L2, 4, 5, 1, "ties", 300, 256, 8, "device", (8, 4)),
    (IP, 4, 5, 5, "ties", 40, 100, 3, "host", (4, 2)),
    (COS, 4, 5, 1, "clustered", 9, 10, 3, "device", (4, 1)),
    (L2, 4, 64, 16, "clustered", 300, 10, 3, "host", (8, 1)),
    (IP, 4, 64, 16, "clustered", 3, 256, 3, "host", (2, 4)),
    (L2, 4, 64, 16, "clustered", 1, 100, 3, "device", (1, 2)),
    (COS, 4, 100, 25, "clustered", 1, 256, 80, "device", (2, 4)),
    (L2, 4, 100, 25, "clustered", 40, 10, 8, "device", (8, 1)),
    (IP, 4, 100, 25, "ties", 9, 1, 1, "host", (2, 1)),
    (L2, 4, 768, 96, "clustered", 300, 256, 8, "host", (8, 4)),
    (L2, 4, 768, 96, "clustered", 9, 256, 80, "device", (4, 4)),
    (IP, 4, 768, 96, "ties", 1, 10, 80, "device", (2, 1)),
    (COS, 4, 768, 96, "clustered", 3, 100, 1, "host", (1, 2)),
    (L2, 4, 5, 5, "clustered", 1, 100, 8, "host", (2, 2)),
    (IP, 4, 64, 16, "ties", 16, 100, 8, "device", (8, 2)),
    (L2, 4, 5, 1, "clustered", 1, 256, 3, "host", (1, 4)),
    (COS, 4, 64, 16, "ties", 300, 1, 80, "host", (8, 1)),
]


def lds_bytes(bits, t, m, k):
    return t * m * (4 << bits) + 40 * t * k + 4 * t


def tile_class(bits, m, nq, k, nprobe):
    pairs = nq * min(nprobe, NLIST)
    t = 8 if pairs >= 16 * NLIST else 4 if pairs >= 2 * NLIST else 2 if pairs >= NLIST else 1
    while t > 1 and lds_bytes(bits, t, m, k) > 160 * 1024:
        t //= 2
    return t, 1 if k <= 64 else 2 if k <= 128 else 4


def test_parity_table_reaches_every_tile_and_k_class():
    reached = {8: set(), 4: set()}
    for metric, bits, dim, m, data, nq, k, nprobe, entry, cls in PARITY:
        assert (dim, m) in SHAPES and k in (1, 10, 100, 256) and nprobe in (1, 3, 8, 80) and 1 <= nq <= 300
        assert tile_class(bits, m, nq, k, nprobe) == cls
        reached[bits].add(cls)
    for bits in (8, 4):
        assert reached[bits] == {(t, r) for t in (1, 2, 4, 8) for r in (1, 2, 4)}
    assert {(r[0], r[1]) for r in PARITY} == {(mt, b) for mt in (L2, IP, COS) for b in (8, 4)}
    assert {r[4] for r in PARITY} == {"clustered", "ties"} and {r[8] for r in PARITY} == {"host", "device"}
    assert lds_bytes(8, 8, 16, 100) == 163104 and lds_bytes(8, 2, 96, 1) > 160 * 1024
    for bits, m in ((8, 128), (4, 256)):  # the T = 1 image is smaller than the default form's: every index that exists fits
        assert lds_bytes(bits, 1, m, 256) <= 160 * 1024


@gpu
@pytest.mark.parametrize("metric,bits,dim,m,data,nq,k,nprobe,entry,cls", PARITY)
def test_search_parity(metric, bits, dim, m, data, nq, k, nprobe, entry, cls):
    ix, exp, q = case(metric, bits, dim, m, data)
    q = q[:nq]
    got = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else device_search(ix, q, k, nprobe)
    same(got, ref_search(exp, q, nprobe, k, metric))


# ---------------------------------------------------------------------------------------- 3. segments and odd lists

def listed(rng, sizes, bits, dim=20, m=5):
    nlist = len(sizes)
    cent = np.zeros((nlist, dim), F)
    cent[:, 0] = 10.0 * np.arange(nlist)
    home = np.repeat(np.arange(nlist), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    cb = (F(0.4) * rng.standard_normal((m, 1 << bits, dim // m), dtype=F)).astype(F)
    ix = capi.PqIndex(L2, dim, params(m, bits))
    ix.set_codebook(cent, cb)
    ix.add(x, rng.permutation(3 * len(home))[:len(home)].astype(np.int64))
    ix.build()
    exp = ix.export()
    assert np.diff(exp[2]).tolist() == list(sizes)
    return ix, exp, cent


@gpu
@pytest.mark.parametrize("bits", [8, 4])
def test_empty_short_and_segmented_lists(bits, opt):
    rng = np.random.default_rng(3 + bits)
    sizes = [1000, 3, 1, 0, 0, 50]  # four segments in the long list; the others start mid-block of the transposed layout
    ix, exp, cent = listed(rng, sizes, bits)
    assert exp[2][1] % 64 == 40 and exp[2][5] % 64 == 44
    opt("pq_ivf_rpb", "256")
    q = (cent[[0, 1, 2, 3, 5, 1]] + F(0.5) * rng.standard_normal((6, 20), dtype=F)).astype(F)
    for nprobe, k in ((6, 100), (2, 10), (1, 256), (3, 1)):
        same(ix.search(q, k, "nprobe=%d" % nprobe), ref_search(exp, q, nprobe, k, L2))
    ids, dis = ix.search(cent[3:4], 5, "nprobe=1")  # an empty list
    assert (ids == -1).all() and (dis == FLT_MAX).all()
    same(device_search(ix, q, 100, 6), ref_search(exp, q, 6, 100, L2))
    assert (ix.export_row_terms().view(np.uint32) == row_terms(exp).view(np.uint32)).all()
    ix.close()


@gpu
@pytest.mark.parametrize("bits", [8, 4])
def test_twelve_segments(bits, opt):
    rng = np.random.default_rng(31 + bits)
    ix, exp, cent = listed(rng, [3000, 70], bits)
    opt("pq_ivf_rpb", "256")  # eleven whole segments and one of 184 rows; the second list starts at row 3000 = 46 * 64 + 56
    q = (cent[[0, 1, 0, 0, 1]] + F(0.5) * rng.standard_normal((5, 20), dtype=F)).astype(F)
    for nprobe, k in ((2, 100), (1, 256), (2, 1)):
        same(ix.search(q, k, "nprobe=%d" % nprobe), ref_search(exp, q, nprobe, k, L2))
    same(device_search(ix, q, 256, 2), ref_search(exp, q, 2, 256, L2))
    ix.close()


@gpu
def test_a_search_in_three_rounds(opt):
    """255 queries, k = 256, 64 lists all probed, one list of 4000 rows in 256-row segments: 2 MiB of partial lists a query, so rounds
    of 127, 127 and 1 queries (the shape of test_coded_host_loops.py) -- the tables and pair terms of a round are indexed by the
    round's own queries."""
    rng = np.random.default_rng(77)
    ix, exp, cent = listed(rng, [4000] + [10] * 63, 8, dim=8, m=2)
    opt("pq_ivf_rpb", "256")
    q = (cent[rng.integers(0, 64, 255)] + F(0.5) * rng.standard_normal((255, 8), dtype=F)).astype(F)
    capi.profile_enable(True)
    try:
        capi.profile_reset()
        got = ix.search(q, 256, "nprobe=64")
        launches = capi.profile_get("pq_ivf_scan")[0], capi.profile_get("pq_query_tables")[0]
    finally:
        capi.profile_enable(False)
        capi.release_scratch()  # (a round's arena is about 256 MB)
    assert launches == (3, 3)
    same(got, ref_search(exp, q, 64, 256, L2))
    ix.close()


# ---------------------------------------------------------------------------------------- 4. filter by label

@gpu
@pytest.mark.parametrize("metric,bits", [(L2, 8), (COS, 4)])
def test_filter_by_label(metric, bits):
    ix, exp, q = case(metric, bits, 64, 16, "ties")
    labels = exp[4]
    q = q[:20]
    rng = np.random.default_rng(6)
    top = int(labels.max()) + 1
    half = rng.random(top) < 0.5
    one = np.zeros(top, bool)
    one[labels[17]] = True
    none = np.zeros(top, bool)
    for alive in (half, one, none):
        same(ix.search(q, 10, "nprobe=3", alive=alive), ref_search(exp, q, 3, 10, metric, alive=alive))
    same(device_search(ix, q, 10, NLIST, alive=half), ref_search(exp, q, NLIST, 10, metric, alive=half))
    # a bitmap shorter than the label space: labels at or beyond nbits are dead
    nbits = top // 2
    cut = np.ones(top, bool)
    cut[nbits:] = False
    ref = ref_search(exp, q, NLIST, 10, metric, alive=cut)
    got = ix.search(q, 10, "nprobe=%d" % NLIST, alive=np.ones(nbits, bool), nbits=nbits)
    same(got, ref)
    assert (got[0] < nbits).all()
    same(device_search(ix, q, 10, NLIST, alive=np.ones(nbits, bool)), ref)


# ---------------------------------------------------------------------------------------- 5. special queries

@gpu
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_special_queries(metric, bits):
    """NaN, +-inf, overflowing (3e38), zero and subnormal queries (test_special_values.special_queries).  A list whose b is not
    admitted is no probe of the reference (oracle.knn gives -1) and contributes nothing."""
    _, ix, exp, x = hand_pair(np.random.default_rng(50 + metric + bits), metric, 100, 20, 8, 3000, bits)
    q, where = sv.special_queries(x[:64] + F(0.1))
    q[20, 5], q[21, 70], q[22, :50] = F(3e38), F(-3e38), F(3e38)  # products that overflow where their sum would not
    ref = ref_search(exp, q, sv.NPROBE, sv.K, metric)
    assert (ref[0][where["nan_one"]] == -1).all()  # no list is admitted
    assert (ref[0][0] >= 0).all()
    same(ix.search(q, sv.K, "nprobe=%d" % sv.NPROBE), ref)
    same(device_search(ix, q, sv.K, sv.NPROBE), ref)
    ix.close()


# ---------------------------------------------------------------------------------------- 6. files

@gpu
@pytest.mark.parametrize("metric,bits", [(L2, 8), (L2, 4), (IP, 8)])
def test_files(metric, bits):
    ix0, ix1, exp, x = hand_pair(np.random.default_rng(60 + bits), metric, 20, 5, 4, 700, bits)
    s0, s1 = {}, {}
    ix0.serialize_io(s0)
    ix1.serialize_io(s1)
    d0, d1 = bytes(s0["pq_data"]), bytes(s1["pq_data"])
    word = (4 if bits == 4 else 0)
    assert bytes(s0["pq_ids"]) == bytes(s1["pq_ids"])
    assert struct.unpack_from("<Q", d0, 48)[0] == word and struct.unpack_from("<Q", d1, 48)[0] == word | 0x100
    assert d1 == cf.with_check(d0[:48] + struct.pack("<Q", word | 0x100)) + d0[64:]  # the reserved word and the check word only
    q = x[:25] + F(0.05)
    ld = capi.PqIndex.load_io(s1)
    assert ld.query_tables == 1 and ld.bits == bits and ld.ready
    for a, b in zip(exp, ld.export()):
        assert a.tobytes() == b.tobytes()
    same(ld.search(q, 10, "nprobe=3"), ix1.search(q, 10, "nprobe=3"))
    same(ld.search(q, 10, "nprobe=3"), ref_search(exp, q, 3, 10, metric))
    again = {}
    ld.serialize_io(again)
    assert bytes(again["pq_data"]) == d1 and bytes(again["pq_ids"]) == bytes(s1["pq_ids"])
    ld.close()
    with pytest.raises(ValueError):
        capi.PqIndex.load_io(s1, query_tables=0)
    capi.PqIndex.load_io(s1, query_tables=1).close()
    for reserved in (0x101, 0x200, 0x108):  # no form; check words recomputed
        bad = dict(s1)
        bad["pq_data"] = bytearray(cf.with_check(d1[:48] + struct.pack("<Q", reserved)) + d1[64:])
        assert pq.code_of(lambda: capi.PqIndex.load_io(bad)) == capi.ERR_IO, reserved
    ld0 = capi.PqIndex.load_io(s0)  # a form-0 file loads as form 0
    assert ld0.query_tables == 0
    same(ld0.search(q, 10, "nprobe=3"), ix0.search(q, 10, "nprobe=3"))
    assert pq.code_of(ld0.export_row_terms) == capi.ERR_INVALID_ARGUMENT
    ld0.close()
    ix0.close()
    ix1.close()


# ---------------------------------------------------------------------------------------- 7. lifecycle

def query_tables_of(handle):
    fn = capi.lib().msvs_pq_index_query_tables
    fn.restype = capi.C.c_int
    fn.argtypes = [capi.C.c_void_p]
    return fn(handle)


@gpu
def test_lifecycle():
    for bad in (2, -1, 256):
        assert pq.code_of(lambda: capi.PqIndex(L2, 16, "m=4,query_tables=%d" % bad)) == capi.ERR_INVALID_ARGUMENT
    assert query_tables_of(None) == 0
    assert capi.PqIndex(L2, 16, "m=4").query_tables == 0 and capi.PqIndex(L2, 16, "m=4,query_tables=0").query_tables == 0
    ix = capi.PqIndex(L2, 16, "m=4,query_tables=1,bit_size=4")
    assert ix.query_tables == 1 and query_tables_of(ix._h) == 1
    assert pq.code_of(ix.export_row_terms) == capi.ERR_NOT_READY
    assert pq.code_of(lambda: ix.search(np.zeros((1, 16), F), 1)) == capi.ERR_NOT_READY
    ix.close()
    built, _, _ = case(L2, 8, 5, 5, "clustered")
    assert pq.code_of(lambda: built.search(np.zeros((1, 5), F), 257)) == capi.ERR_UNSUPPORTED_K
    assert pq.code_of(lambda: built.search(np.zeros((1, 5), F), 1, "nprobe=0")) == capi.ERR_INVALID_ARGUMENT
    ids, dis = built.search(np.zeros((3, 5), F), 0)
    assert ids.shape == (3, 0) and dis.shape == (3, 0)


@gpu
@pytest.mark.parametrize("metric,bits", [(L2, 8), (L2, 4), (IP, 8)])
def test_memory_usage_within_the_documented_bound(metric, bits):
    rng = np.random.default_rng(10)
    n, dim, m, nlist = 20000, 64, 16, 16
    cent, x = blobs(rng, n, dim, nlist)
    ix = capi.PqIndex(metric, dim, params(m, bits))
    ix.set_codebook(cent, (F(0.3) * rng.standard_normal((m, 1 << bits, dim // m), dtype=F)).astype(F))
    ix.add(x[:12000])
    ix.add(x[12000:])
    ix.build()
    tables = nlist * dim * 4 + (1 << bits) * dim * 4 + (nlist + 1) * 8
    row = m * bits // 8
    terms = 4 * n if metric == L2 else 0  # one f32 per row for an L2 index of this form only
    assert n * row + terms <= ix.memory_usage <= n * ((row + 15) // 16 * 16 + 8) + tables + 4096 + terms
    ix.close()


@gpu
@pytest.mark.parametrize("bits", [8, 4])
def test_training_ignores_the_key(bits):
    rng = np.random.default_rng(9)
    _, x = blobs(rng, 2000, 32, NLIST)
    out = []
    for extra in ("", ",query_tables=0", ",query_tables=1"):
        ix = capi.PqIndex(L2, 32, "ncentroids=%d,m=8,bit_size=%d,kmeans_iters=5%s" % (NLIST, bits, extra))
        ix.train(x)
        ix.add(x)
        ix.build()
        out.append(ix.export())
        ix.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):  # centroids, codebooks, offsets, codes and labels: the same bits
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------- 8. the definition is a distance

@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("dim,m", SHAPES)
def test_the_definition_is_a_distance(dim, m, bits):
    """The reference's value against the f64 |q - (c + cb)|^2 and q . (c + cb) on random rows, codes and queries.  The margin is
    (d + m + 8) * 2^-23 * A: the standard forward bound (n roundings: n * 2^-24 * A) for the d + m + 8 roundings at most that any
    product passes through, doubled; A is the f64 sum of the absolute values of every product entering the formula.  In numpy on
    these shapes the worst error is about 0.10 of the margin."""
    rng = np.random.default_rng(80 + dim + m + bits)
    n, nq, nlist, dsub = 200, 16, 4, dim // m
    cent = rng.standard_normal((nlist, dim), dtype=F)
    cb = (F(0.5) * rng.standard_normal((m, 1 << bits, dsub), dtype=F)).astype(F)
    home = np.sort(rng.integers(0, nlist, n))
    off = np.searchsorted(home, np.arange(nlist + 1)).astype(np.int64)
    codes = rng.integers(0, 1 << bits, (n, m)).astype(np.uint8)
    exp = (cent, cb, off, codes, np.arange(n, dtype=np.int64))
    q = (cent[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    c64 = cent[home].astype(np.float64)
    cb64 = np.concatenate([cb[s][codes[:, s]] for s in range(m)], axis=1).astype(np.float64)  # [n, d]
    q64 = q.astype(np.float64)[:, None, :]
    eps = (dim + m + 8) * 2.0 ** -23
    worst = 0.0
    for ip in (False, True):
        dis, probed = scores(exp, q, nlist, ip)
        assert probed.all()
        if ip:
            exact = (q64 * (c64 + cb64)[None]).sum(-1)
            A = (np.abs(q64) * (np.abs(c64) + np.abs(cb64))[None]).sum(-1)
        else:
            exact = ((q64 - (c64 + cb64)[None]) ** 2).sum(-1)
            A = ((q64 - c64[None]) ** 2).sum(-1) + (np.abs(cb64) * (np.abs(2 * c64) + np.abs(cb64))).sum(-1)[None] \
                + 2 * (np.abs(q64) * np.abs(cb64)[None]).sum(-1)
        err = np.abs(dis.astype(np.float64) - exact) / (eps * A)
        worst = max(worst, err.max())
        assert (err <= 1).all(), (ip, err.max())
    print("worst error / margin: %.3f" % worst)


# ---------------------------------------------------------------------------------------- 9. recall

@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_recall_against_the_original_rows(metric):
    """The set-up of test_pq_ivf.test_recall_against_the_original_rows (4000 x 64 rows in 8 blobs, 8 lists all probed, m = 16, 100
    queries): the share of the exact top-10 of the ORIGINAL rows inside the top-100 must be >= 0.95, first for the reference, then
    for the index, which must equal it bit for bit.  Top-10 in top-10 is printed, not asserted."""
    rng = np.random.default_rng(11)
    n, dim, m, nlist, nq = 4000, 64, 16, 8, 100
    centres, x = blobs(rng, n, dim, nlist)
    q = (centres[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    if metric == L2:
        exact = ((q[:, None, :].astype(np.float64) - x[None]) ** 2).sum(-1)
    else:
        exact = -(q.astype(np.float64) @ x.T.astype(np.float64))
    truth = np.argsort(exact, axis=1, kind="stable")[:, :10]
    ix = capi.PqIndex(metric, dim, params(m, 8, ",ncentroids=%d,kmeans_iters=5" % nlist))
    ix.train(x)
    ix.add(x)
    ix.build()
    exp = ix.export()

    def share(ids, width):
        return np.mean([len(set(t.tolist()) & set(g[:width].tolist())) / 10 for t, g in zip(truth, ids)])

    ref = ref_search(exp, q, nlist, 100, metric)
    print("reference: 10 in 100 %.3f, 10 in 10 %.3f" % (share(ref[0], 100), share(ref[0], 10)))
    assert share(ref[0], 100) >= 0.95
    got = ix.search(q, 100, "nprobe=%d" % nlist)
    print("index: 10 in 100 %.3f, 10 in 10 %.3f" % (share(got[0], 100), share(got[0], 10)))
    assert share(got[0], 100) >= 0.95
    same(got, ref)
    ix.close()
