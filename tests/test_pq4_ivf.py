"""The 4-bit form of the IVFPQ index (bit_size=4): 16 entries per sub-quantiser, two codes a stored byte, 16-entry tables in the scan.

The reference is the one of test_pq_ivf.py, whose numpy helpers (seqsum, encode, decoded, adc, ref_search, same, device_search) are
generic in the number of entries: the export gives one code a byte in both forms.  Every comparison is == on ids and on the uint32
view of the distances; codes and files byte for byte."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_coded_index_files as cf
import test_pq_ivf as pq
import test_special_values as sv

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
FLT_MAX = np.finfo(np.float32).max
NLIST = pq.NLIST
# dsub 1 + a partial table pass + an odd m (pad nibble); a single nibble; exactly one word; one word + one nibble; one exact table
# pass; mw = 5 (the second unit of four has one word); m = 25; the equal-bytes partner of 8-bit m = 96; the largest m (mw = 32)
SHAPES = [(5, 5), (5, 1), (16, 8), (72, 9), (64, 16), (80, 40), (100, 25), (768, 192), (768, 256)]


def codebooks16(rng, m, dsub, scale=0.5):
    return (F(scale) * rng.standard_normal((m, 16, dsub), dtype=F)).astype(F)


@functools.lru_cache(maxsize=None)
def case(metric, dim, m, data):
    """test_pq_ivf.case with bit_size=4: a trained and built index of 3000 rows in three chunks, its export, the decoded matrix and
    300 queries; computed once."""
    rng = np.random.default_rng(dim * 13 + m * 101 + metric * 5 + len(data))
    n = 3000
    centres, x = pq.blobs(rng, n, dim, NLIST)
    if data == "ties":  # 40 distinct vectors: equal distances everywhere, ordered by label
        x = np.ascontiguousarray(x[:40][rng.integers(0, 40, n)])
    labels = rng.permutation(3 * n)[:n].astype(np.int64)  # shuffled, not contiguous
    q = (centres[rng.integers(0, NLIST, 300)] + F(0.3) * rng.standard_normal((300, dim), dtype=F)).astype(F)
    ix = capi.PqIndex(metric, dim, "ncentroids=%d,m=%d,bit_size=4,kmeans_iters=4" % (NLIST, m))
    ix.train(x)
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        ix.add(x[a:b], labels[a:b])
    ix.build()
    exp = ix.export()
    return ix, exp, pq.decoded(exp), x, labels, q


def by_hand(rng, metric, dim, m, nlist, n, scale=0.5):
    centres, x = pq.blobs(rng, n, dim, nlist)
    ix = capi.PqIndex(metric, dim, "m=%d,bit_size=4" % m)
    ix.set_codebook(centres, codebooks16(rng, m, dim // m, scale))
    ix.add(x, np.arange(n, dtype=np.int64) * 3)
    ix.build()
    exp = ix.export()
    return ix, exp, pq.decoded(exp), x


# ---------------------------------------------------------------------------------------- 1. structure and codes

@pytest.mark.parametrize("dim,m", SHAPES)
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_structure_and_codes(metric, dim, m):
    ix, exp, _, x, labels, _ = case(metric, dim, m, "clustered")
    cent, cb, off, codes, elab = exp
    n = len(x)
    assert ix.bits == 4 and ix.ready and ix.num_data == n and ix.num_lists == NLIST
    assert cent.shape == (NLIST, dim) and cb.shape == (m, 16, dim // m) and codes.shape == (n, m)
    assert np.isfinite(cb).all() and (codes < 16).all()
    assert len(off) == NLIST + 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert sorted(elab.tolist()) == sorted(labels.tolist())
    for l in range(NLIST):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    where = {int(l): i for i, l in enumerate(labels)}
    xs = pq.stored(x, metric)[[where[int(l)] for l in elab]]  # the fed rows in export order
    assert (codes == pq.encode(xs, cent[pq.lists_of(off)], cb)).all()


def test_ties_go_to_the_lower_entry_and_an_all_equal_subspace_gives_zero():
    rng = np.random.default_rng(21)
    dim, m, nlist = 12, 3, 3
    dsub = dim // m
    cent = rng.standard_normal((nlist, dim), dtype=F)
    cb = codebooks16(rng, m, dsub)
    cb[0, 8:] = cb[0, :8]   # every entry of sub-space 0 twice: the lower one wins
    cb[1, :] = cb[1, 7]     # sub-space 1: all entries equal
    cb[2, 5] = cb[2, 12]    # one duplicated pair in an otherwise distinct codebook
    home = rng.integers(0, nlist, 1500)
    x = (cent[home] + F(0.5) * rng.standard_normal((1500, dim), dtype=F)).astype(F)
    x[:300, 2 * dsub:] = (cent[home[:300], 2 * dsub:] + cb[2, 12]).astype(F)  # rows at the duplicated entry
    ix = capi.PqIndex(L2, dim, "m=%d,bit_size=4" % m)
    ix.set_codebook(cent, cb)
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent2, cb2, off, codes, labels = exp
    assert cent2.tobytes() == cent.tobytes() and cb2.tobytes() == cb.tobytes()
    assert (codes[:, 0] < 8).all() and (codes[:, 1] == 0).all() and (codes[:, 2] != 12).all() and (codes[:, 2] == 5).any()
    assert (codes == pq.encode(x[labels], cent[pq.lists_of(off)], cb)).all()
    pq.same(ix.search(x[:7], 20, "nprobe=%d" % nlist), pq.ref_search(exp, pq.decoded(exp), x[:7], nlist, 20, L2))
    ix.close()


# ---------------------------------------------------------------------------------------- 2. search parity

# The list scan's query tile T: 8 from 16 pairs per list on, 4 from 2, 2 from 1, else 1 (pairs = nq * min(nprobe, nlist), nlist = 8),
# halved until 64 * T * m bytes of tables + (T + 1) * 4 * round_up(dim, 4) + T * 40 * k bytes fit 160 KiB; its top-k class R: 1 / 2 / 4
# for k <= 64 / <= 128 / <= 256.  The last column names the (T, R) a row reaches; together they reach all twelve.
PARITY = [
    (L2, 5, 5, "clustered", 1, 1, 1, "host", (1, 1)),
    (L2, 5, 1, "ties", 300, 256, NLIST, "device", (8, 4)),
    (IP, 5, 5, "ties", 40, 100, 4, "host", (8, 2)),
    (COS, 5, 1, "clustered", 9, 10, 4, "device", (4, 1)),
    (L2, 16, 8, "clustered", 300, 10, 4, "host", (8, 1)),
    (L2, 16, 8, "ties", 3, 256, NLIST, "host", (4, 4)),
    (IP, 72, 9, "clustered", 3, 256, 4, "host", (2, 4)),
    (COS, 72, 9, "ties", 300, 1, NLIST, "host", (8, 1)),
    (L2, 64, 16, "clustered", 1, 100, 4, "device", (1, 2)),
    (L2, 80, 40, "ties", 3, 100, NLIST, "host", (4, 2)),
    (IP, 80, 40, "clustered", 300, 100, 1, "host", (8, 2)),
    (COS, 100, 25, "clustered", 1, 256, 10 * NLIST, "device", (2, 4)),
    (L2, 100, 25, "clustered", 40, 10, NLIST, "device", (8, 1)),
    (IP, 100, 25, "ties", 9, 1, 1, "host", (2, 1)),
    (L2, 768, 256, "clustered", 16, 10, NLIST, "host", (8, 1)),  # the largest image: 131072 + 27648 + 3200 = 161920 of 163840 bytes
    (L2, 768, 256, "clustered", 16, 100, 10 * NLIST, "device", (4, 2)),  # (tile 8 would need 131072 + 27648 + 32000 bytes)
    (IP, 768, 192, "clustered", 16, 10, NLIST, "device", (8, 1)),
    (COS, 768, 192, "clustered", 16, 100, NLIST, "host", (8, 2)),
    (IP, 768, 192, "clustered", 1, 10, 10 * NLIST, "device", (2, 1)),
    (COS, 768, 256, "clustered", 3, 100, 1, "host", (1, 2)),
    (L2, 768, 192, "clustered", 9, 256, 10 * NLIST, "device", (4, 4)),
    (L2, 5, 1, "clustered", 1, 256, 4, "host", (1, 4)),
    (IP, 64, 16, "clustered", 3, 10, 4, "host", (2, 1)),
    (L2, 100, 25, "clustered", 1, 100, NLIST, "host", (2, 2)),
    (COS, 64, 16, "clustered", 40, 256, 1, "device", (4, 4)),
    (IP, 16, 8, "clustered", 2, 10, 2, "host", (1, 1)),
    (IP, 80, 40, "clustered", 5, 10, NLIST, "device", (4, 1)),
]


def lds_bytes4(t, dim, m, k):
    return 64 * t * m + 4 * (t + 1) * ((dim + 3) // 4 * 4) + 40 * t * k


def tile_class4(dim, m, nq, k, nprobe):
    pairs = nq * min(nprobe, NLIST)
    t = 8 if pairs >= 16 * NLIST else 4 if pairs >= 2 * NLIST else 2 if pairs >= NLIST else 1
    while t > 1 and lds_bytes4(t, dim, m, k) > 160 * 1024:
        t //= 2
    return t, 1 if k <= 64 else 2 if k <= 128 else 4


def test_parity_table_reaches_every_tile_and_k_class():
    reached = set()
    for metric, dim, m, data, nq, k, nprobe, entry, cls in PARITY:
        assert tile_class4(dim, m, nq, k, nprobe) == cls
        reached.add(cls)
    assert reached == {(t, r) for t in (1, 2, 4, 8) for r in (1, 2, 4)}
    assert lds_bytes4(8, 768, 256, 10) == 161920 and tile_class4(768, 256, 16, 10, NLIST) == (8, 1)
    assert tile_class4(768, 256, 16, 100, NLIST) == (4, 2) and tile_class4(768, 192, 16, 10, NLIST) == (8, 1)
    for dim, m in ((8192, 256), (8192, 1), (768, 256)):  # the T = 1 image fits at every shape the form admits
        assert lds_bytes4(1, dim, m, 256) <= 160 * 1024


@pytest.mark.parametrize("metric,dim,m,data,nq,k,nprobe,entry,cls", PARITY)
def test_search_parity(metric, dim, m, data, nq, k, nprobe, entry, cls):
    ix, exp, xh, _, _, q = case(metric, dim, m, data)
    q = q[:nq]
    got = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else pq.device_search(ix, q, k, nprobe)
    pq.same(got, pq.ref_search(exp, xh, q, nprobe, k, metric))


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
    ix = capi.PqIndex(L2, dim, "m=%d,bit_size=4" % m)
    ix.set_codebook(cent, codebooks16(rng, m, dim // m, 0.4))
    ix.add(x, labels)
    ix.build()
    exp = ix.export()
    assert np.diff(exp[2]).tolist() == sizes
    xh = pq.decoded(exp)
    opt("pq_ivf_rpb", "64")  # rounded up to one 256-row step: the 1000-row list spans 4 segments, each with tables of its own
    q = (cent[[0, 1, 2, 3, 5, 1]] + F(0.5) * rng.standard_normal((6, dim), dtype=F)).astype(F)
    for nprobe, k in ((nlist, 100), (2, 10), (1, 256), (3, 1)):
        pq.same(ix.search(q, k, "nprobe=%d" % nprobe), pq.ref_search(exp, xh, q, nprobe, k, L2))
    near = cent[1:2].copy()
    near[0, 0] = 12.0  # between the centroids of lists 1 (at 10) and 2 (at 20), nearer to both than to list 0 (at 0)
    ids, dis = ix.search(near, 10, "nprobe=2")  # lists 1 and 2: four rows for ten slots
    assert (ids[0, :4] >= 0).all() and (ids[0, 4:] == -1).all() and (dis[0, 4:] == FLT_MAX).all()
    ids, dis = ix.search(cent[3:4], 5, "nprobe=1")  # an empty list
    assert (ids == -1).all() and (dis == FLT_MAX).all()
    pq.same(pq.device_search(ix, q, 100, nlist), pq.ref_search(exp, xh, q, nlist, 100, L2))
    ix.close()


def test_twelve_segments(opt):
    """A 3000-row list in 256-row segments: eleven whole ones and one of 184 rows, every one with tables of its own."""
    rng = np.random.default_rng(31)
    dim, m, sizes = 20, 5, [3000, 70]
    cent = np.zeros((2, dim), F)
    cent[1, 0] = 10.0
    home = np.repeat(np.arange(2), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    ix = capi.PqIndex(L2, dim, "m=%d,bit_size=4" % m)
    ix.set_codebook(cent, codebooks16(rng, m, dim // m, 0.4))
    ix.add(x, rng.permutation(9000)[:len(home)].astype(np.int64))
    ix.build()
    exp = ix.export()
    assert np.diff(exp[2]).tolist() == sizes
    xh = pq.decoded(exp)
    opt("pq_ivf_rpb", "64")  # rounded up to one 256-row step
    q = (cent[[0, 1, 0, 0, 1]] + F(0.5) * rng.standard_normal((5, dim), dtype=F)).astype(F)
    for nprobe, k in ((2, 100), (1, 256), (2, 1)):
        pq.same(ix.search(q, k, "nprobe=%d" % nprobe), pq.ref_search(exp, xh, q, nprobe, k, L2))
    pq.same(pq.device_search(ix, q, 256, 2), pq.ref_search(exp, xh, q, 2, 256, L2))
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
        pq.same(ix.search(q, 10, "nprobe=4", alive=alive), pq.ref_search(exp, xh, q, 4, 10, metric, alive=alive))
        pq.same(pq.device_search(ix, q, 10, 4, alive=alive), pq.ref_search(exp, xh, q, 4, 10, metric, alive=alive))
    ids, _ = ix.search(q, 10, "nprobe=%d" % NLIST, alive=none)
    assert (ids == -1).all()
    # a bitmap shorter than the label space: labels at or beyond nbits are dead
    nbits = top // 2
    cut = np.ones(top, bool)
    cut[nbits:] = False
    ref = pq.ref_search(exp, xh, q, NLIST, 10, metric, alive=cut)
    got = ix.search(q, 10, "nprobe=%d" % NLIST, alive=np.ones(nbits, bool), nbits=nbits)
    pq.same(got, ref)
    assert (got[0] < nbits).all()
    pq.same(pq.device_search(ix, q, 10, NLIST, alive=np.ones(nbits, bool)), ref)


# ---------------------------------------------------------------------------------------- 5. special queries

@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_special_queries(metric):
    """NaN, +-inf, overflowing, zero and subnormal queries (test_special_values.special_queries) through a hand-made index."""
    ix, exp, xh, x = by_hand(np.random.default_rng(50 + metric), metric, 100, 20, 8, 3000)
    q, _ = sv.special_queries(x[:64] + F(0.1))
    ref = pq.ref_search(exp, xh, q, sv.NPROBE, sv.K, metric)
    pq.same(ix.search(q, sv.K, "nprobe=%d" % sv.NPROBE), ref)
    pq.same(pq.device_search(ix, q, sv.K, sv.NPROBE), ref)
    ix.close()


# ---------------------------------------------------------------------------------------- 6. lifecycle and errors

def bit_size_of(handle):
    fn = capi.lib().msvs_pq_index_bit_size
    fn.restype = capi.C.c_size_t
    fn.argtypes = [capi.C.c_void_p]
    return fn(handle)


def test_lifecycle_and_errors():
    rng = np.random.default_rng(7)
    dim, m = 16, 4
    _, x = pq.blobs(rng, 500, dim, 4)
    for bad in (3, 0, 16):
        assert pq.code_of(lambda: capi.PqIndex(L2, dim, "m=4,bit_size=%d" % bad)) == capi.ERR_INVALID_ARGUMENT
    assert pq.code_of(lambda: capi.PqIndex(L2, 257, "m=257,bit_size=4")) == capi.ERR_INVALID_ARGUMENT
    assert pq.code_of(lambda: capi.PqIndex(L2, 258, "m=129")) == capi.ERR_INVALID_ARGUMENT  # 8 bits keep their limit ...
    assert pq.code_of(lambda: capi.PqIndex(L2, 258, "m=129,bit_size=8")) == capi.ERR_INVALID_ARGUMENT
    capi.PqIndex(L2, 258, "m=129,bit_size=4").close()  # ... which the 4-bit form does not have
    capi.PqIndex(L2, 8192, "m=256,bit_size=4").close()  # the largest shape
    assert pq.code_of(lambda: capi.PqIndex(L2, 16, "m=3,bit_size=4")) == capi.ERR_INVALID_ARGUMENT  # m does not divide dim
    assert bit_size_of(None) == 0
    ix = capi.PqIndex(L2, dim, "ncentroids=4,m=%d,bit_size=4,kmeans_iters=3" % m)
    assert ix.bits == 4 and bit_size_of(ix._h) == 4
    assert capi.PqIndex(L2, dim, "m=4").bits == 8 and capi.PqIndex(L2, dim, "m=4,bit_size=8").bits == 8
    assert pq.code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # no codebook yet
    assert pq.code_of(lambda: ix.train(x[:15])) == capi.ERR_INVALID_ARGUMENT  # fewer rows than entries of a sub-codebook
    assert pq.code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY
    small = capi.PqIndex(L2, dim, "ncentroids=4,m=%d,bit_size=4,kmeans_iters=3" % m)
    small.train(x[:16])  # as many rows as entries
    assert small.export(with_lists=False)[1].shape == (m, 16, dim // m)
    small.close()
    ix.train(x)
    ix.add(x[:2], np.array([1000, 2 ** 32 - 2]))  # the largest label
    ix.add(x[2:])
    assert pq.code_of(lambda: ix.train(x)) == capi.ERR_INVALID_ARGUMENT  # the codebook is fixed once rows are staged
    ix.build()
    assert ix.ready and ix.num_data == 500 and bit_size_of(ix._h) == 4
    assert pq.code_of(lambda: ix.search(x[:1], 257)) == capi.ERR_UNSUPPORTED_K
    exp = ix.export()
    pq.same(ix.search(x[:4], 3, "nprobe=4"), pq.ref_search(exp, pq.decoded(exp), x[:4], 4, 3, L2))
    store = {}
    ix.serialize_io(store)
    ld = capi.PqIndex.load_io(store)
    assert ld.bits == 4 and bit_size_of(ld._h) == 4
    ld.close()
    ix.close()
    bad = capi.PqIndex(L2, dim, "m=%d,bit_size=4" % m)
    cb = codebooks16(rng, m, dim // m)
    for v in (np.nan, np.inf):
        cb2 = cb.copy()
        cb2[2, 9, 1] = v
        assert pq.code_of(lambda: bad.set_codebook(x[:3], cb2)) == capi.ERR_INVALID_ARGUMENT
        assert pq.code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # a refused codebook leaves none
    bad.set_codebook(x[:3], cb)
    cb2 = cb.copy()
    cb2[0, 0, 0] = np.nan
    assert pq.code_of(lambda: bad.set_codebook(x[:3], cb2)) == capi.ERR_INVALID_ARGUMENT
    assert pq.code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # ... not even the one it had
    bad.close()


def test_bit_size_8_is_the_default_index():
    rng = np.random.default_rng(14)
    _, x = pq.blobs(rng, 1500, 32, NLIST)
    out = []
    for extra in ("", ",bit_size=8"):
        ix = capi.PqIndex(IP, 32, "ncentroids=%d,m=8,kmeans_iters=3%s" % (NLIST, extra))
        ix.train(x)
        ix.add(x)
        ix.build()
        assert ix.bits == 8 and bit_size_of(ix._h) == 8
        store = {}
        ix.serialize_io(store)
        ld = capi.PqIndex.load_io(store)
        assert ld.bits == 8
        ld.close()
        out.append((ix.export(), store, ix.search(x[:9], 10, "nprobe=3")))
        ix.close()
    (e0, s0, r0), (e1, s1, r1) = out
    for a, b in zip(e0, e1):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert e0[1].shape == (8, 256, 4)
    assert bytes(s0["pq_data"]) == bytes(s1["pq_data"]) and bytes(s0["pq_ids"]) == bytes(s1["pq_ids"])
    assert struct.unpack_from("<Q", bytes(s0["pq_data"]), 48)[0] == 0  # the reserved word of an 8-bit file stays 0
    pq.same(r0, r1)


# ---------------------------------------------------------------------------------------- 7. determinism

def test_training_is_deterministic():
    rng = np.random.default_rng(9)
    _, x = pq.blobs(rng, 2000, 32, NLIST)
    exps = []
    for _ in range(2):
        ix = capi.PqIndex(L2, 32, "ncentroids=%d,m=8,bit_size=4,kmeans_iters=5" % NLIST)
        ix.train(x)
        if exps:
            ix.train(x)  # (again on the same object: replaces the codebook with the same one)
        ix.add(x)
        ix.build()
        exps.append(ix.export())
        ix.close()
    for a, b in zip(*exps):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------- 8. memory

def test_memory_usage_is_packed_codes_plus_labels():
    rng = np.random.default_rng(10)
    n, dim, m, nlist = 20000, 64, 32, 16
    _, x = pq.blobs(rng, n, dim, nlist)
    ix = capi.PqIndex(L2, dim, "ncentroids=%d,m=%d,bit_size=4,kmeans_iters=2" % (nlist, m))
    ix.train(x[:4000])
    ix.add(x[:12000])
    ix.add(x[12000:])
    ix.build()
    tables = nlist * dim * 4 + 16 * dim * 4 + (nlist + 1) * 8
    half = (m + 1) // 2
    assert n * half <= ix.memory_usage <= n * ((half + 15) // 16 * 16 + 8) + tables + 4096
    ix.close()


# ---------------------------------------------------------------------------------------- 9. files

def packed(codes):
    """[n, m] codes < 16 -> [n, ceil(m / 2)] bytes: code s in the low nibble of byte s / 2 for even s, else in the high one"""
    n, m = codes.shape
    c = np.zeros((n, (m + 1) // 2 * 2), np.uint8)
    c[:, :m] = codes
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def file_index(metric, dim, m, n):
    """test_coded_index_files.pq_index with 16 integer-valued entries: two lists in use, the third empty, the largest label"""
    rng = np.random.default_rng(dim + n)
    cent, x, labels = cf.rows_and_labels(rng, n, dim)
    ix = capi.PqIndex(metric, dim, "m=%d,bit_size=4" % m)
    ix.set_codebook(cent, rng.integers(-4, 5, (m, 16, dim // m)).astype(F))
    ix.add(x[:n // 3], labels[:n // 3])
    ix.add(x[n // 3:], labels[n // 3:])
    ix.build()
    return ix


# m = 5: one word a row, a pad nibble and a pad byte; 130 rows are two whole blocks of 64 and a partial one.  m = 16, 64 rows: two
# words a row, one block.
@pytest.mark.parametrize("dim,m,n", [(20, 5, 130), (16, 16, 64)])
def test_files_to_the_byte(dim, m, n):
    ix = file_index(L2, dim, m, n)
    cent, cb, off, codes, labels = ix.export()
    assert off[0] == 0 and off[-1] == n and off[2] == off[3] and 0 < off[1] < n
    assert codes.shape == (n, m) and (codes < 16).all() and (labels == 2 ** 32 - 2).sum() == 1
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["pq_data", "pq_ids"]
    data = cf.with_check(b"MSVSPQ01" + struct.pack("<IiQQQQQ", 1, L2, dim, m, 3, n, 4)) + cent.astype("<f4").tobytes() \
        + cb.astype("<f4").tobytes() + off.astype("<i8").tobytes() + packed(codes).tobytes()
    assert cb.size == 16 * dim and len(data) == 64 + 3 * dim * 4 + 16 * dim * 4 + 4 * 8 + n * ((m + 1) // 2)
    assert bytes(store["pq_data"]) == data
    assert bytes(store["pq_ids"]) == cf.id_file(b"MSVSPQID", labels)
    ld = capi.PqIndex.load_io(store, L2, dim, m, 4)
    again = {}
    ld.serialize_io(again)
    assert bytes(again["pq_data"]) == data and bytes(again["pq_ids"]) == bytes(store["pq_ids"])
    ld.close()
    ix.close()


def test_files_round_trip_and_corruption():
    ix, exp, xh, _, _, q = case(IP, 100, 25, "clustered")
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["pq_data", "pq_ids"] and bytes(store["pq_data"][:8]) == b"MSVSPQ01"
    ld = capi.PqIndex.load_io(store)  # nothing repeated by the caller
    assert (ld.metric, ld.dim, ld.m, ld.bits) == (IP, 100, 25, 4)
    assert ld.ready and ld.num_data == ix.num_data and ld.num_lists == NLIST
    for a, b in zip(exp, ld.export()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    pq.same(ld.search(q[:30], 10, "nprobe=3"), pq.ref_search(exp, xh, q[:30], 3, 10, IP))
    ld.close()
    load = lambda s: capi.PqIndex.load_io(s, IP, 100, 25, 4)
    for name in ("pq_data", "pq_ids"):
        full = store[name]
        for cut in (0, 10, len(full) // 2, len(full) - 1):
            bad = dict(store)
            bad[name] = bytearray(full[:cut])
            assert pq.code_of(lambda: load(bad)) == capi.ERR_IO, (name, cut)
        header = 64 if name == "pq_data" else 24
        for pos in range(header):
            bad = dict(store)
            bad[name] = bytearray(full)
            bad[name][pos] ^= 0x01
            assert pq.code_of(lambda: load(bad)) == capi.ERR_IO, (name, pos)
        bad = dict(store)
        bad[name] = bytearray(full) + b"\0"
        assert pq.code_of(lambda: load(bad)) == capi.ERR_IO, name
    full = bytes(store["pq_data"])
    # a reserved word that names no form, and the 8-bit one (n * 25 code bytes expected, n * 13 there), check words recomputed
    for reserved in (2, 0):
        bad = dict(store)
        bad["pq_data"] = bytearray(cf.with_check(full[:48] + struct.pack("<Q", reserved)) + full[64:])
        assert pq.code_of(lambda: load(bad)) == capi.ERR_IO, reserved
    # m = 25 is odd: the high nibble of a row's last byte is padding and must be 0
    assert (np.frombuffer(full[-13 * ix.num_data:], np.uint8).reshape(-1, 13)[:, 12] < 16).all()
    for row in (0, ix.num_data - 1):
        bad = dict(store)
        bad["pq_data"] = bytearray(full)
        bad["pq_data"][len(full) - 13 * (ix.num_data - row) + 12] |= 0x10
        assert pq.code_of(lambda: load(bad)) == capi.ERR_IO, row
    # 4-bit files have their own limit of m, 8-bit files keep theirs: m = 129 .. 256 with reserved = 0 is refused
    big = file_index(L2, 258, 129, 70)
    big_store = {}
    big.serialize_io(big_store)
    capi.PqIndex.load_io(big_store, bits=4).close()
    b = bytes(big_store["pq_data"])
    bad = dict(big_store)
    bad["pq_data"] = bytearray(cf.with_check(b[:48] + struct.pack("<Q", 0)) + b[64:])
    assert pq.code_of(lambda: capi.PqIndex.load_io(bad)) == capi.ERR_IO
    big.close()
    for wrong in ((L2, 100, 25, 4), (IP, 50, 25, 4), (IP, 100, 20, 4), (IP, 100, 25, 8)):  # a caller's mistake is an error
        with pytest.raises(ValueError):
            capi.PqIndex.load_io(store, *wrong)
    with pytest.raises(ValueError):
        capi.PqIndex.load_io(store, bits=8)


# ---------------------------------------------------------------------------------------- 10. recall of the trained index

@pytest.mark.parametrize("metric", [L2, IP])
def test_recall_against_the_original_rows(metric):
    """The data of test_pq_ivf.test_recall_against_the_original_rows (4000 x 64 rows in 8 blobs, sigma 0.3, 8 lists all probed, 100
    queries) at bit_size=4, m = 64: 32 bytes a row.  The share of the exact top-10 of the ORIGINAL rows found in the top-100 must be
    >= 0.95 (the bar of the 8-bit test) -- first for the numpy restatement over the exported codebook, then for the index, which must
    equal it bit for bit (a numpy restatement with 5-iteration Lloyd codebooks gave 0.999 - 1.000 over five seeds for both metrics;
    m = 32 gave 0.948 - 1.000, too close to the bar to use).  Top-10 in top-10 is the quantiser's loss: printed, not asserted."""
    rng = np.random.default_rng(11)
    n, dim, m, nlist, nq = 4000, 64, 64, 8, 100
    centres, x = pq.blobs(rng, n, dim, nlist)
    q = (centres[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    if metric == L2:
        exact = ((q[:, None, :].astype(np.float64) - x[None]) ** 2).sum(-1)
    else:
        exact = -(q.astype(np.float64) @ x.T.astype(np.float64))
    truth = np.argsort(exact, axis=1, kind="stable")[:, :10]
    ix = capi.PqIndex(metric, dim, "ncentroids=%d,m=%d,bit_size=4,kmeans_iters=5" % (nlist, m))
    ix.train(x)
    ix.add(x)
    ix.build()
    exp = ix.export()
    assert exp[1].shape == (m, 16, 1)

    def share(ids, width):
        return np.mean([len(set(t.tolist()) & set(g[:width].tolist())) / 10 for t, g in zip(truth, ids)])

    ref = pq.ref_search(exp, pq.decoded(exp), q, nlist, 100, metric)
    print("reference: 10 in 100 %.3f, 10 in 10 %.3f" % (share(ref[0], 100), share(ref[0], 10)))
    assert share(ref[0], 100) >= 0.95
    got = ix.search(q, 100, "nprobe=%d" % nlist)
    print("index: 10 in 100 %.3f, 10 in 10 %.3f" % (share(got[0], 100), share(got[0], 10)))
    assert share(got[0], 100) >= 0.95
    pq.same(got, ref)
    ix.close()
