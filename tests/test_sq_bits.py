"""The 4-bit and binary16 forms of the IVFSQ index (bit_size=4 / 16): the same index, lists, scan arithmetic and files as the 8-bit
form (test_sq_ivf.py) with another code word.

The reference is composed as there, from the semantics in include/msvs.h alone: a numpy encode / decode per width (every step
rounded to f32; at 16 bits `(x - c).astype(float16).astype(float32)`), X^ = decode(exported codes), oracle.ivf_search over X^.
Every comparison is == on ids and on the uint32 view of the distances."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_coded_index_files as cf
import test_sq_ivf as sq
from oracle import oracle as o
from test_refine import store_of
from test_sq_ivf import blobs, code_of, lists_of, ref_search, same, stored

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
FLT_MAX = np.finfo(np.float32).max
NLIST = sq.NLIST
WIDTHS = [4, 16]


def params(bits, rest=""):
    """an 8-bit index is created as it always was"""
    own = "" if bits == 8 else "bit_size=%d" % bits
    return ",".join(p for p in (rest, own) if p)


def step_of(vmin, vmax, bits):
    return ((vmax - vmin).astype(F) / F(15 if bits == 4 else 255)).astype(F)


def encode(x, c, vmin, vmax, bits):
    """x: stored rows, c: the centroid of each row's list -> uint8 codes, or the uint16 bit patterns of the binary16 residuals"""
    r = (x - c).astype(F)
    if bits == 16:
        with np.errstate(over="ignore"):
            return r.astype(np.float16).view(np.uint16)
    step = step_of(vmin, vmax, bits)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((r - vmin).astype(F) / step).astype(F)
    code = np.clip(np.rint(t), 0, 15 if bits == 4 else 255)
    code[:, step == 0] = 0
    return code.astype(np.uint8)


def decode(codes, c, vmin, vmax, bits):
    if bits == 16:
        with np.errstate(invalid="ignore"):
            return (c + codes.view(np.float16).astype(F)).astype(F)
    step = step_of(vmin, vmax, bits)
    return (c + (vmin + (codes.astype(F) * step).astype(F)).astype(F)).astype(F)


def decoded(exp, bits):
    cent, lo, hi, off, codes, labels = exp
    return decode(codes, cent[lists_of(off)], lo, hi, bits)


def bit_size_of(handle):
    fn = capi.lib().msvs_sq_index_bit_size
    fn.restype, fn.argtypes = capi.C.c_size_t, [capi.C.c_void_p]
    return fn(handle)


def build_case(bits, metric, dim, data, labelled=True):
    rng = np.random.default_rng(dim * 13 + metric * 5 + len(data))
    n = 3000
    centres, x = blobs(rng, n, dim, NLIST)
    if data == "ties":  # 40 distinct vectors: equal distances everywhere, ordered by label
        x = np.ascontiguousarray(x[:40][rng.integers(0, 40, n)])
    labels = rng.permutation(3 * n)[:n].astype(np.int64) if labelled else np.arange(n, dtype=np.int64)  # shuffled, not contiguous
    q = (centres[rng.integers(0, NLIST, 300)] + F(0.3) * rng.standard_normal((300, dim), dtype=F)).astype(F)
    ix = capi.SqIndex(metric, dim, params(bits, "ncentroids=%d,kmeans_iters=4" % NLIST))
    ix.train(x)
    for a, b in ((0, 1100), (1100, 1101), (1101, n)):
        ix.add(x[a:b], labels[a:b] if labelled else None)
    ix.build()
    exp = ix.export()
    return ix, exp, decoded(exp, bits), x, labels, q


@functools.lru_cache(maxsize=None)
def case(bits, metric, dim, data):
    """test_sq_ivf.case at another width: a trained and built index of 3000 rows in three chunks, its export, the decoded matrix and
    300 queries; computed once."""
    return build_case(bits, metric, dim, data)


def row_bound(bits, dim):
    """bytes of a stored row and its label, as include/msvs.h bounds them"""
    up = lambda v: (v + 15) // 16 * 16
    return {4: up((dim + 1) // 2), 8: up(dim), 16: 2 * up(dim)}[bits] + 8


# ---------------------------------------------------------------------------------------- 1. structure and codes

@pytest.mark.parametrize("dim", [5, 31, 64, 100, 520, 768])  # odd (a pad nibble), tail only, a 512-block and a tail, whole blocks
@pytest.mark.parametrize("bits", WIDTHS)
def test_structure_codes_and_trained_range(bits, dim):
    metric = (L2, IP, COS)[dim % 3]
    ix, exp, _, x, labels, _ = case(bits, metric, dim, "clustered")
    cent, lo, hi, off, codes, elab = exp
    n = len(x)
    assert ix.bits == bits and bit_size_of(ix._h) == bits
    assert ix.ready and ix.num_data == n and ix.num_lists == NLIST
    assert len(off) == NLIST + 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert sorted(elab.tolist()) == sorted(labels.tolist())
    for l in range(NLIST):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    where = {int(l): i for i, l in enumerate(labels)}
    xs = stored(x, metric)[[where[int(l)] for l in elab]]  # the fed rows in export order
    lists = lists_of(off)
    assert codes.dtype == (np.uint16 if bits == 16 else np.uint8) and codes.shape == (n, dim)
    assert codes.tobytes() == encode(xs, cent[lists], lo, hi, bits).tobytes()
    if bits == 4:
        assert (codes < 16).all()
    # the rows fed ARE the training rows: their residuals against their exported lists' centroids give the trained range (all widths)
    r = (xs - cent[lists]).astype(F)
    assert (lo == r.min(axis=0)).all() and (hi == r.max(axis=0)).all()
    tables = NLIST * dim * 4 + 2 * dim * 4 + (NLIST + 1) * 8
    assert n * dim * bits // 8 <= ix.memory_usage <= n * row_bound(bits, dim) + tables + 4096


@pytest.mark.parametrize("bits", WIDTHS)
def test_two_builds_give_the_same_bytes(bits):
    a, b = build_case(bits, L2, 100, "clustered"), build_case(bits, L2, 100, "clustered")
    for u, v in zip(a[1], b[1]):
        assert u.tobytes() == v.tobytes()
    a[0].close()
    b[0].close()


# ---------------------------------------------------------------------------------------- 2. search parity

PARITY = [
    # nq = 1: tile 2 with a repeated pair; 7: tile 4 from two pairs a list on; 300: tile 8 (tile 4 at k = 256, by the tile's LDS)
    (L2, 5, "clustered", 1, 1, 1, "host"),
    (L2, 64, "clustered", 7, 10, 4, "device"),
    (L2, 100, "ties", 7, 256, NLIST, "host"),
    (L2, 520, "clustered", 300, 10, 4, "host"),
    (L2, 768, "clustered", 300, 10, 4, "device"),
    (L2, 768, "clustered", 7, 256, 10 * NLIST, "device"),
    (L2, 64, "ties", 300, 256, NLIST, "host"),
    (IP, 5, "ties", 300, 10, NLIST, "device"),
    (IP, 64, "clustered", 1, 256, 4, "host"),
    (IP, 100, "clustered", 300, 10, 1, "host"),
    (IP, 520, "ties", 7, 1, NLIST, "device"),
    (IP, 768, "ties", 1, 10, 10 * NLIST, "device"),
    (COS, 5, "clustered", 7, 10, 4, "host"),
    (COS, 64, "ties", 300, 1, NLIST, "host"),
    (COS, 100, "clustered", 1, 256, 10 * NLIST, "device"),
    (COS, 520, "clustered", 300, 256, 2, "host"),
    (COS, 768, "clustered", 7, 10, 1, "host"),
    # 64 < k <= 128 (two top-k registers a lane) at tile 2 and tile 8
    (L2, 64, "clustered", 1, 100, 4, "host"),
    (IP, 5, "ties", 300, 100, NLIST, "device"),
]


@pytest.mark.parametrize("metric,dim,data,nq,k,nprobe,entry", PARITY)
@pytest.mark.parametrize("bits", WIDTHS)
def test_search_parity(bits, metric, dim, data, nq, k, nprobe, entry):
    ix, exp, xh, _, _, q = case(bits, metric, dim, data)
    q = q[:nq]
    got = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else sq.device_search(ix, q, k, nprobe)
    same(got, ref_search(exp, xh, q, nprobe, k, metric))


@pytest.mark.parametrize("dim", [20, 531])  # the tail alone; a block (two at 16 bits ... four), then an odd tail
@pytest.mark.parametrize("bits", WIDTHS)
def test_empty_short_and_segmented_lists(opt, bits, dim):
    rng = np.random.default_rng(3 + dim)
    sizes = [1000, 3, 1, 0, 0, 50, 15, 16, 17]  # empty lists, lists around one 16-row step, one of many segments
    nlist = len(sizes)
    cent = np.zeros((nlist, dim), F)
    cent[:, 0] = 10.0 * np.arange(nlist)
    home = np.repeat(np.arange(nlist), sizes)
    x = (cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    labels = rng.permutation(5000)[:len(home)].astype(np.int64)
    ix = capi.SqIndex(L2, dim, params(bits))
    ix.set_codebook(cent, np.full(dim, -2, F), np.full(dim, 2, F))
    ix.add(x, labels)
    ix.build()
    exp = ix.export()
    assert np.diff(exp[3]).tolist() == sizes
    xh = decoded(exp, bits)
    q = (cent[[0, 1, 2, 3, 5, 1, 6, 7, 8]] + F(0.5) * rng.standard_normal((9, dim), dtype=F)).astype(F)
    for rpb in ("64", "16"):  # the 1000-row list spans 16 segments; then every list longer than 16 rows spans several
        opt("sq_ivf_rpb", rpb)
        for nprobe, k in ((nlist, 100), (2, 10), (1, 256), (3, 1)):
            same(ix.search(q, k, "nprobe=%d" % nprobe), ref_search(exp, xh, q, nprobe, k, L2))
        same(sq.device_search(ix, q, 100, nlist), ref_search(exp, xh, q, nlist, 100, L2))
    between = q[1:2].copy()
    between[0, 0] = 14  # nearer to the centroids of lists 1 and 2 (10, 20) than to list 0's
    ids, dis = ix.search(between, 10, "nprobe=2")  # lists 1 and 2: four rows for ten slots
    assert (ids[0, :4] >= 0).all() and (ids[0, 4:] == -1).all() and (dis[0, 4:] == FLT_MAX).all()
    ids, dis = ix.search(q[3:4], 5, "nprobe=1")  # an empty list
    assert (ids == -1).all() and (dis == FLT_MAX).all()
    ix.close()


# ---------------------------------------------------------------------------------------- 3. the LDS edge

@pytest.mark.parametrize("bits", WIDTHS)
def test_largest_dimension_at_the_lds_edge(bits):
    """d = 2240, k = 256, as test_sq_ivf's: the 8-bit LDS image of the smallest tile is 65280 of 65536 bytes, and the dimension limit is
    that image's at every width."""
    rng = np.random.default_rng(12)
    dim, nlist, n = 2240, 4, 600
    centres, x = blobs(rng, n, dim, nlist)
    ix = capi.SqIndex(IP, dim, params(bits))
    ix.set_codebook(centres, np.full(dim, -1.5, F), np.full(dim, 1.5, F))
    ix.add(x, np.arange(n, dtype=np.int64) * 3)
    ix.build()
    exp = ix.export()
    xh = decoded(exp, bits)
    q = x[:40] + F(0.1)
    for k in (256, 10):
        same(ix.search(q, k, "nprobe=%d" % nlist), ref_search(exp, xh, q, nlist, k, IP))
    same(sq.device_search(ix, q[:3], 256, 2), ref_search(exp, xh, q[:3], 2, 256, IP))
    ix.close()
    for b in (4, 8, 16):
        assert code_of(lambda: capi.SqIndex(L2, 4096, params(b))) == capi.ERR_INVALID_ARGUMENT  # beyond the scan's LDS stage, at every width
        assert code_of(lambda: capi.SqIndex(L2, 2241, params(b))) == capi.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------- 4. 4-bit corners

def test_4bit_constant_dimension_and_rows_outside_the_range():
    rng = np.random.default_rng(4)
    dim, n = 24, 2000
    centres, x = blobs(rng, n, dim, NLIST)
    x[:, 7] = 0  # constant over the training rows (and so over the centroids: every residual there is 0)
    ix = capi.SqIndex(L2, dim, "ncentroids=%d,kmeans_iters=4,bit_size=4" % NLIST)
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
    zero_step = step_of(lo, hi, 4) == 0
    assert zero_step[7] and lo[7] == hi[7]
    where = labels // 2
    assert (codes == encode(allx[where], cent[lists], lo, hi, 4)).all()
    xh = decoded(exp, 4)
    assert (codes[:, zero_step] == 0).all()
    assert (xh[:, zero_step] == (cent[lists] + lo).astype(F)[:, zero_step]).all()
    out = where >= n
    assert out.sum() == 6
    moving = ~zero_step
    assert (codes[out][labels[out] < 2 * (n + 3)][:, moving] == 15).all() and (codes[out][labels[out] >= 2 * (n + 3)][:, moving] == 0).all()
    q = np.concatenate([far, x[:10]])
    same(ix.search(q, 10, "nprobe=%d" % NLIST), ref_search(exp, xh, q, NLIST, 10, L2))
    ix.close()


def test_4bit_ties_and_step_zero_by_hand():
    """vmin = 0, vmax = 15: step is exactly 1, so t = r, and a residual of c + 0.5 is a tie that goes to the even code; one column
    with an empty range."""
    dim = 19
    cent = np.zeros((2, dim), F)
    cent[1] = 100
    lo, hi = np.zeros(dim, F), np.full(dim, 15, F)
    lo[5] = hi[5] = F(0.375)
    halves = (np.arange(-1, 17, dtype=F) + F(0.5))  # -0.5, 0.5, ..., 16.5
    x = np.zeros((len(halves), dim), F)
    x[:] = halves[:, None]
    x[:, 1] += F(0.25)  # no tie there
    x = np.concatenate([x, x + F(100)])
    ix = capi.SqIndex(L2, dim, "bit_size=4")
    ix.set_codebook(cent, lo, hi)
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent_, lo_, hi_, off, codes, labels = exp
    assert np.diff(off).tolist() == [len(halves)] * 2 and (labels == np.arange(len(x))).all()
    assert codes.tobytes() == encode(x, cent[lists_of(off)], lo, hi, 4).tobytes()
    even = [0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 15, 15]  # rint(-0.5) = -0 -> 0; 15.5 -> 16 -> 15; 16.5 -> 15
    assert codes[:len(halves), 0].tolist() == even and codes[len(halves):, 18].tolist() == even
    assert (codes[:, 5] == 0).all()
    xh = decoded(exp, 4)
    assert (xh[:, 5] == (cent[lists_of(off)][:, 5] + F(0.375)).astype(F)).all()
    q = x[::3] + F(0.1)
    same(ix.search(q, 20, "nprobe=2"), ref_search(exp, xh, q, 2, 20, L2))
    ix.close()


# ---------------------------------------------------------------------------------------- 5. binary16 corners

@pytest.mark.parametrize("metric", [L2, IP])
def test_fp16_corners_by_hand(metric):
    """Residuals placed by hand (zero centroids): binary16 subnormals, underflow to +-0, ties to even, the largest finite value and
    what rounds to it, and one residual that overflows to +inf.  One special column inside a whole block, one in the tail."""
    rng = np.random.default_rng(21)
    dim = 136
    vals = np.array([1e-6, -1e-6, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65504, 65519, -65519,
                     6.1e-5, 65520], F)
    want = [0x0011, 0x8011, 0x0000, 0x8000, 0x0001, 0x3c00, 0x3c02, 0xbc00, 0x7bff, 0x7bff, 0xfbff, 0x03ff, 0x7c00]
    x = (F(0.5) * rng.standard_normal((200, dim), dtype=F)).astype(F)
    x[:len(vals), 3] = vals
    x[:len(vals), 130] = vals[::-1]
    cent = np.zeros((2, dim), F)
    ix = capi.SqIndex(metric, dim, "bit_size=16")
    ix.set_codebook(cent, np.full(dim, -1, F), np.full(dim, 1, F))  # (the range enters no arithmetic: nothing is clamped to it)
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent_, lo, hi, off, codes, labels = exp
    assert (lo == -1).all() and (hi == 1).all()
    assert codes.dtype == np.uint16 and codes.tobytes() == encode(x[labels], cent[lists_of(off)], lo, hi, 16).tobytes()
    at = {int(l): i for i, l in enumerate(labels)}
    assert [int(codes[at[i], 3]) for i in range(len(vals))] == want
    assert [int(codes[at[i], 130]) for i in range(len(vals))] == want[::-1]
    xh = decoded(exp, 16)
    assert np.isinf(xh).sum() == 2 and not np.isnan(xh).any()
    q = (F(0.5) * rng.standard_normal((12, dim), dtype=F)).astype(F)
    q[:, [3, 130]] = np.abs(q[:, [3, 130]]) + F(0.1)  # (no 0 * inf)
    for k in (10, 200):
        same(ix.search(q, k, "nprobe=2"), ref_search(exp, xh, q, 2, k, metric))
    ix.close()


# ---------------------------------------------------------------------------------------- 6. filter by label

@pytest.mark.parametrize("metric", [L2, COS])
@pytest.mark.parametrize("bits", WIDTHS)
def test_filter_by_label(bits, metric):
    ix, exp, xh, _, labels, q = case(bits, metric, 64, "clustered")
    q = q[:20]
    rng = np.random.default_rng(6)
    top = int(labels.max()) + 1
    half = rng.random(top) < 0.5
    one = np.zeros(top, bool)
    one[labels[17]] = True
    none = np.zeros(top, bool)
    for alive in (half, one, none):
        same(ix.search(q, 10, "nprobe=4", alive=alive), ref_search(exp, xh, q, 4, 10, metric, alive=alive))
    same(sq.device_search(ix, q, 10, NLIST, alive=half), ref_search(exp, xh, q, NLIST, 10, metric, alive=half))
    nbits = top // 2  # a bitmap shorter than the label space: labels at or beyond nbits are dead
    cut = np.ones(top, bool)
    cut[nbits:] = False
    got = ix.search(q, 10, "nprobe=%d" % NLIST, alive=np.ones(nbits, bool), nbits=nbits)
    same(got, ref_search(exp, xh, q, NLIST, 10, metric, alive=cut))
    assert (got[0] < nbits).all()


# ---------------------------------------------------------------------------------------- 7. rounds and refine

@functools.lru_cache(maxsize=None)
def plain_case(bits, metric):
    """labels = positions, the row store's rule"""
    return build_case(bits, metric, 100, "clustered", labelled=False)


@pytest.mark.parametrize("metric", [L2, COS])
@pytest.mark.parametrize("bits", WIDTHS)
def test_rounds_and_refine(bits, metric):
    """k = 600 and kc = 300 run the later rank rounds (the scan's AFTER form) of both widths."""
    ix, exp, xh, x, _, q = plain_case(bits, metric)
    q = q[:12]
    same(ix.search_rounds(q, 600, "nprobe=%d" % NLIST), ref_search(exp, xh, q, NLIST, 600, metric))
    same(ix.search_rounds(q[:1], 300, "nprobe=2"), ref_search(exp, xh, q[:1], 2, 300, metric))
    rows = store_of(x, metric)
    same(ix.search_refine(rows, q, 10, 50, "nprobe=4"), capi.refine(rows, metric, q, ix.search(q, 50, "nprobe=4")[0], 10))
    same(ix.search_refine_rounds(rows, q, 10, 300, "nprobe=4"), capi.refine(rows, metric, q, ix.search_rounds(q, 300, "nprobe=4")[0], 10))
    same(ix.search_rounds(q, 300, "nprobe=4"), ref_search(exp, xh, q, 4, 300, metric))


# ---------------------------------------------------------------------------------------- 8. files

@pytest.mark.parametrize("bits,dim", [(4, 5), (4, 100), (16, 100)])
def test_files_round_trip_and_corruption(bits, dim):
    ix, exp, xh, _, _, q = case(bits, IP, dim, "clustered")
    n = ix.num_data
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["sq_data", "sq_ids"]
    full = bytes(store["sq_data"])
    assert full[:8] == b"MSVSSQ01" and struct.unpack_from("<Q", full, 40)[0] == bits  # the header's `reserved` word
    body = NLIST * dim * 4 + 2 * dim * 4 + (NLIST + 1) * 8
    assert len(full) == 56 + body + n * {4: (dim + 1) // 2, 16: 2 * dim}[bits]
    if bits == 4:  # the codes section: code j in the low (even j) or high nibble of byte j / 2
        sect = np.frombuffer(full, np.uint8, offset=56 + body).reshape(n, -1)
        nib = np.stack([sect & 15, sect >> 4], axis=2).reshape(n, -1)
        assert (nib[:, :dim] == exp[4]).all() and (nib[:, dim:] == 0).all()
    else:
        assert full[56 + body:] == exp[4].astype("<u2").tobytes()
    ld = capi.SqIndex.load_io(store, IP, dim, bits=bits)
    assert ld.ready and ld.num_data == n and ld.num_lists == NLIST and ld.bits == bits and bit_size_of(ld._h) == bits
    for a, b in zip(exp, ld.export()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    same(ld.search(q[:30], 10, "nprobe=3"), ix.search(q[:30], 10, "nprobe=3"))
    same(ld.search(q[:30], 10, "nprobe=3"), ref_search(exp, xh, q[:30], 3, 10, IP))
    ld.close()
    capi.SqIndex.load_io(store).close()
    with pytest.raises(ValueError):
        capi.SqIndex.load_io(store, IP, dim, bits=8)
    for name in ("sq_data", "sq_ids"):
        whole = store[name]
        for cut in (0, 10, len(whole) // 2, len(whole) - 1):
            bad = dict(store)
            bad[name] = bytearray(whole[:cut])
            assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO, (name, cut)
        for pos in range(56 if name == "sq_data" else 24):
            bad = dict(store)
            bad[name] = bytearray(whole)
            bad[name][pos] ^= 0x01
            assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO, (name, pos)
        bad = dict(store)
        bad[name] = bytearray(whole) + b"\0"
        assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO, name
    for word in (5, 8, 1, 32, 1 << 32 | bits):  # a width that does not exist (8 is written as 0), under a correct check word
        bad = dict(store)
        bad["sq_data"] = bytearray(cf.with_check(full[:40] + struct.pack("<Q", word)) + full[56:])
        assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO, word
    if bits == 4 and dim % 2:
        bad = dict(store)
        bad["sq_data"] = bytearray(full)
        bad["sq_data"][-1] |= 0x10  # the last row's pad nibble; the header and its check word are untouched
        assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO


def test_8bit_files_are_what_they_were():
    """bit_size=8 and no bit_size at all: the same index, the same bytes, `reserved` 0."""
    rng = np.random.default_rng(31)
    _, x = blobs(rng, 700, 37, NLIST)
    stores = []
    for own in ("", ",bit_size=8"):
        ix = capi.SqIndex(L2, 37, "ncentroids=%d,kmeans_iters=3%s" % (NLIST, own))
        assert ix.bits == 8 and bit_size_of(ix._h) == 8
        ix.train(x)
        ix.add(x)
        ix.build()
        exp = ix.export()
        assert exp[4].dtype == np.uint8 and exp[4].tobytes() == sq.encode(x[exp[5]], exp[0][lists_of(exp[3])], exp[1], exp[2]).tobytes()
        stores.append({})
        ix.serialize_io(stores[-1])
        ix.close()
    assert stores[0] == stores[1]
    data = bytes(stores[0]["sq_data"])
    assert struct.unpack_from("<Q", data, 40)[0] == 0 and len(data) == 56 + NLIST * 37 * 4 + 2 * 37 * 4 + (NLIST + 1) * 8 + 700 * 37
    ld = capi.SqIndex.load_io(stores[0], bits=8)
    assert ld.bits == 8
    ld.close()
    assert bit_size_of(None) == 0


# ---------------------------------------------------------------------------------------- 9. errors

def test_bit_size_values():
    for bad in (0, 6, 12, 32):
        assert code_of(lambda: capi.SqIndex(L2, 16, "bit_size=%d" % bad)) == capi.ERR_INVALID_ARGUMENT
        assert code_of(lambda: capi.SqIndex(L2, 16, "ncentroids=4,bit_size=%d" % bad)) == capi.ERR_INVALID_ARGUMENT
    for good in (4, 8, 16):
        ix = capi.SqIndex(COS, 16, "bit_size=%d" % good)
        assert ix.bits == good
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_lifecycle_and_errors(bits):
    rng = np.random.default_rng(7)
    dim = 16
    _, x = blobs(rng, 500, dim, 4)
    ix = capi.SqIndex(L2, dim, "ncentroids=4,kmeans_iters=3,bit_size=%d" % bits)
    assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # no codebook yet
    assert code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY
    ix.train(x)
    assert not ix.ready
    assert code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY  # not built yet
    assert code_of(lambda: ix.serialize_io({})) == capi.ERR_NOT_READY
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
    assert code_of(lambda: ix.search_rounds(x[:1], 4097)) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: ix.search(x[:1], 1, "nprobe=0")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: ix.search(x[:1], 1, "efsearch=3")) == capi.ERR_INVALID_ARGUMENT
    ids, dis = ix.search(x[:3], 0)  # k = 0: nothing to return, as everywhere in the library
    assert ids.shape == (3, 0) and dis.shape == (3, 0)
    ids, _ = ix.search(x[:1], 1, "nprobe=4")
    assert ids[0, 0] == 1000
    assert code_of(lambda: capi.SqIndex(capi.METRIC_HAMMING, dim, "bit_size=%d" % bits)) == capi.ERR_NOT_IMPLEMENTED
    assert code_of(lambda: capi.SqIndex(L2, 0, "bit_size=%d" % bits)) == capi.ERR_INVALID_ARGUMENT
    bad = capi.SqIndex(L2, dim, "bit_size=%d" % bits)
    cent, lo, hi = x[:3], np.full(dim, -1, F), np.full(dim, 1, F)
    for j, (a, b) in enumerate(((1.0, -1.0), (np.nan, 1.0), (-1.0, np.inf))):  # validated at 16 bits too, where they enter no arithmetic
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j], hi2[j] = a, b
        assert code_of(lambda: bad.set_codebook(cent, lo2, hi2)) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: bad.add(x)) == capi.ERR_NOT_READY  # a refused codebook leaves none


def small_index(bits, dim=16):
    rng = np.random.default_rng(70 + bits)
    _, x = blobs(rng, 500, dim, 4)
    x[:, 5] = np.abs(x[:, 5]) + F(1)  # (every centroid is positive there: a row with +inf in that column has a nearest one)
    return x, "ncentroids=4,kmeans_iters=3,bit_size=%d" % bits


@pytest.mark.parametrize("bits", [8, 4, 16])
def test_a_quantiser_without_a_finite_step_is_refused(bits):
    """vmin = -3e38, vmax = 3e38 are finite and ordered, but fl(vmax - vmin) = inf: the step is infinite, every code of the column is
    0 and decodes to vmin + 0 * inf = NaN, and the index would build, save, load and never return a row.  At 8 and 4 bits set_codebook
    and train refuse it (MSVS_ERR_INVALID_ARGUMENT, no codebook left) and load does (MSVS_ERR_IO); one infinite element among the
    training rows is enough for train.  At 16 bits the range enters no arithmetic and all three accept it, as they did."""
    dim, j = 16, 5
    x, params_ = small_index(bits, dim)
    cent = np.ascontiguousarray(x[:4])
    lo, hi = np.full(dim, -1, F), np.full(dim, 1, F)
    lo[j], hi[j] = -3e38, 3e38
    q = x[:20] + F(0.05)
    # set_codebook
    ix = capi.SqIndex(L2, dim, "bit_size=%d" % bits)
    if bits == 16:
        ix.set_codebook(cent, lo, hi)
        ix.add(x)
        ix.build()
        assert (ix.search(q, 5, "nprobe=4")[0] >= 0).all()
    else:
        with pytest.raises(capi.MsvsError) as e:
            ix.set_codebook(cent, lo, hi)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "dimension %d" % j in str(e.value)
        assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY  # a refused codebook leaves none
        lo[j], hi[j] = -1.7e38, 1.7e38  # the widest kind of range that has a finite step: accepted
        ix.set_codebook(cent, lo, hi)
        ix.add(x)
        ix.build()
        exp = ix.export()
        same(ix.search(q, 5, "nprobe=4"), ref_search(exp, decoded(exp, bits), q, 4, 5, L2))
    ix.close()
    # train: one +inf element among the training rows
    xi = x.copy()
    xi[123, j] = np.inf
    ix = capi.SqIndex(L2, dim, params_)
    if bits == 16:
        ix.train(xi)
        assert ix.export(with_lists=False)[2][j] == np.inf  # the exact range of the training residuals, as the header promises
    else:
        with pytest.raises(capi.MsvsError) as e:
            ix.train(xi)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT and "dimension %d" % j in str(e.value)
        assert code_of(lambda: ix.add(x)) == capi.ERR_NOT_READY and ix.num_lists == 0  # untrained
        ix.train(x)  # ... and trainable
        ix.add(x)
        ix.build()
        assert (ix.search(q, 5, "nprobe=4")[0] >= 0).all()
    ix.close()
    # load: a file whose range has been patched, under a correct header check word
    ix = capi.SqIndex(L2, dim, params_)
    ix.train(x)
    ix.add(x)
    ix.build()
    want = ix.search(q, 5, "nprobe=4")
    store = {}
    ix.serialize_io(store)
    ix.close()
    full = bytes(store["sq_data"])
    at_lo = 56 + 4 * dim * 4 + 4 * j
    at_hi = at_lo + 4 * dim
    for a, b in ((-3e38, 3e38), (-1.0, np.inf), (np.nan, 1.0)):
        body = bytearray(full[56:])
        body[at_lo - 56:at_lo - 52] = struct.pack("<f", a)
        body[at_hi - 56:at_hi - 52] = struct.pack("<f", b)
        bad = dict(store)
        bad["sq_data"] = bytearray(cf.with_check(full[:48]) + bytes(body))
        if bits == 16:
            ld = capi.SqIndex.load_io(bad)
            same(ld.search(q, 5, "nprobe=4"), want)
            ld.close()
        else:
            assert code_of(lambda: capi.SqIndex.load_io(bad)) == capi.ERR_IO, (a, b)
    good = dict(store)
    good["sq_data"] = bytearray(cf.with_check(full[:48]) + full[56:])
    ld = capi.SqIndex.load_io(good)
    same(ld.search(q, 5, "nprobe=4"), want)
    ld.close()


# ---------------------------------------------------------------------------------------- 10. quality of the specification

@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("bits", WIDTHS)
def test_recall_against_the_original_rows(bits, metric):
    """The semantics, not the kernel, in the set-up of test_sq_ivf's test of this name: 8192 x 64 rows in 32 blobs, the quantiser
    trained on every second row, every list probed; first the numpy restatement, then the index, then their equality.
    16 bits: recall@10 against the exact search of the ORIGINAL rows >= 0.99 (0.9990 - 1.000 over three seeds in a stand-alone
    restatement with a plain k-means: at most 2 misses in 2000 slots, the bound allows 20).
    4 bits: the share of the exact top-10 inside the form's top-50 >= 0.95, the project's recall contract (0.9985 - 1.000 there);
    search_refine(k = 10, kc = 50) over the original rows returns exactly those, so the same share is its recall@10.  The plain
    4-bit recall@10 (0.73 - 0.77 there) is printed, not asserted."""
    rng = np.random.default_rng(11)
    n, dim, nlist, nq, k = 8192, 64, 32, 200, 10
    centres, x = blobs(rng, n, dim, nlist)
    q = (centres[rng.integers(0, nlist, nq)] + F(0.3) * rng.standard_normal((nq, dim), dtype=F)).astype(F)
    om = o.METRIC_L2 if metric == L2 else o.METRIC_IP
    truth, _ = o.knn(q, x, k, om)
    ix = capi.SqIndex(metric, dim, "ncentroids=%d,kmeans_iters=6,bit_size=%d" % (nlist, bits))
    ix.train(x[::2])
    ix.add(x)
    ix.build()
    exp = ix.export()
    cent, lo, hi, off, codes, labels = exp
    lists = lists_of(off)
    xh = decode(encode(x[labels], cent[lists], lo, hi, bits), cent[lists], lo, hi, bits)

    def share(ids):
        """of the exact top-10, the part found among ids (its recall@10 where ids has 10 columns)"""
        return np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, truth)])

    depth = 10 if bits == 16 else 50
    floor = 0.99 if bits == 16 else 0.95
    ref_ids, ref_dis, _ = o.ivf_search(cent, off, xh, labels, q, nlist, depth, om)
    r_ref = share(ref_ids)
    print("bits %d: share of the exact top-10 in the reference's top-%d: %.4f" % (bits, depth, r_ref))
    assert r_ref >= floor
    got = ix.search(q, depth, "nprobe=%d" % nlist)
    r_ix = share(got[0])
    print("bits %d: share of the exact top-10 in the index's top-%d: %.4f" % (bits, depth, r_ix))
    assert r_ix >= floor
    same(got, (ref_ids, ref_dis))
    if bits == 4:
        print("bits 4: plain recall@10 of the index: %.4f" % share(got[0][:, :k]))
        rows = store_of(x, metric)
        fine = ix.search_refine(rows, q, k, depth, "nprobe=%d" % nlist)
        r_fine = share(fine[0])
        print("bits 4: recall@10 after search_refine(kc = 50): %.4f" % r_fine)
        assert r_fine >= floor and r_fine == r_ix
    ix.close()
