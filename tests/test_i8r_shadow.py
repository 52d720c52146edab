"""The int8 residual form of the IVF list shadow (h16_scan_kernels.hpp, "i8r"): the operand map of v_mfma_i32_32x32x32_i8 as the
scan uses it, the error bound of set_error_model_i8r on the hardware, bit-exact parity with the oracle under the forced forms, and
the auto rule that picks the form at build time."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o


def same(a_ids, a_dis, b_ids, b_dis):
    assert np.array_equal(a_ids, b_ids), "ids differ"
    assert np.array_equal(a_dis.view(np.uint32), b_dis.view(np.uint32)), "distances differ"


def shadow_form(ix):
    capi.lib().msvs_debug_shadow_form.restype = C.c_int
    return capi.lib().msvs_debug_shadow_form(ix._h)


def build_ivf(x, nlist, params="", centroids=None, ids=None):
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, x.shape[1], "ncentroids=%d,kmeans_iters=5%s" % (nlist, params))
    if centroids is not None:
        ix.set_centroids(centroids)
    else:
        ix.train(x)
    half = x.shape[0] // 2
    ix.add(x[:half], None if ids is None else ids[:half])
    ix.add(x[half:], None if ids is None else ids[half:])
    ix.build()
    return ix


def oracle(ix, q, nprobe, k, alive=None):
    cent, off, vecs, lids = ix.export()
    return o.ivf_search(cent, off, vecs, lids, q, nprobe, k, o.METRIC_L2, alive=alive)


def blobs(rng, nblob, n, nq, d, sigma=0.3):
    c = rng.standard_normal((nblob, d), dtype=np.float32)
    x = (c[rng.integers(0, nblob, n)] + sigma * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    q = (c[rng.integers(0, nblob, nq)] + sigma * rng.standard_normal((nq, d), dtype=np.float32)).astype(np.float32)
    return x, q


def last_keys(nq, cap):
    keys = np.zeros((nq, cap), np.uint64)
    cnt = np.zeros(nq, np.uint32)
    rc = capi.lib().msvs_debug_h16_keys(keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(cap), cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        C.c_size_t(nq))
    assert rc == 0, capi.lib().msvs_last_error()
    return keys, cnt


def key_values(kk):
    o_ = (kk >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o_ & np.uint32(0x80000000), o_ & np.uint32(0x7FFFFFFF), ~o_).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def i8r_bound(d, nq):
    cd = np.zeros(nq, np.float64)
    cn, cc, ran = C.c_double(), C.c_double(), C.c_int()
    rc = capi.lib().msvs_debug_i8r_bound(C.c_size_t(d), C.c_size_t(nq), cd.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cn), C.byref(cc),
                                         C.byref(ran))
    assert rc == 0, capi.lib().msvs_last_error()
    assert ran.value == 1, "the last list scan did not run over an i8r shadow"
    return cd, cn.value


@pytest.mark.gpu
@pytest.mark.parametrize("d", [128, 200, 768])
def test_int8_operand_map_with_exact_integer_data(d, opt):
    """Residuals that are integers with a largest |element| of exactly 127 quantise without error (s = 1, lo = 0): every key the
    scan and the sample launch compute (one probe: the query's own list) must then be the exact distance -- any mismatch between
    the A (query) and B (row) lane maps of the int8 MFMA moves elements against each other and shows.  Random integers: A and B
    are asymmetric; the sums stay below 2^24, so the f32 epilogue is exact too."""
    rng = np.random.default_rng(d)
    nlist, n, nq = 4, 4096, 40
    cents = rng.integers(-50, 50, (nlist, d)).astype(np.float32)
    lists = rng.integers(0, nlist, n)
    res = rng.integers(-20, 21, (n, d))
    res[np.arange(n), rng.integers(0, d, n)] = 127
    x = (cents[lists] + res).astype(np.float32)
    qres = rng.integers(-20, 21, (nq, d))
    qres[np.arange(nq), rng.integers(0, d, nq)] = -127
    q = (cents[rng.integers(0, nlist, nq)] + qres).astype(np.float32)
    opt("h16_form", "3")
    ix = build_ivf(x, nlist, centroids=cents)
    assert shadow_form(ix) == 3
    opt("ivf_pass", "2")
    opt("h16_nocut", "1")
    opt("cand_cap", "16384")
    ids, dis = ix.search(q, 10, "nprobe=1")
    keys, cnt = last_keys(nq, 8192)
    cent, off, vecs, _ = ix.export()
    assert np.array_equal(np.diff(off), np.bincount(lists, minlength=nlist)), "every row sits in its own centroid's list"
    v64, q64 = vecs.astype(np.float64), q.astype(np.float64)
    for qi in range(nq):
        assert 0 < cnt[qi] <= 8192
        kk = keys[qi, : cnt[qi]]
        pos = (kk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        diff = v64[pos] - q64[qi]
        assert np.array_equal(key_values(kk), (diff * diff).sum(1)), "query %d: an approximate key is not the exact distance" % qi
    oi, od, _ = oracle(ix, q, 1, 10)
    same(ids, dis, oi, od)


ADVERSARIAL = ["blobs", "one_huge_element", "residuals_near_zero", "queries_far_from_the_lists"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ADVERSARIAL)
@pytest.mark.parametrize("d", [768, 100, 200, 2432])
def test_i8r_error_bound_on_hardware(name, d, opt):
    """The kernels' OWN approximate keys (every probed row of every list: h16_nocut, no pruning) against f64 exact distances:
    approx - eps <= exact with eps = 2 c_dot(q) |x||q| + c_norm (|x|^2 + |q|^2), c_dot(q) the per-query bound of
    set_error_model_i8r -- the lower bound every consumer of the keys relies on (the keys of a query's farther lists are lowered
    on purpose, so the band is one-sided there).  d = 100, 200: not multiples of 64 / 128 (zero padding of the last chunk);
    d = 2432: 19 chunks, the largest dimension whose query tile the list scan holds in LDS (1024 rows there: the f64 reference
    stays in seconds)."""
    rng = np.random.default_rng(ADVERSARIAL.index(name) * 1000 + d)
    nlist, n, nq = 8, (4096 if d <= 1024 else 1024), 64
    x, q = blobs(rng, nlist, n, nq, d)
    if name == "one_huge_element":
        hit = rng.random(n) < 0.1
        x[hit, rng.integers(0, d, hit.sum())] += 40.0  # s_x large: the rest of those rows quantises coarsely
    elif name == "residuals_near_zero":
        x, q = blobs(rng, nlist, n, nq, d, sigma=1e-5)
    elif name == "queries_far_from_the_lists":
        q = (q * 3.0 + rng.standard_normal((nq, d)).astype(np.float32)).astype(np.float32)
    opt("h16_form", "3")
    ix = build_ivf(x, nlist)
    assert shadow_form(ix) == 3
    opt("ivf_pass", "2")
    opt("h16_nocut", "1")
    opt("h16_preprune", "0")  # every pair scanned: the far lists too
    opt("h16_prune", "0")
    opt("cand_cap", "16384")
    ids, dis = ix.search(q, 10, "nprobe=%d" % nlist)
    cd, cn = i8r_bound(d, nq)  # (before the keys: reading them retires the record of the pass)
    assert np.isfinite(cd).all(), "every query inside the model's range"
    keys, cnt = last_keys(nq, 8192)
    assert (cnt == n).all()
    _, _, vecs, _ = ix.export()
    v64, q64 = vecs.astype(np.float64), q.astype(np.float64)
    xn = np.sqrt((v64 * v64).sum(1))
    worst = 0.0
    for qi in range(nq):
        kk = keys[qi, :n]
        pos = (kk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        diff = v64[pos] - q64[qi]
        exact = (diff * diff).sum(1)
        qn = np.sqrt((q64[qi] * q64[qi]).sum())
        eps = 2 * cd[qi] * xn[pos] * qn + cn * (xn[pos] ** 2 + qn ** 2)
        worst = max(worst, float(((key_values(kk) - exact) / (eps + 1e-300)).max()))
    assert worst < 1.0, "approximate keys leave the certified band: max (approx - exact) / eps = %.3f" % worst
    oi, od, _ = oracle(ix, q, nlist, 10)
    same(ids, dis, oi, od)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["3", "2"])
@pytest.mark.parametrize("nq,k", [(5, 10), (300, 1), (2100, 40), (700, 128)])
def test_forced_forms_match_oracle(form, nq, k, opt):
    """Both forms give the canonical answer bit for bit: small and large batches, k up to 128, a filter, a delete bitmap, rows added
    in two batches before the build, and serialise -> load (the shadow is derived data: rebuilt at load, in the form the knob asks
    for)."""
    rng = np.random.default_rng(nq + k)
    d, nlist, n, nprobe = 192, 32, 30000, 6
    x, q = blobs(rng, 48, n, nq, d)
    opt("h16_form", form)
    ix = build_ivf(x, nlist)
    assert shadow_form(ix) == int(form)
    opt("ivf_pass", "2")
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
    oi, od, _ = oracle(ix, q, nprobe, k)
    same(ids, dis, oi, od)
    alive = rng.random(n) < 0.6
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe, alive=alive)
    oa, oda, _ = oracle(ix, q, nprobe, k, alive=alive)
    same(ids, dis, oa, oda)
    dead = rng.random(n) < 0.3
    ix.set_delete_bitmap(~dead)
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
    od_i, od_d, _ = oracle(ix, q, nprobe, k, alive=~dead)
    same(ids, dis, od_i, od_d)
    ix.set_delete_bitmap(np.ones(n, bool))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ix")
        ix.serialize(path)
        ix2 = capi.Index.load(path, capi.INDEX_IVFFLAT, capi.METRIC_L2, d)
        assert shadow_form(ix2) == int(form)
        ids, dis = ix2.search(q, k, "nprobe=%d" % nprobe)
        same(ids, dis, oi, od)
        ix2.close()


@pytest.mark.gpu
def test_auto_rule_picks_i8r_on_blobs_and_fp16_on_iid(opt):
    """shadow = 1 (auto): clustered rows (sigma-0.3 blobs, one per list: the blob centres are the centroids) take the int8 residual
    form, iid rows keep fp16; IP keeps fp16 whatever the data; shadow = 2 / 3 force the form."""
    rng = np.random.default_rng(7)
    d, nlist, n = 768, 16, 16384
    cents = rng.standard_normal((nlist, d), dtype=np.float32)
    x = (cents[rng.integers(0, nlist, n)] + 0.3 * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    assert shadow_form(build_ivf(x, nlist, centroids=cents)) == 3
    assert shadow_form(build_ivf(x, nlist, ",shadow=2", centroids=cents)) == 2
    iid = rng.standard_normal((n, d), dtype=np.float32)
    assert shadow_form(build_ivf(iid, nlist)) == 2
    assert shadow_form(build_ivf(iid, nlist, ",shadow=3")) == 3
    assert shadow_form(build_ivf(iid, nlist, ",shadow=0")) == 0
    ip = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_IP, d, "ncentroids=%d,kmeans_iters=5,shadow=3" % nlist)
    ip.train(x)
    ip.add(x)
    ip.build()
    assert shadow_form(ip) == 2
