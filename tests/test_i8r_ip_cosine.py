"""The int8 residual list shadow ("i8r") under inner product and cosine: <q, x> = <q, c_l> + <q, x - c_l> with ONE hi / lo int8
image per query (h8_ip_prep_kernel), one constant per (query, list) pair, and the error model of set_error_model_i8r's second
half.  Build parameter / option values 4 (i8r whatever the metric) and 5 (auto over every metric) select it."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu
OM = {capi.METRIC_L2: o.METRIC_L2, capi.METRIC_IP: o.METRIC_IP, capi.METRIC_COSINE: o.METRIC_COSINE}
METRICS = {"ip": capi.METRIC_IP, "cosine": capi.METRIC_COSINE}


def same(a_ids, a_dis, b_ids, b_dis):
    assert np.array_equal(a_ids, b_ids), "ids differ"
    assert np.array_equal(a_dis.view(np.uint32), b_dis.view(np.uint32)), "distances differ"


def shadow_form(ix):
    capi.lib().msvs_debug_shadow_form.restype = C.c_int
    return capi.lib().msvs_debug_shadow_form(ix._h)


def build_ivf(x, metric, nlist, params="", centroids=None):
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, x.shape[1], "ncentroids=%d,kmeans_iters=5%s" % (nlist, params))
    if centroids is not None:
        ix.set_centroids(centroids)
    else:
        ix.train(x)
    half = x.shape[0] // 2
    ix.add(x[:half])
    ix.add(x[half:])
    ix.build()
    return ix


def oracle(ix, q, nprobe, k, metric, alive=None):
    cent, off, vecs, lids = ix.export()
    if metric == capi.METRIC_COSINE:
        oi, od, _ = o.ivf_search(cent, off, vecs, lids, o.normalize_rows(q), nprobe, k, o.METRIC_IP, alive=alive)
        return oi, (np.float32(1) - od).astype(np.float32)
    oi, od, _ = o.ivf_search(cent, off, vecs, lids, q, nprobe, k, OM[metric], alive=alive)
    return oi, od


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


def ip_key_values(kk):
    """The inner product behind a key of the IP ordered word (~f2ord(v) in the high half)."""
    o_ = ~(kk >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o_ & np.uint32(0x80000000), o_ & np.uint32(0x7FFFFFFF), ~o_).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def i8r_bound(d, nq):
    cd = np.zeros(nq, np.float64)
    cn, cc, ran = C.c_double(), C.c_double(), C.c_int()
    rc = capi.lib().msvs_debug_i8r_bound(C.c_size_t(d), C.c_size_t(nq), cd.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cn), C.byref(cc),
                                         C.byref(ran))
    assert rc == 0, capi.lib().msvs_last_error()
    assert ran.value == 1, "the last list scan did not run over an i8r shadow"
    return cd, cn.value, cc.value


def i8r_limit(d):
    return float(np.sqrt((d + 8.0) / 6.0))


def list_alpha_beta(cent, off, vecs):
    """alpha_l = max E_x / |x| and beta_l = max (|r_x| + E_x) / |x| of every list, as h8_build_kernel defines them (f64)."""
    nlist = len(off) - 1
    al, be = np.zeros(nlist), np.zeros(nlist)
    for l in range(nlist):
        x = vecs[off[l]:off[l + 1]].astype(np.float64)
        if not len(x):
            continue
        r = x - cent[l].astype(np.float64)
        s = np.abs(r).max(1, keepdims=True) / 127.0
        s = s.astype(np.float32).astype(np.float64)
        iq = np.clip(np.rint(np.divide(r, s, out=np.zeros_like(r), where=s > 0)), -127, 127)
        ex = np.sqrt(((r - s * iq) ** 2).sum(1))
        nx, nr = np.sqrt((x * x).sum(1)), np.sqrt((r * r).sum(1))
        al[l], be[l] = (ex / nx).max(), ((nr + ex) / nx).max()
    return al, be


def c16_of(vecs, d):
    """The fp16 form's coefficient the auto rule compares with: 2 rho16 + 1.01 d' 2^-23, rho16 = max |fp16(x s) / s - x| / |x|."""
    m = float(np.abs(vecs).max())
    s = 2.0 ** (14 - np.frexp(m)[1])
    v = vecs.astype(np.float64)
    back = (vecs * np.float32(s)).astype(np.float16).astype(np.float64) / s
    rho = (np.sqrt(((back - v) ** 2).sum(1)) / np.sqrt((v * v).sum(1))).max()
    return 2.0 * rho + 1.01 * (-(-d // 64) * 64) * 2.0 ** -23


@pytest.mark.parametrize("d", [128, 200, 768])
def test_ip_operand_map_with_exact_integer_data(d, opt):
    """Integer centroids, residuals and queries with a largest |element| of exactly 127 quantise without error (s_q = s_x = 1,
    lo = 0) and every sum stays below 2^24: every key of the scan and the sample launch must be the exact inner product.  A tile
    load indexed by pair instead of by query, or a slip in the A / B lane maps, moves elements against each other and shows."""
    rng = np.random.default_rng(d)
    nlist, n, nq = 4, 4096, 40
    cents = rng.integers(-50, 50, (nlist, d)).astype(np.float32)
    lists = rng.integers(0, nlist, n)
    res = rng.integers(-20, 21, (n, d))
    res[np.arange(n), rng.integers(0, d, n)] = 127
    x = (cents[lists] + res).astype(np.float32)
    q = rng.integers(-60, 61, (nq, d))
    q[np.arange(nq), rng.integers(0, d, nq)] = -127
    q = q.astype(np.float32)
    opt("h16_form", "4")
    ix = build_ivf(x, capi.METRIC_IP, nlist, centroids=cents)
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
        assert np.array_equal(ip_key_values(kk), v64[pos] @ q64[qi]), "query %d: an approximate key is not the exact product" % qi
    oi, od = oracle(ix, q, 1, 10, capi.METRIC_IP)
    same(ids, dis, oi, od)


ADVERSARIAL = ["blobs", "one_huge_element", "residuals_near_zero", "queries_with_one_huge_element"]


@pytest.mark.parametrize("name", ADVERSARIAL)
@pytest.mark.parametrize("d", [768, 100, 200, 2432])  # 2432: the largest d whose query tile the list scan holds in LDS (1024 rows there)
@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_i8r_ip_error_bound_on_hardware(metric, name, d, opt):
    """The kernels' own keys (every row of every list: no cut, no pruning) against f64 products: exact <= approx + eps with eps the
    re-rank's inner-product form (c_dot(q) + c_canon) |x||q|, c_dot(q) the per-query coefficient of set_error_model_i8r -- the
    one-sided bound the certificate uses (the keys of a query's other lists are raised on purpose) -- and with c_dot(q) |x||q|
    alone, which puts the model's rounding constants to the test."""
    m = METRICS[metric]
    rng = np.random.default_rng(ADVERSARIAL.index(name) * 1000 + d)
    nlist, n, nq = 8, (4096 if d <= 1024 else 1024), 64
    x, q = blobs(rng, nlist, n, nq, d)
    if name == "one_huge_element":
        hit = rng.random(n) < 0.1
        x[hit, rng.integers(0, d, hit.sum())] += 40.0
    elif name == "residuals_near_zero":
        x, q = blobs(rng, nlist, n, nq, d, sigma=1e-5)
    elif name == "queries_with_one_huge_element":
        q[np.arange(nq), rng.integers(0, d, nq)] += 40.0  # s_q large: the rest of the query lives in the lo image
    opt("h16_form", "4")
    ix = build_ivf(x, m, nlist)
    assert shadow_form(ix) == 3
    cent, off, vecs, _ = ix.export()
    al, be = list_alpha_beta(cent, off, vecs)
    print("alpha_l max %.3e  beta_l max %.3f  limit %.3f" % (al.max(), be.max(), i8r_limit(d)))
    assert be.max() < i8r_limit(d), "the inputs stay inside the model's range"
    opt("ivf_pass", "2")
    opt("h16_nocut", "1")
    opt("h16_preprune", "0")
    opt("h16_prune", "0")
    opt("cand_cap", "16384")
    ids, dis = ix.search(q, 10, "nprobe=%d" % nlist)
    cd, _, cc = i8r_bound(d, nq)  # (before the keys: reading them retires the record of the pass)
    assert np.isfinite(cd).all(), "every query inside the model's range"
    keys, cnt = last_keys(nq, 8192)
    assert (cnt == n).all()
    qs = o.normalize_rows(q) if m == capi.METRIC_COSINE else q
    v64, q64 = vecs.astype(np.float64), qs.astype(np.float64)
    xn = np.sqrt((v64 * v64).sum(1))
    worst = own = 0.0
    for qi in range(nq):
        kk = keys[qi, :n]
        pos = (kk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        gap = v64[pos] @ q64[qi] - ip_key_values(kk)
        xq = xn[pos] * np.sqrt((q64[qi] * q64[qi]).sum())
        worst = max(worst, float((gap / ((cd[qi] + cc) * xq + 1e-30)).max()))
        own = max(own, float((gap / (cd[qi] * xq + 1e-300)).max()))
    print("max (exact - approx) / eps = %.4f, without c_canon %.4f   c_dot(q) %.3e .. %.3e" % (worst, own, cd.min(), cd.max()))
    assert worst < 1.0, "a product exceeds its key by more than the certified eps: max (exact - approx) / eps = %.3f" % worst
    # the keys are compared with f64 products, not with canonical f32 values: the model's own coefficient must cover the gap without
    # c_canon -- with residuals near zero the rounding terms u (4.1 + 2.02 beta_l) + 3.1 u beta_l h are the whole bound
    assert own < 1.0, "the model's own terms do not cover the keys: max (exact - approx) / (c_dot |x||q|) = %.3f" % own
    oi, od = oracle(ix, q, nlist, 10, m)
    same(ids, dis, oi, od)


@pytest.mark.parametrize("form", ["4", "2"])
@pytest.mark.parametrize("nq,k", [(5, 10), (300, 1), (2100, 40), (700, 128)])
@pytest.mark.parametrize("metric", ["ip", "cosine"])
def test_forced_forms_match_oracle_ip_cosine(metric, form, nq, k, opt):
    """Both forms give the canonical answer bit for bit: small and large batches, k up to 128, a filter, a delete bitmap, rows added
    in two batches, serialise -> load; (300, 1) also carries a zero query and an empty list."""
    m = METRICS[metric]
    rng = np.random.default_rng(nq + k)
    d, nlist, n, nprobe = 192, 32, 30000, 6
    x, q = blobs(rng, 48, n, nq, d)
    opt("h16_form", form)
    want = 3 if form == "4" else 2
    if (nq, k) == (300, 1):
        q[7] = 0.0
        # user-supplied centroids, one of them where no row goes (the zero vector: some other product is positive)
        cents = x[rng.choice(n, nlist, replace=False)].copy()
        cents[5] = 0.0
        ix = build_ivf(x, m, nlist, centroids=cents)
        assert (np.diff(ix.export(with_vecs=False)[1]) == 0).any(), "one list is empty"
    else:
        ix = build_ivf(x, m, nlist)
    assert shadow_form(ix) == want
    opt("ivf_pass", "2")
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
    oi, od = oracle(ix, q, nprobe, k, m)
    same(ids, dis, oi, od)
    alive = rng.random(n) < 0.6
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe, alive=alive)
    same(ids, dis, *oracle(ix, q, nprobe, k, m, alive=alive))
    dead = rng.random(n) < 0.3
    ix.set_delete_bitmap(~dead)
    ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
    same(ids, dis, *oracle(ix, q, nprobe, k, m, alive=~dead))
    ix.set_delete_bitmap(np.ones(n, bool))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ix")
        ix.serialize(path)
        ix2 = capi.Index.load(path, capi.INDEX_IVFFLAT, m, d)
        assert shadow_form(ix2) == want
        ids, dis = ix2.search(q, k, "nprobe=%d" % nprobe)
        same(ids, dis, oi, od)
        ix2.close()


def auto_rule_side(ix, d, margin=2.0):
    """Which form shadow = 5 must give an inner-product / cosine index by the rule -- every beta_l in range and >= 97 % of the rows
    in lists with alpha_l <= 3 c16 -- computed here in numpy from the exported structure; the inputs must sit at least `margin`
    away from the threshold on their side."""
    cent, off, vecs, _ = ix.export()
    al, be = list_alpha_beta(cent, off, vecs)
    c16 = c16_of(vecs, d)
    rows = np.diff(off).astype(np.float64)
    frac = lambda thr: rows[al <= thr].sum() / rows.sum()
    print("alpha_l %.3e .. %.3e  3 c16 %.3e  beta_l max %.3f" % (al.min(), al.max(), 3 * c16, be.max()))
    if be.max() * margin <= i8r_limit(d) and frac(3 * c16 / margin) >= 0.97:
        return 3
    if be.max() > i8r_limit(d) * margin or frac(3 * c16 * margin) < 0.97:
        return 2
    raise AssertionError("the inputs sit within %.1fx of the auto rule's threshold" % margin)


def test_forms_and_auto_rule_over_every_metric(opt):
    """shadow = 4 forces i8r whatever the metric, 3 still leaves an inner-product index fp16, 5 applies the auto rule to every metric
    (inner product, cosine: alpha_l against 3 c16).  Centroids = the blob centres (cosine: on the sphere, where its rows are)."""
    rng = np.random.default_rng(7)
    d, nlist, n = 768, 16, 16384
    cents = rng.standard_normal((nlist, d), dtype=np.float32)
    which = rng.integers(0, nlist, n)
    tight = (cents[which] + 0.05 * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    unit = o.normalize_rows(cents)
    IP, COS, L2 = capi.METRIC_IP, capi.METRIC_COSINE, capi.METRIC_L2
    assert shadow_form(build_ivf(tight, IP, nlist, ",shadow=4", centroids=cents)) == 3
    assert shadow_form(build_ivf(tight, COS, nlist, ",shadow=4", centroids=unit)) == 3
    assert shadow_form(build_ivf(tight, L2, nlist, ",shadow=4", centroids=cents)) == 3
    ix = build_ivf(tight, IP, nlist, ",shadow=3", centroids=cents)
    assert shadow_form(ix) == 2
    assert auto_rule_side(ix, d) == 3, "sigma-0.05 blobs: well inside the rule under inner product"
    assert shadow_form(build_ivf(tight, IP, nlist, ",shadow=5", centroids=cents)) == 3
    iid = rng.standard_normal((n, d), dtype=np.float32)
    for m in (IP, COS):
        ix = build_ivf(iid, m, nlist, ",shadow=2")
        assert auto_rule_side(ix, d) == 2, "iid rows: residuals as long as the rows"
        assert shadow_form(build_ivf(iid, m, nlist, ",shadow=5")) == 2
    ix = build_ivf(tight, COS, nlist, ",shadow=2", centroids=unit)
    side = auto_rule_side(ix, d)
    assert side == 3, "sigma-0.05 blobs on the sphere: alpha_l ~ 4e-4 against 3 c16 ~ 1.5e-3"
    assert shadow_form(build_ivf(tight, COS, nlist, ",shadow=5", centroids=unit)) == side
    opt("h16_form", "5")  # the option names the same values
    assert shadow_form(build_ivf(tight, IP, nlist, centroids=cents)) == 3
    assert shadow_form(build_ivf(iid, IP, nlist)) == 2
