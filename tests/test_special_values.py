"""Non-finite, overflowing and subnormal queries and rows through every search path, against the CPU oracle bit for bit.

The batched paths step aside when a value makes their error model meaningless (the `bad` mark of the fp16 query images, qnorm = +inf
as "never certify", the |q|^2 and xmax < 1e30 gates of the re-rank and band kernels, qbound = +inf of the i8r pair images, xnorm_max
of the index).  The inputs here enter those branches: sixteen kinds of special query mixed into a batch of ordinary ones, and the
same kinds as stored rows.  Every distance comparison is on the uint32 view."""
import ctypes as C
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_pq_ivf as pq
import test_sq_ivf as sq
from oracle import oracle as o

gpu = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
OM = {L2: o.METRIC_L2, IP: o.METRIC_IP, COS: o.METRIC_COSINE}
NAME = {L2: "l2", IP: "ip", COS: "cosine"}
METRICS = [pytest.param(m, id=NAME[m]) for m in (L2, IP, COS)]
FLT_MAX, FLT_MIN = np.finfo(F).max, np.finfo(F).tiny
K, NPROBE = 10, 4


def same(a_ids, a_dis, b_ids, b_dis, what=""):
    au, bu = np.ascontiguousarray(a_dis).view(np.uint32), np.ascontiguousarray(b_dis).view(np.uint32)
    bad = np.flatnonzero((a_ids != b_ids).any(axis=1) | (au != bu).any(axis=1))
    if len(bad):
        r = int(bad[0])
        raise AssertionError("%s queries %s differ from the reference; query %d: got %s %s, reference %s %s"
                             % (what, bad.tolist(), r, a_ids[r].tolist(), a_dis[r].tolist(), b_ids[r].tolist(), b_dis[r].tolist()))


def build_ivf(x, metric, nlist, params="", centroids=None, chunks=None):
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, x.shape[1], "ncentroids=%d,kmeans_iters=5%s" % (nlist, params))
    if centroids is not None:
        ix.set_centroids(centroids)
    else:
        ix.train(x)
    for a, b in chunks or ((0, x.shape[0] // 2), (x.shape[0] // 2, x.shape[0])):
        ix.add(x[a:b])
    ix.build()
    return ix


def oracle_on_structure(cent, off, vecs, lids, q, nprobe, k, metric, alive=None):
    if metric == COS:
        oi, od, pr = o.ivf_search(cent, off, vecs, lids, o.normalize_rows(q), nprobe, k, o.METRIC_IP, alive=alive)
        return oi, (F(1) - od).astype(F), pr
    return o.ivf_search(cent, off, vecs, lids, q, nprobe, k, OM[metric], alive=alive)


def oracle_on_exported(ix, q, nprobe, k, metric, alive=None):
    return oracle_on_structure(*ix.export(), q, nprobe, k, metric, alive=alive)


def oracle_flat(q, x, k, metric, labels=None):
    """A FLAT index / a resident block: cosine stores normalised rows and reports 1 - ip in every slot."""
    if metric == COS:
        oi, od = o.knn(o.normalize_rows(q), o.normalize_rows(x), k, o.METRIC_IP, labels=labels)
        return oi, (F(1) - od).astype(F)
    return o.knn(q, x, k, OM[metric], labels=labels)


def device_search(ix, q, k, nprobe, alive=None):
    """msvs_*_search_device with the queries in a torch tensor"""
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).cuda()
    di = torch.empty((len(q), k), device="cuda", dtype=torch.int64)
    dd = torch.empty((len(q), k), device="cuda", dtype=torch.float32)
    bits, nbits = 0, 0
    if alive is not None:
        db = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).cuda()
        bits, nbits = db.data_ptr(), len(alive)
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream, d_alive=bits,
                     nbits=nbits)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


def blobs(rng, nblob, n, nq, d, sigma=0.3):
    c = rng.standard_normal((nblob, d), dtype=F)
    x = (c[rng.integers(0, nblob, n)] + sigma * rng.standard_normal((n, d), dtype=F)).astype(F)
    q = (c[rng.integers(0, nblob, nq)] + sigma * rng.standard_normal((nq, d), dtype=F)).astype(F)
    return x, q


# ---------------------------------------------------------------------------------------- 0. the inputs

QUERY_KINDS = ("nan_one", "nan_all", "pos_inf", "neg_inf", "flt_max", "e3e19", "e1e19", "e2e15", "e1e5", "x7e4", "pos_zero", "neg_zero",
               "x1e-41", "x1e-30", "x1e-20", "flt_min")
MODERATE_ROWS = ("pos_zero", "neg_zero", "x1e-41", "x1e-20", "e1e5", "x7e4")
EXTREME_ROWS = MODERATE_ROWS + ("nan_one", "nan_all", "pos_inf", "neg_inf", "flt_max_row", "e3e19", "e1e19", "e2e15")
ELEMENT = {"nan_one": np.nan, "pos_inf": np.inf, "neg_inf": -np.inf, "flt_max": FLT_MAX, "e3e19": 3e19, "e1e19": 1e19, "e2e15": 2e15,
           "e1e5": 1e5}
SCALE = {"x7e4": 7e4, "x1e-41": 1e-41, "x1e-30": 1e-30, "x1e-20": 1e-20}
WHOLE = {"nan_all": np.nan, "pos_zero": 0.0, "neg_zero": -0.0, "flt_max_row": FLT_MAX}


def positions(d):
    """column 0, a column inside the first 64-column block, column 64 and the last column (the tail block at d = 100)"""
    return (0, 37, 64, d - 1)


def put(v, kind, j):
    """Overwrite the ordinary vector v in place with its special form `kind`; a kind that changes one element changes element j."""
    if kind in ELEMENT:
        v[j] = F(ELEMENT[kind])
    elif kind in SCALE:
        v *= F(SCALE[kind])
    elif kind in WHOLE:
        v[:] = F(WHOLE[kind])
    elif kind == "flt_min":
        v[j], v[(j + 1) % len(v)] = FLT_MIN, -FLT_MIN
    else:
        raise KeyError(kind)


def is_kind(v, kind):
    """Does v still carry what makes `kind` special?  (The CPU test holds every input to this.)"""
    a = np.abs(v)
    if kind == "nan_one":
        return np.isnan(v).sum() == 1
    if kind == "nan_all":
        return np.isnan(v).all()
    if kind in ("pos_inf", "neg_inf"):
        return (v == F(ELEMENT[kind])).sum() == 1 and np.isinf(v).sum() == 1
    if kind == "flt_max_row":
        return (v == FLT_MAX).all()
    if kind in ELEMENT:
        return (v == F(ELEMENT[kind])).sum() == 1 and np.sort(a)[-2] < 10
    if kind == "pos_zero":
        return (v.view(np.uint32) == 0).all()
    if kind == "neg_zero":
        return (v.view(np.uint32) == 0x80000000).all()
    if kind == "x1e-41":
        return (a < FLT_MIN).all() and (a > 0).sum() > len(v) // 2
    if kind in SCALE:
        s = SCALE[kind]
        return s * 1e-3 < np.median(a) < s * 10 and a.max() < s * 10
    if kind == "flt_min":
        return (v == FLT_MIN).sum() == 1 and (v == -FLT_MIN).sum() == 1
    raise KeyError(kind)


def special_queries(q):
    """-> (a copy of the batch q with rows 1 ... 16 overwritten by the sixteen kinds, {kind: row}).  Rows 0 and >= 17 stay ordinary."""
    q = np.array(q, F)
    pos = positions(q.shape[1])
    where = {}
    for i, kind in enumerate(QUERY_KINDS):
        put(q[1 + i], kind, pos[i % 4])
        where[kind] = 1 + i
    return q, where


def ordinary_rows(nq):
    return np.array([0] + list(range(1 + len(QUERY_KINDS), nq)))


# The class of the oracle's answer per kind and metric (L2, IP, cosine) -- from the arithmetic, not from a run:
#   empty       no slot filled: every distance is inf or NaN, or the coarse quantiser admits no centroid
#   full        k rows, finite distances
#   inf         k rows, every score +inf (IP; ties by id)
#   equal       k rows, one distance bit pattern, ids ascending
#   level       k rows, one distance bit pattern, ids in another order (cosine: the order of the products, which fl(1 - ip) hides)
#   subnormal   k rows, every score a non-zero f32 subnormal
# NaN anywhere: every product sum is NaN.  +-inf: (inf - x)^2 = inf under L2; inf * x = +-inf under IP (x = 0: NaN, skipped); the
# sum of squares is inf and inf / inf = NaN under cosine.  FLT_MAX: its square and FLT_MAX * x for |x| > 1 overflow; under cosine the
# sum of squares overflows and x / inf = 0 makes a zero query, whose products are all +0: 1 - 0 in every slot.  3e19: 9e38 = inf
# under L2, finite products under IP, and under cosine the sum of squares overflows as for FLT_MAX.  1e19: fl(1e19 - x) = 1e19
# for every |x| < 2^39, so every L2 distance is fl(1e38); 2e15 likewise (its ulp is 2^27, and 4e30 absorbs the other columns' sum).
# Zero queries: every product is +-0 and +0 + -0 = +0.  x 1e-41 .. x 1e-20
# under cosine: the sum of squares is below FLT_EPSILON, the query stays as it is, and fl(1 - ip) = 1 in every slot, best product first.
EXPECT = {
    "nan_one": ("empty", "empty", "empty"), "nan_all": ("empty", "empty", "empty"),
    "pos_inf": ("empty", "inf", "empty"), "neg_inf": ("empty", "inf", "empty"),
    "flt_max": ("empty", "inf", "equal"), "e3e19": ("empty", "full", "equal"),
    "e1e19": ("equal", "full", "full"), "e2e15": ("equal", "full", "full"), "e1e5": ("full", "full", "full"), "x7e4": ("full", "full", "full"),
    "pos_zero": ("full", "equal", "equal"), "neg_zero": ("full", "equal", "equal"),
    "x1e-41": ("full", "subnormal", "level"), "x1e-30": ("full", "full", "level"), "x1e-20": ("full", "full", "level"),
    "flt_min": ("full", "full", "full"),
}


def outcome_class(ids, dis, metric):
    neutral = -FLT_MAX if metric == IP else FLT_MAX  # (cosine: fl(1 - -FLT_MAX) = FLT_MAX)
    if (ids == -1).all():
        assert (dis == neutral).all()
        return "empty"
    assert (ids >= 0).all() and len(set(ids.tolist())) == len(ids), "neither empty nor full: %s" % ids
    if (dis == np.inf).all():
        return "inf"
    assert np.isfinite(dis).all()
    if (dis.view(np.uint32) == dis.view(np.uint32)[0]).all():
        return "equal" if (np.diff(ids) > 0).all() else "level"
    if (np.abs(dis) < FLT_MIN).all() and (dis != 0).all():
        return "subnormal"
    return "full"


@pytest.mark.parametrize("metric", METRICS)
def test_reference_outcome_classes(metric):
    """What the CPU oracle answers for every kind of special query, by class; every ordinary query is full.  Keeps the GPU tests from
    passing vacuously: a kind dropped from special_queries, or one whose value no longer does what its name says, fails here."""
    rng = np.random.default_rng(5)
    n, d, nlist, nq = 4096, 100, 16, 64
    x, q0 = blobs(rng, nlist, n, nq, d)
    q, where = special_queries(q0)
    assert list(where) == list(EXPECT) == list(QUERY_KINDS) and sorted(where.values()) == list(range(1, 17))
    used = set()
    for kind, row in where.items():
        assert is_kind(q[row], kind), kind
        used |= set(np.flatnonzero(q[row].view(np.uint32) != q0[row].view(np.uint32)).tolist()) if kind in ELEMENT else set()
    assert used == set(positions(d)), "the element kinds cover column 0, the first block, column 64 and the tail"
    ordinary = ordinary_rows(nq)
    assert np.array_equal(q[ordinary].view(np.uint32), q0[ordinary].view(np.uint32))
    xs = o.normalize_rows(x) if metric == COS else x
    cent = o.kmeans(xs, nlist, 5)
    off, vecs, lids = o.build_ivf(xs, np.arange(n, dtype=np.int64), cent)
    ids, dis, _ = oracle_on_structure(cent, off, vecs, lids, q, NPROBE, K, metric)
    col = (L2, IP, COS).index(metric)
    got = {kind: outcome_class(ids[row], dis[row], metric) for kind, row in where.items()}
    assert got == {kind: EXPECT[kind][col] for kind in QUERY_KINDS}
    for row in ordinary:
        assert outcome_class(ids[row], dis[row], metric) == "full", "ordinary query %d" % row


# ---------------------------------------------------------------------------------------- 1. special queries mixed into a batch

FORMS = {"default": "", "fp16": ",shadow=2", "i8r": None, "none": ",shadow=0"}  # i8r: 3 for L2, 4 for inner product and cosine
SETTINGS = {"plain": {}, "split_bf16": {"ivf_h16": "0"}, "grouped_scan": {"ivf_pass": "0"}, "all_fallback": {"ivf_eps_scale": "1e12"},
            "cand_cap_64": {"cand_cap": "64"}}


SHADOW_FORM = {"fp16": 2, "i8r": 3}  # msvs_debug_shadow_form of a forced form


def shadow_form(ix):
    capi.lib().msvs_debug_shadow_form.restype = C.c_int
    return capi.lib().msvs_debug_shadow_form(ix._h)


def form_params(form, metric):
    return (",shadow=3" if metric == L2 else ",shadow=4") if form == "i8r" else FORMS[form]


@functools.lru_cache(maxsize=None)
def mixed_data(d):
    """4096 blob rows and two batches of 128 queries: `mixed` carries the sixteen kinds in rows 1 ... 16, `clean` ordinary queries
    there (the other rows are the same)."""
    rng = np.random.default_rng(1000 + d)
    x, clean = blobs(rng, 8, 4096, 128, d)
    mixed, where = special_queries(clean)
    alive = rng.random(len(x)) < 0.5
    return x, mixed, clean, where, alive


@functools.lru_cache(maxsize=None)
def mixed_case(metric, d, form):
    """One index per (metric, d, shadow form) and the oracle's answers over its exported structure, shared by every setting."""
    x, mixed, clean, _, _ = mixed_data(d)
    ix = build_ivf(x, metric, 8, form_params(form, metric))
    assert form not in SHADOW_FORM or shadow_form(ix) == SHADOW_FORM[form], "the build did not give the %s shadow" % form
    exp = ix.export()
    om =oracle_on_structure(*exp, mixed, NPROBE, K, metric)[:2]
    oc = oracle_on_structure(*exp, clean, NPROBE, K, metric)[:2]
    return ix, exp, om, oc


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_mixed_into_a_batch(metric, d, form, setting, opt, request):
    """The mixed batch equals the oracle bit for bit, and so does the clean one; the ordinary queries of the mixed batch get what they
    get in the clean batch (one query must not poison its neighbours).  The fallback counts of both are recorded, not bounded."""
    ix, _, om, oc = mixed_case(metric, d, form)
    _, mixed, clean, _, _ = mixed_data(d)
    for name, value in SETTINGS[setting].items():
        opt(name, value)
    p0 = capi.prefilter_stats()
    mi, md = ix.search(mixed, K, "nprobe=%d" % NPROBE)
    p1 = capi.prefilter_stats()
    ci, cd = ix.search(clean, K, "nprobe=%d" % NPROBE)
    p2 = capi.prefilter_stats()
    fb = "fallbacks: mixed batch %d, clean batch %d" % (p1[1] - p0[1], p2[1] - p1[1])
    print(request.node.name, fb)  # (recorded: nobody has measured a bound on their difference)
    ordinary = ordinary_rows(len(mixed))
    same(mi[ordinary], md[ordinary], ci[ordinary], cd[ordinary], "ordinary queries, mixed against clean batch (%s):" % fb)
    same(ci, cd, *oc, "clean batch (%s):" % fb)
    same(mi, md, *om, "mixed batch (%s):" % fb)
    if setting != "grouped_scan":
        assert p1[0] - p0[0] == len(mixed) and p2[0] - p1[0] == len(clean), "the candidate pass did not run for both batches (%s)" % fb
    else:
        assert p2[0] == p0[0], "ivf_pass = 0 is the canonical grouped scan"


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_through_the_device_entry(metric, d, form):
    """search_device normalises a cosine query on the device, the host-pointer entry on the CPU: the FLT_MAX, 3e19 and inf queries
    are where an overflowing sum of squares could part them."""
    ix, _, om, _ = mixed_case(metric, d, form)
    mixed = mixed_data(d)[1]
    same(*device_search(ix, mixed, K, NPROBE), *om, "device entry:")
    same(*ix.search(mixed, K, "nprobe=%d" % NPROBE), *om, "host entry:")


@gpu
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_with_a_filter(metric, d):
    ix, exp, _, _ = mixed_case(metric, d, "default")
    _, mixed, _, _, alive = mixed_data(d)
    oi, od, _ = oracle_on_structure(*exp, mixed, NPROBE, K, metric, alive=alive)
    same(*ix.search(mixed, K, "nprobe=%d" % NPROBE, alive=alive), oi, od, "host entry, filter:")
    same(*device_search(ix, mixed, K, NPROBE, alive=alive), oi, od, "device entry, filter:")


def few_query_groups(where):
    """Every special query alone, in pairs, and in groups of four = one ordinary and three special queries."""
    rows = sorted(where.values())
    groups = [[r] for r in rows] + [rows[i:i + 2] for i in range(0, len(rows), 2)]
    return groups + [[0] + (rows + rows)[i:i + 3] for i in range(0, len(rows), 3)]


@gpu
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_on_the_few_query_path(metric, d, opt):
    """latency_kernels.hpp (lat_path = 2) against the general path (lat_path = 0) and the oracle, both entries."""
    ix, _, om, _ = mixed_case(metric, d, "default")
    _, mixed, _, where, _ = mixed_data(d)
    groups = few_query_groups(where)
    assert {len(g) for g in groups} == {1, 2, 4} and all(g[0] == 0 and len(set(g)) == 4 for g in groups if len(g) == 4)
    for g in groups:
        for lp in ("2", "0"):
            opt("lat_path", lp)
            same(*ix.search(mixed[g], K, "nprobe=%d" % NPROBE), om[0][g], om[1][g], "lat_path %s, host entry, queries %s:" % (lp, g))
            same(*device_search(ix, mixed[g], K, NPROBE), om[0][g], om[1][g], "lat_path %s, device entry, queries %s:" % (lp, g))


@gpu
@pytest.mark.parametrize("nlist", [8, 64, 300])
def test_fewer_admitted_centroids_than_nprobe(nlist, opt):
    """An inner-product query with an infinite element scores +inf with the centroids whose element there has its sign, -inf (no
    entry) with the others: the coarse quantiser admits fewer centroids than nprobe.  Here the admitted ones are the LAST two of the
    table; the probe selection of small batches once filled the probe list with empty slots in lane order and dropped them."""
    rng = np.random.default_rng(nlist)
    n, d, nprobe = 4096, 100, 8
    cents = rng.standard_normal((nlist, d), dtype=F)
    j = positions(d)[1]
    cents[:, j] = -np.abs(cents[:, j]) - F(0.5)
    cents[-2:, j] = 1.0
    x = (cents[rng.integers(0, nlist, n)] + F(0.1) * rng.standard_normal((n, d), dtype=F)).astype(F)
    q = (cents[rng.integers(0, nlist, 40)] + F(0.1) * rng.standard_normal((40, d), dtype=F)).astype(F)
    q[::2, j] = np.inf
    q[1::4, j] = -np.inf
    ix = build_ivf(x, IP, nlist, centroids=cents)
    oi, od, probes = oracle_on_exported(ix, q, nprobe, K, IP)
    assert sorted(probes[0].tolist()) == [-1] * (nprobe - 2) + [nlist - 2, nlist - 1] and (oi[0] >= 0).all()
    assert (probes[1] >= 0).sum() == min(nprobe, nlist - 2)
    for lp in ("2", "0"):
        opt("lat_path", lp)
        for nq in (1, 4, 40):
            same(*ix.search(q[:nq], K, "nprobe=%d" % nprobe), oi[:nq], od[:nq], "lat_path %s, %d queries:" % (lp, nq))
    ix.close()


# ---------------------------------------------------------------------------------------- 2. special rows in the index

ROWS_N, ROWS_D, ROWS_NLIST, ROWS_K = 4096, 100, 8, 16
HOMES = (1, 4, 6, 3)  # the blobs the four copies of a kind are made from; copy t changes the element at positions(d)[t]


def special_rows(x, home, kinds):
    """-> (a copy of x with four rows per kind overwritten, made from rows of four different blobs, and the LAST row made `x7e4`;
    {row: kind})."""
    x = np.array(x, F)
    pos = positions(x.shape[1])
    kind_of = {}
    for i, kind in enumerate(kinds):
        for t, h in enumerate(HOMES):
            row = int(np.flatnonzero(home == h)[3 + 2 * i])
            put(x[row], kind, pos[t])
            kind_of[row] = kind
    put(x[-1], "x7e4", 0)
    kind_of[len(x) - 1] = "x7e4"
    return x, kind_of


@functools.lru_cache(maxsize=None)
def rows_data(level):
    """Hand-made centres (column positions(d)[t] has its largest value in list 2 t and its smallest in list 2 t + 1, so a row with
    one huge element there has a definite nearest centre), blob rows around them with the special rows of `level` among them, and the
    queries: 128 ordinary ones, the special rows themselves, an ordinary query with a positive / a negative element where the rows
    with +inf / -inf have theirs, and per list l one query -sum(centres) + centre_l / 2, whose products with everything it probes are
    negative, so that rows scoring zero come first."""
    rng = np.random.default_rng(77)
    n, d, nlist = ROWS_N, ROWS_D, ROWS_NLIST
    pos = positions(d)
    cents = (2 * rng.standard_normal((nlist, d), dtype=F)).astype(F)
    for t, j in enumerate(pos):
        cents[:, j] = np.clip(cents[:, j], -2.5, 2.5)
        cents[2 * t, j], cents[2 * t + 1, j] = 3.0, -3.0
    home = rng.integers(0, nlist, n)
    x0 = (cents[home] + F(0.3) * rng.standard_normal((n, d), dtype=F)).astype(F)
    x, kind_of = special_rows(x0, home, MODERATE_ROWS if level == "moderate" else EXTREME_ROWS)
    q = (cents[rng.integers(0, nlist, 128)] + F(0.3) * rng.standard_normal((128, d), dtype=F)).astype(F)
    on_rows = x[sorted(kind_of)]
    signed = np.repeat(q[:2], 4, axis=0)
    for t, j in enumerate(pos):
        signed[t, j], signed[4 + t, j] = 2.0, -2.0
    against = (-cents.sum(0)[None, :] + F(0.5) * cents).astype(F)
    return cents, x, kind_of, np.concatenate([q, on_rows, signed, against]).astype(F)


def rows_centroids(metric, cents):
    return o.normalize_rows(cents) if metric == COS else cents


# The kinds of row that some query must find (a row of the kind in its oracle top-k), per metric: the conditions of section 2 on the
# inputs.  L2: a query equal to the row is at distance 0, except where the coarse quantiser admits no centroid (3e19: every centroid
# distance is inf) and where the distance is NaN or inf.  Inner product: the huge rows score highest for their own copies, +-inf rows
# score +inf for a query with an element of their sign, the rows near zero score highest for the queries built against a list.  Cosine
# stores normalised rows: a 3e19 or FLT_MAX row overflows its sum of squares and is stored as a zero row, NaN and inf rows as NaN.
FOUND = {
    L2: {"pos_zero", "neg_zero", "x1e-41", "x1e-20", "e1e5", "x7e4", "e1e19", "e2e15"},
    IP: {"pos_zero", "neg_zero", "x1e-41", "x1e-20", "e1e5", "x7e4", "e1e19", "e2e15", "e3e19", "pos_inf", "neg_inf"},
    COS: {"pos_zero", "neg_zero", "x1e-41", "x1e-20", "e1e5", "x7e4", "e1e19", "e2e15", "e3e19", "flt_max_row"},
}


def check_row_inputs(exp, kind_of, probes, oi, metric, level):
    """Conditions on the inputs (CPU): every list holding a special row is probed, every kind that can be found is found, a kind spreads
    over lists where its value lets it, and a special row closes a list whose length no block size divides."""
    cent, off, vecs, lids = exp
    list_of = np.searchsorted(off, np.arange(len(lids)), side="right") - 1
    at = {int(l): i for i, l in enumerate(lids)}
    lists = {}
    for row, kind in kind_of.items():
        lists.setdefault(kind, set()).add(int(list_of[at[row]]))
    holding = set().union(*lists.values())
    assert holding <= set(probes[probes >= 0].tolist()), "a list with special rows is never probed: %s" % (holding,)
    found = {kind_of[int(i)] for i in oi[oi >= 0].tolist() if int(i) in kind_of}
    want = FOUND[metric] & set(kind_of.values())
    assert want <= found, "special rows no query finds: %s" % sorted(want - found)
    for kind in ("e1e5", "x7e4"):
        assert len(lists[kind]) >= 3, "%s rows sit in lists %s" % (kind, lists[kind])
    assert len(holding) >= 3
    last = at[len(lids) - 1]
    l = int(list_of[last])
    assert last == off[l + 1] - 1 and (off[l + 1] - off[l]) % 2 == 1, "the last row closes a list of odd length"


@functools.lru_cache(maxsize=None)
def rows_case(metric, level, form):
    cents, x, kind_of, q = rows_data(level)
    n = len(x)
    ix = build_ivf(x, metric, ROWS_NLIST, form_params(form, metric), centroids=rows_centroids(metric, cents))
    exp = ix.export()
    off = exp[1]
    l = int(np.searchsorted(off, np.flatnonzero(exp[3] == n - 1)[0], side="right") - 1)
    if (off[l + 1] - off[l]) % 2 == 0:  # the list the last row closes must have an odd length: leave its first ordinary row out
        drop = next(int(i) for i in exp[3][off[l]:off[l + 1]] if int(i) not in kind_of)
        ix.close()
        x = np.delete(x, drop, axis=0)
        kind_of = {r - (r > drop): kind for r, kind in kind_of.items()}
        ix = build_ivf(x, metric, ROWS_NLIST, form_params(form, metric), centroids=rows_centroids(metric, cents))
        exp = ix.export()
    oi, od, probes = oracle_on_structure(*exp, q, NPROBE, ROWS_K, metric)
    check_row_inputs(exp, kind_of, probes, oi, metric, level)
    return ix, x, kind_of, q, oi, od


ROW_SETTINGS = [("default", {}), ("fp16", {}), ("i8r", {}), ("default", {"ivf_h16": "0"}), ("default", {"ivf_pass": "0"})]


@gpu
@pytest.mark.parametrize("form,knobs", ROW_SETTINGS, ids=["default", "fp16", "i8r", "split_bf16", "grouped_scan"])
@pytest.mark.parametrize("level", ["moderate", "extreme"])
@pytest.mark.parametrize("metric", METRICS)
def test_special_rows_in_the_index(metric, level, form, knobs, opt, request):
    """Rows that are zero, subnormal, tiny, huge (moderate) and NaN, inf, FLT_MAX, beyond the 1e30 gate (extreme) in the lists of an
    index: the oracle's answer bit for bit in every form.  With the extreme rows the candidate pass must be off."""
    ix, _, _, q, oi, od = rows_case(metric, level, form)
    for name, value in knobs.items():
        opt(name, value)
    p0 = capi.prefilter_stats()
    ids, dis = ix.search(q, ROWS_K, "nprobe=%d" % NPROBE)
    p1 = capi.prefilter_stats()
    same(ids, dis, oi, od)
    if level == "extreme":
        assert p1[0] == p0[0], "the candidate pass ran over an index with rows beyond its error model"
    else:
        print(request.node.name, "shadow form %d," % shadow_form(ix), "candidate pass ran:", p1[0] > p0[0], "fallbacks: %d of %d queries"
              % (p1[1] - p0[1], len(q)))


@gpu
@pytest.mark.parametrize("level", ["moderate", "extreme"])
@pytest.mark.parametrize("metric", METRICS)
def test_special_rows_one_query_at_a_time(metric, level, opt):
    """lat_path = 2 with nq = 1, host and device entry: the queries placed on the special rows and against the lists."""
    ix, _, kind_of, q, oi, od = rows_case(metric, level, "default")
    opt("lat_path", "2")
    for i in list(range(4)) + list(range(128, len(q))):
        same(*ix.search(q[i:i + 1], ROWS_K, "nprobe=%d" % NPROBE), oi[i:i + 1], od[i:i + 1], "host entry, query %d:" % i)
        same(*device_search(ix, q[i:i + 1], ROWS_K, NPROBE), oi[i:i + 1], od[i:i + 1], "device entry, query %d:" % i)


@gpu
@pytest.mark.parametrize("form", ["default", "fp16", "i8r"])
@pytest.mark.parametrize("metric", METRICS)
def test_extreme_rows_fed_in_a_chunk_of_their_own(metric, form):
    """msvs_index_add refuses a built index, so rows cannot follow a build; the nearest thing a host can do is feed them as a last
    chunk of their own: ordinary rows first, then every extreme row in one add.  The shadow and the norms see them like any row."""
    cents, x, kind_of, q = rows_data("extreme")
    special = np.array(sorted(kind_of))
    order = np.concatenate([np.setdiff1d(np.arange(len(x)), special), special])
    n0 = len(x) - len(special)
    ix = build_ivf(x[order], metric, ROWS_NLIST, form_params(form, metric), centroids=rows_centroids(metric, cents), chunks=((0, n0), (n0, len(x))))
    with pytest.raises(capi.MsvsError):
        ix.add(x[special])
    p0 = capi.prefilter_stats()
    ids, dis = ix.search(q, ROWS_K, "nprobe=%d" % NPROBE)
    assert capi.prefilter_stats()[0] == p0[0]
    oi, od, _ = oracle_on_exported(ix, q, NPROBE, ROWS_K, metric)
    same(ids, dis, oi, od)
    found = {int(i) for i in oi[oi >= n0].tolist()}
    assert {kind_of[int(special[i - n0])] for i in found} >= FOUND[metric]
    ix.close()


@gpu
@pytest.mark.parametrize("setting", [{"flat_mfma": "2"}, {"flat_mfma": "0"}, {"flat_mfma": "2", "cand_cap": "1024"}],
                         ids=["shadow_pass", "canonical", "cand_cap_1024"])
@pytest.mark.parametrize("level", ["moderate", "extreme"])
@pytest.mark.parametrize("metric", METRICS)
def test_special_rows_in_a_flat_index(metric, level, setting, opt):
    _, x, kind_of, q = rows_data(level)
    labels = np.arange(len(x), dtype=np.int64) * 2 + 1
    ix = capi.Index(capi.INDEX_FLAT, metric, x.shape[1])
    ix.add(x, labels)
    ix.build()
    for name, value in setting.items():
        opt(name, value)
    oi, od = flat_reference(metric, level)
    same(*ix.search(q, ROWS_K), oi, od, "batch:")
    same(*ix.search(q[128:132], ROWS_K), oi[128:132], od[128:132], "four queries:")
    ix.close()


@functools.lru_cache(maxsize=None)
def flat_reference(metric, level):
    _, x, _, q = rows_data(level)
    return oracle_flat(q, x, ROWS_K, metric, labels=np.arange(len(x), dtype=np.int64) * 2 + 1)


@gpu
@pytest.mark.parametrize("level", ["moderate", "extreme"])
def test_special_rows_in_a_resident_block(level):
    """knn_resident over a Cache block uploaded with normalize = True (the host's cosine scan without an index) and without."""
    _, x, _, q = rows_data(level)
    cache = capi.Cache(64 << 20)
    raw, unit = cache.upload("special/raw", 0, x), cache.upload("special/unit", 0, x, normalize=True)
    for metric in (L2, IP):
        same(*capi.knn_resident(raw, q, ROWS_K, metric, x.shape[1]), *o.knn(q, x, ROWS_K, OM[metric]), NAME[metric])
    qn = o.normalize_rows(q)
    same(*capi.knn_resident(unit, qn, ROWS_K, IP, x.shape[1]), *o.knn(qn, o.normalize_rows(x), ROWS_K, o.METRIC_IP), "normalised block")
    cache.release(raw)
    cache.release(unit)
    cache.close()


@gpu
@pytest.mark.parametrize("d", [77, 100])
def test_normalize_special_rows(d):
    """capi.normalize against o.normalize_rows: a sum of squares below FLT_EPSILON leaves the row, an overflowing one divides by inf
    (every finite element becomes +-0), NaN and inf rows become NaN."""
    rng = np.random.default_rng(d)
    n = 512
    home = rng.integers(0, 8, n)
    x, kind_of = special_rows(rng.standard_normal((n, d), dtype=F), home, EXTREME_ROWS + ("flt_max", "x1e-30", "flt_min"))
    a, b = capi.normalize(x), o.normalize_rows(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "rows %s" % sorted({kind_of.get(int(r), "ordinary") for r in
                                                                                   np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:, 0]})
    by_kind = {kind: row for row, kind in kind_of.items()}
    assert (b[by_kind["e3e19"]] == 0).all() and (b[by_kind["flt_max_row"]] == 0).all()
    assert np.isnan(b[by_kind["pos_inf"]]).sum() == 1 and (b[by_kind["pos_inf"]] == 0).sum() == d - 1 and np.isnan(b[by_kind["nan_one"]]).all()
    assert np.array_equal(b[by_kind["x1e-20"]].view(np.uint32), x[by_kind["x1e-20"]].view(np.uint32))


# ---------------------------------------------------------------------------------------- 3. coded indexes and brute force

@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_through_the_sq_index(metric):
    rng = np.random.default_rng(40 + metric)
    dim, nlist, n = 100, 8, 3000
    centres, x = sq.blobs(rng, n, dim, nlist)
    ix = capi.SqIndex(metric, dim)
    ix.set_codebook(centres, np.full(dim, -1.5, F), np.full(dim, 1.5, F))
    ix.add(x, np.arange(n, dtype=np.int64) * 3)
    ix.build()
    exp = ix.export()
    q, _ = special_queries(x[:64] + F(0.1))
    ref = sq.ref_search(exp, sq.decoded(exp), q, NPROBE, K, metric)
    sq.same(ix.search(q, K, "nprobe=%d" % NPROBE), ref)
    sq.same(device_search(ix, q, K, NPROBE), ref)
    ix.close()


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries_through_the_pq_index(metric):
    ix, exp, xh, x = pq.by_hand(np.random.default_rng(50 + metric), metric, 100, 20, 8, 3000)
    q, _ = special_queries(x[:64] + F(0.1))
    ref = pq.ref_search(exp, xh, q, NPROBE, K, metric)
    pq.same(ix.search(q, K, "nprobe=%d" % NPROBE), ref)
    pq.same(device_search(ix, q, K, NPROBE), ref)
    ix.close()


@gpu
@pytest.mark.parametrize("k", [10, 300])
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_special_queries_through_brute_force(metric, k):
    """capi.knn over 1000 rows; k = 300 goes in rounds of 256."""
    rng = np.random.default_rng(60)
    y, q0 = blobs(rng, 8, 1000, 64, 100)
    q, _ = special_queries(q0)
    same(*capi.knn(q, y, k, metric), *o.knn(q, y, k, OM[metric]))
