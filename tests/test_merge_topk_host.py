"""The top-k merge of partial lists: a sort reference in plain numpy, the input models shared with the device tests
(test_merge_topk.py), and the CPU form msvs_host_merge_topk against that reference.

The reference uses no project code.  Per query it takes every (dis, id) of every part that is admitted -- id >= 0, distance not NaN
and strictly better than the neutral value (< FLT_MAX for L2, > -FLT_MAX for IP) -- sorts by the oracle's better(): distances as
FLOATS (ascending for L2, descending for IP, so -0 and +0 tie), ties by ascending id, every copy of a duplicated (dis, id) kept;
the first k entries are the answer and the remaining slots are id -1 at the neutral distance.  Every comparison is exact: ids with
==, distances on their uint32 view (by value only where -0 meets +0)."""
import ctypes as C

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import myscaledb_amd.host as host

F = np.float32
L2, IP = capi.METRIC_L2, capi.METRIC_IP
METRICS = [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")]
FLT_MAX = np.finfo(F).max
ID_TOP = 2 ** 32 - 2  # the largest id of the library


def neutral(metric):
    return F(-FLT_MAX) if metric == IP else F(FLT_MAX)


def admitted(ids, dis, metric):
    with np.errstate(invalid="ignore"):
        return (ids >= 0) & ((dis > -FLT_MAX) if metric == IP else (dis < FLT_MAX))  # (NaN: both comparisons are false)


def _order_key(dis, metric):
    with np.errstate(invalid="ignore"):  # (a signalling NaN on its way to a hole)
        d = dis.astype(np.float64)
    return -d if metric == IP else d


def reference_merge(ids, dis, metric, k=None):
    """ids / dis [nparts, nq, k_in] -> (ids [nq, k], dis [nq, k]); k defaults to k_in."""
    nparts, nq, k_in = ids.shape
    k = k_in if k is None else k
    out_i, out_d = np.full((nq, k), -1, np.int64), np.full((nq, k), neutral(metric), F)
    for q in range(nq):
        i, d = ids[:, q, :].reshape(-1), dis[:, q, :].reshape(-1)
        m = admitted(i, d, metric)
        i, d = i[m], d[m]
        o = np.lexsort((i, _order_key(d, metric)))[:k]  # by distance as a float, then by id; stable, so every copy stays
        out_i[q, :len(o)], out_d[q, :len(o)] = i[o], d[o]
    return out_i, out_d


def canonical(ids, dis, metric):
    """Every [k] list in the order a search writes: the admitted entries by the reference order, best first, everything else behind."""
    ids, dis = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dis, F)
    hole = ~admitted(ids, dis, metric)
    key = np.where(hole, 0.0, _order_key(dis, metric))
    o = np.lexsort((ids, key, hole), axis=-1)
    return np.take_along_axis(ids, o, -1), np.take_along_axis(dis, o, -1)


def same(got_i, got_d, ref_i, ref_d, what="", by_value=False):
    got_d, ref_d = np.ascontiguousarray(got_d, F), np.ascontiguousarray(ref_d, F)
    eq_d = (got_d == ref_d) if by_value else (got_d.view(np.uint32) == ref_d.view(np.uint32))
    bad = np.flatnonzero((got_i != ref_i).any(axis=1) | ~eq_d.all(axis=1))
    if len(bad):
        r = int(bad[0])
        c = np.flatnonzero((got_i[r] != ref_i[r]) | ~eq_d[r])[:6]
        raise AssertionError("%s: queries %s differ from the reference; query %d slots %s: got ids %s dis %s, reference ids %s dis %s"
                             % (what, bad.tolist()[:8], r, c.tolist(), got_i[r, c].tolist(), got_d[r, c].tolist(), ref_i[r, c].tolist(),
                                ref_d[r, c].tolist()))


# ---------------------------------------------------------------------------------------- the input models

MODELS = ("distinct", "ties", "equal", "duplicates", "ragged", "short", "subnormal", "inf_best", "nan", "neutral", "id_edges")


def _distinct_ids(rng, shape):
    n = int(np.prod(shape))
    return (rng.permutation(n).astype(np.int64) * 7919 % (ID_TOP + 1)).reshape(shape) if n else np.zeros(shape, np.int64)


def _cut(ids, dis, keep, metric, rng=None):
    """Entries past keep[p, q] become holes: id -1 at the neutral distance (rng: some carry another id < 0 and a distance that
    would win, which the id alone must keep out)."""
    hole = np.arange(ids.shape[2])[None, None, :] >= keep[:, :, None]
    ids[hole], dis[hole] = -1, neutral(metric)
    if rng is not None:
        odd = hole & (rng.random(ids.shape) < 0.5)
        ids[odd] = rng.choice(np.array([-1, -7, -2 ** 40], np.int64), int(odd.sum()))
        dis[odd] = rng.choice(np.array([0.0, -3.0, 3.0], F), int(odd.sum()))
    return ids, dis


def _junk_share(nparts, nq):
    """The share of entries that carry a valid id and a distance no merge admits, per query [1, nq, 1]: a fifth in the odd queries;
    in the even ones so many that fewer than k entries remain, so a form that admits one shows it."""
    return np.where(np.arange(nq) % 2 == 1, 0.2, 1 - 0.6 / nparts)[None, :, None]


def make_parts(model, nparts, nq, k, metric, seed=0):
    """-> (ids [nparts, nq, k] int64, dis f32) of `model`, every list canonical with its holes at the end."""
    rng = np.random.default_rng([seed, nparts, nq, k, metric, MODELS.index(model) if model in MODELS else 99])
    shape = (nparts, nq, k)
    ids = _distinct_ids(rng, shape)
    dis = rng.standard_normal(shape, dtype=F)  # distinct, mixed sign
    if model == "distinct":
        pass
    elif model == "mixed":
        # one (distance, id) table per query, entries drawn from it with repetition: ties between ids, the same key in several
        # parts, lists of every length
        pool = max(4, nparts * k // 2)
        pi, pd = _distinct_ids(rng, (nq, pool)), (np.round(rng.standard_normal((nq, pool)) * 8) / 8 + 0.0).astype(F)  # (+ 0.0: no -0)
        pick = rng.integers(0, pool, shape)
        qq = np.arange(nq)[None, :, None]
        ids, dis = pi[qq, pick], pd[qq, pick]
        keep = np.where(rng.random((nparts, nq)) < 0.7, k, rng.integers(0, k + 1, (nparts, nq)))
        ids, dis = _cut(ids, dis, keep, metric)
    elif model == "ties":
        dis = rng.integers(0, 6, shape).astype(F)
    elif model == "equal":
        dis = np.full(shape, 1.5, F)
    elif model == "duplicates":
        # the same list in every part (overlapping parts, replicated shards), each part keeping a prefix of its own length
        ids = np.broadcast_to(_distinct_ids(rng, (1, nq, k)), shape).copy()
        dis = np.broadcast_to(rng.integers(0, 30, (1, nq, k)).astype(F), shape).copy()
        ids, dis = canonical(ids, dis, metric)
        ids, dis = _cut(ids, dis, rng.integers((k + 1) // 2, k + 1, (nparts, nq)), metric)
    elif model == "ragged":
        keep = rng.integers(0, k + 1, (nparts, nq))
        keep[nparts // 2, :] = 0  # an empty part
        keep[:, 0] = 0            # a query whose parts are all empty
        ids, dis = _cut(ids, dis, keep, metric, rng)
    elif model == "short":
        # fewer valid entries in total than k: one entry in each of the first (k - 1) // 2 parts at the most
        keep = (np.arange(nparts) < (k - 1) // 2).astype(np.int64)[:, None].repeat(nq, 1)
        ids, dis = _cut(ids, dis, keep, metric)
    elif model == "subnormal":
        bits = rng.integers(1, 1 << 23, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31)
        dis = bits.view(F)
    elif model == "inf_best":
        dis[rng.random(shape) < 0.05] = np.inf if metric == IP else -np.inf  # admitted, and first
    elif model == "nan":
        m = rng.random(shape) < _junk_share(nparts, nq)
        dis[m] = rng.choice(np.array([0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001], np.uint32), int(m.sum())).view(F)
    elif model == "neutral":
        m, share = rng.random(shape), _junk_share(nparts, nq)
        dis[m < share / 2] = neutral(metric)
        dis[(m >= share / 2) & (m < share)] = -np.inf if metric == IP else np.inf
    elif model == "id_edges":
        dis = rng.integers(0, 3, shape).astype(F)
        edge = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, ID_TOP - 1, ID_TOP], np.int64)
        m = rng.random(shape) < 0.3
        ids[m] = rng.choice(edge, int(m.sum()))
        if nparts * k >= 2:
            ids[0, :, 0], ids[-1, :, -1] = 0, ID_TOP
    else:
        raise KeyError(model)
    return canonical(ids, dis, metric)


def signed_zero_parts(nparts, nq, k, metric, seed=0):
    """Zeros of both signs as the best distance of every query, about 0.6 k of them so that all reach the merged list, with distinct
    ids: the float order lets the id decide between -0 and +0, an order on the bit patterns puts every -0 before every +0 (L2) or
    behind it (IP).  Every query also holds the pair (+0, id a), (-0, id b) with the ids the way round that separates the rules."""
    rng = np.random.default_rng([seed, nparts, nq, k, metric])
    shape = (nparts, nq, k)
    ids = _distinct_ids(rng, shape) + 16
    worse = np.array([1.0, 2.0], F) * (-1 if metric == IP else 1)
    dis = np.where(rng.random(shape) < 0.6 / nparts, rng.choice(np.array([-0.0, 0.0], F), shape), rng.choice(worse, shape))
    a, b = (3, 9) if metric == L2 else (9, 3)  # L2: +0 has the smaller id, the bits order -0 first; IP: the other way round
    ids[0, :, 0], dis[0, :, 0] = a, F(0.0)
    ids[-1, :, -1], dis[-1, :, -1] = b, F(-0.0)
    return canonical(ids, dis, metric)


def shuffled(ids, dis, seed=1):
    """every [k] list in a random order of its own (holes anywhere)"""
    rng = np.random.default_rng(seed)
    o = np.argsort(rng.random(ids.shape), axis=-1)
    return np.take_along_axis(ids, o, -1), np.take_along_axis(dis, o, -1)


# ---------------------------------------------------------------------------------------- the reference itself

def test_reference_on_a_case_worked_by_hand():
    """Keeps the other tests from agreeing with a wrong reference: three parts of k = 3, every rule once."""
    nan = np.nan
    ids = np.array([[[5, 2, -1]], [[7, 5, 1]], [[4, 3, 6]]], np.int64)
    l2 = np.array([[[1.0, 2.0, 0.0]], [[-0.0, 1.0, FLT_MAX]], [[0.0, nan, np.inf]]], F)
    ri, rd = reference_merge(ids, l2, L2)
    assert ri.tolist() == [[4, 7, 5]] and rd.tolist() == [[0.0, 0.0, 1.0]]  # 4 before 7: +0 and -0 tie, the id decides
    ri, rd = reference_merge(ids, l2, L2, k=7)
    assert ri.tolist() == [[4, 7, 5, 5, 2, -1, -1]] and rd[0, 3:].tolist() == [1.0, 2.0, FLT_MAX, FLT_MAX]  # both copies of (1, 5)
    ip = np.array([[[2.0, 1.0, 9.0]], [[np.inf, 1.0, -FLT_MAX]], [[1.0, nan, -np.inf]]], F)
    ri, rd = reference_merge(ids, ip, IP)
    assert ri.tolist() == [[7, 5, 2]] and rd.tolist() == [[np.inf, 2.0, 1.0]]
    ri, rd = reference_merge(ids, ip, IP, k=6)
    assert ri.tolist() == [[7, 5, 2, 4, 5, -1]] and rd[0, 5] == -FLT_MAX
    ci, cd = canonical(ids, l2, L2)
    assert ci.tolist() == [[[5, 2, -1]], [[7, 5, 1]], [[4, 3, 6]]] and np.isnan(cd[2, 0, 1])


@pytest.mark.parametrize("metric", METRICS)
def test_models_are_what_their_names_say(metric):
    """Every list of every model is canonical with its holes at the end, and each model holds what it is there for."""
    nparts, nq, k = 6, 3, 20
    for model in MODELS + ("mixed",):
        ids, dis = make_parts(model, nparts, nq, k, metric)
        ok = admitted(ids, dis, metric)
        assert (ok[..., :-1] >= ok[..., 1:]).all(), model  # holes at the end
        for p in range(nparts):
            ri, rd = reference_merge(ids[p:p + 1], dis[p:p + 1], metric)
            same(np.where(ok[p], ids[p], -1), np.where(ok[p], dis[p], neutral(metric)), ri, rd, model)  # sorted
        n_ok = ok.sum(axis=(0, 2))
        if model == "short":
            assert (n_ok < k).all() and (n_ok > 0).all()
        elif model == "ragged":
            assert n_ok[0] == 0 and not ok[nparts // 2].any() and (n_ok[1:] > k).all() and ((ids < -1) & ~ok).any()
        elif model == "duplicates":
            assert all(len(set(zip(ids[:, q][ok[:, q]].tolist(), dis[:, q][ok[:, q]].tolist()))) <= k for q in range(nq))
        elif model == "nan":
            assert (np.isnan(dis) & (ids >= 0)).any()
        elif model == "neutral":
            assert ((dis == neutral(metric)) & (ids >= 0)).any() and (np.isinf(dis) & (ids >= 0) & ~ok).any()
        elif model == "inf_best":
            assert (np.isinf(dis) & ok).any() and np.isinf(reference_merge(ids, dis, metric)[1][:, 0]).all()
        elif model == "subnormal":
            assert (np.abs(dis) < np.finfo(F).tiny).all() and (dis != 0).all() and (dis < 0).any() and (dis > 0).any()
        elif model == "id_edges":
            assert (ids == 0).any() and (ids == ID_TOP).any() and (ids == 2 ** 31).any()
        elif model == "equal":
            assert len(np.unique(dis.view(np.uint32))) == 1
        elif model == "mixed":
            assert (~ok).any() and len(np.unique(dis[ok])) < ok.sum() // 2
    ids, dis = signed_zero_parts(nparts, nq, k, metric)
    z = dis.view(np.uint32)
    assert (z == 0).any() and (z == 0x80000000).any()
    ri, _ = reference_merge(ids, dis, metric)
    by_bits = reference_merge(ids, np.where(z == 0x80000000, F(-1e-40), dis), metric)[0]
    assert (ri != by_bits).any(), "the float order and the order of the bit patterns must differ on this input"


# ---------------------------------------------------------------------------------------- msvs_host_merge_topk

HOST_SHAPES = [(1, 1), (3, 85), (5, 52), (70, 63), (6145, 1), (48, 129)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("model", MODELS + ("mixed",))
def test_host_merge_matches_the_sort_reference(model, metric):
    """Finding 2 (NaN breaks the comparator's ordering) and finding 3 (an entry at or beyond the neutral distance is admitted by its
    id alone) show in the nan and neutral models."""
    for i, (nparts, k) in enumerate(HOST_SHAPES):
        ids, dis = make_parts(model, nparts, (1, 3, 4, 5, 9)[i % 5], k, metric)
        same(*host.merge_topk(ids, dis, metric), *reference_merge(ids, dis, metric), what="%s (%d, %d)" % (model, nparts, k))


@pytest.mark.parametrize("metric", METRICS)
def test_host_merge_signed_zero_follows_the_float_order(metric):
    """-0 and +0 tie and the id decides (the oracle's better()); distances compared by value."""
    for nparts, k in HOST_SHAPES:
        ids, dis = signed_zero_parts(nparts, 3, k, metric)
        same(*host.merge_topk(ids, dis, metric), *reference_merge(ids, dis, metric), what="(%d, %d)" % (nparts, k), by_value=True)


@pytest.mark.parametrize("metric", METRICS)
def test_host_merge_is_order_free(metric):
    """The CPU form sorts everything: shuffled lists, holes anywhere, NaN among them, give the reference's answer."""
    for model in ("mixed", "nan", "ragged"):
        ids, dis = shuffled(*make_parts(model, 7, 5, 40, metric))
        same(*host.merge_topk(ids, dis, metric), *reference_merge(ids, dis, metric), what=model)


@pytest.mark.parametrize("metric", METRICS)
def test_host_merge_keeps_64_bit_ids(metric):
    """The CPU form carries ids as they are: above 2^32 - 2 they neither wrap nor collide (the device forms document [0, 2^32 - 1))."""
    ids, dis = make_parts("ties", 4, 3, 12, metric)
    big = ids.copy()
    big[ids % 3 == 0] += 2 ** 32      # the same low word as a smaller id ...
    big[ids % 3 == 1] += 2 ** 40 + 5  # ... and far beyond
    big, dis = canonical(big, dis, metric)
    gi, gd = host.merge_topk(big, dis, metric)
    same(gi, gd, *reference_merge(big, dis, metric))
    assert (gi >= 2 ** 32).any()


def _host_rc(ids, dis, nparts, nq, k, metric, oi, od):
    return host.lib().msvs_host_merge_topk(capi._p(ids, C.c_int64), capi._p(dis, C.c_float), C.c_size_t(nparts), C.c_size_t(nq), C.c_size_t(k),
                                           int(metric), capi._p(oi, C.c_int64), capi._p(od, C.c_float))


def test_host_merge_errors_and_empty_shapes():
    ids, dis = make_parts("distinct", 2, 3, 4, L2)
    oi, od = np.full((3, 4), 77, np.int64), np.full((3, 4), 7.0, F)
    assert _host_rc(ids, dis, 2, 3, 4, capi.METRIC_COSINE, oi, od) == capi.ERR_NOT_IMPLEMENTED
    assert _host_rc(ids, dis, 2, 0, 4, L2, oi, od) == 0 and _host_rc(ids, dis, 2, 3, 0, L2, oi, od) == 0  # no-ops
    assert (oi == 77).all() and (od == 7.0).all()
    for metric in (L2, IP):
        oi[:], od[:] = 77, 7.0
        assert _host_rc(None, None, 0, 3, 4, metric, oi, od) == 0  # no parts: nq * k empty slots
        assert (oi == -1).all() and (od == neutral(metric)).all()
