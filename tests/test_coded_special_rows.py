"""Non-finite, overflowing, zero and subnormal rows STORED in the coded indexes (IVFSQ at 8, 4 and 16 bits, IVFPQ at 8 and 4 bits with
and without query tables), against the CPU reference bit for bit.  test_special_values.py feeds such values to these indexes as
queries only; here they pass through the coarse assignment, the encoder, the decoder, the scan's admission, the rank rounds, the
filter and the exact re-rank.

The rows, centroids and queries are test_special_values.rows_data's.  Every index gets its codebook by hand: the centroids of the
data, and the quantiser vmin = -1.5, vmax = 1.5 (the blob sigma is 0.3: ordinary rows are not clamped, the special rows are) or
sub-codebooks drawn here.  The reference is the composition the other coded tests use -- the numpy encode / decode of test_sq_bits.py
and test_pq_ivf.py, oracle.ivf_search over the decoded matrix (the query-table form: test_pq_query_tables.ref_search), cosine via
normalised rows and 1 - ip -- with one rule added: at 8 and 4 bits a NaN t encodes to code 0 (include/msvs.h).  At 16 bits every NaN
here is a quiet one, which numpy and the hardware convert to the same binary16 NaN.

The assignment rule (include/msvs.h, "as msvs_index_add does"): the score of centroid l is |c_l|^2 - 2 <c_l, x> (L2) or -<c_l, x>
(inner product, cosine); the smallest score that is not NaN and not above FLT_MAX wins, -inf included, the lowest l among equals; a
row without such a score goes to list 0.  Finite scores are compared by ivf_build_ref's rule for float data, with one term added to
the bound for products that underflow (below)."""
import functools

import numpy as np
import pytest

import ivf_build_ref as R
import myscaledb_amd.capi as capi
import test_pq_ivf as pq
import test_pq_query_tables as tq
import test_sq_bits as sqb
import test_sq_ivf as sq
from oracle import oracle as o
from test_refine import ref_refine, store_of
from test_special_values import (EXTREME_ROWS, MODERATE_ROWS, NPROBE, ROWS_D, ROWS_K, ROWS_N, ROWS_NLIST, device_search, rows_centroids,
                                 rows_data, same)

gpu = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
NAME = {L2: "l2", IP: "ip", COS: "cosine"}
METRICS = [pytest.param(m, id=NAME[m]) for m in (L2, IP, COS)]
LEVELS = ["moderate", "extreme"]
FLT_MAX = np.finfo(F).max
VMIN, VMAX = F(-1.5), F(1.5)
PQ_M = 20  # dsub = 5
# (kind, bits of a code, query_tables)
SQ_FORMS = [("sq", 8, 0), ("sq", 4, 0), ("sq", 16, 0)]
PQ_FORMS = [("pq", 8, 0), ("pq", 8, 1), ("pq", 4, 0), ("pq", 4, 1)]
FORMS = SQ_FORMS + PQ_FORMS
FORM_IDS = ["%s%d%s" % (k, b, "qt" if t else "") for k, b, t in FORMS]
CHUNKS = ((0, 1100), (1100, 1101), (1101, None))


# ---------------------------------------------------------------------------------------- the reference: assignment

def scores(xs, cent, ip):
    """-> (s [n, nlist], B [n, nlist]): the assignment scores in float64 from the f32 products (a product that overflows in f32 is
    +-inf here too, and +inf + -inf = NaN as in any order of the kernel's sum), and the bound of ivf_build_ref.float_scores on the
    error of the kernel's f32 score, plus (d + 2) 2^-126 per product sum: a product or partial sum below FLT_MIN may be rounded to a
    subnormal or flushed to zero, and either is less than 2^-126 off."""
    d = xs.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        p = (xs[:, None, :] * cent[None, :, :]).astype(F).astype(np.float64)
        dot, adot = p.sum(axis=2), np.abs(p).sum(axis=2)
        cn = (cent.astype(np.float64) ** 2).sum(axis=1)[None, :]
        tiny = np.where(adot > 0, (d + 2) * 2.0 ** -126, 0.0)  # (products that are all +-0 neither round nor underflow)
        if ip:
            s, B = -dot, (d + 2) * R.U * adot + tiny
        else:
            s, B = cn - 2 * dot, (d + 2) * R.U * (cn + 2 * adot) + 2 * tiny
        big = np.abs(s) > FLT_MAX
        assert not (big & (np.abs(s) < 1.001 * FLT_MAX)).any(), "a score at the edge of the f32 range"
        s = np.where(big, np.sign(s) * np.inf, s)  # (NaN compares false: it stays)
    return s, B


def assign_rule(xs, cent, ip):
    """-> (want [n], definite [n], allowed [n, nlist]): the list the rule gives every row; allowed[r, l]: list l is within the two
    scores' error bounds of the winner's (an exact tie of two scores without error, as between the all-zero products of a zero row,
    allows the lower list only); definite: `want` is the only list allowed (every row without a finite score is definite)."""
    s, B = scores(xs, cent, ip)
    n, nlist = s.shape
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(s) & (s <= FLT_MAX)
        neg_inf = valid & (s == -np.inf)
    finite = valid & ~neg_inf
    fin = np.where(finite, s, np.inf)
    Bf = np.where(finite, B, 0.0)
    want = np.argmin(fin, axis=1)  # (the first minimum: the lowest list among equals)
    rows = np.arange(n)
    with np.errstate(invalid="ignore"):
        allowed = finite & (fin - fin[rows, want][:, None] <= Bf + Bf[rows, want][:, None])
    exact_tie = (fin == fin[rows, want][:, None]) & (Bf == 0) & (Bf[rows, want][:, None] == 0)
    allowed &= ~exact_tie
    none = ~valid.any(axis=1)
    has_ni = neg_inf.any(axis=1)
    want[none] = 0
    want[has_ni] = np.argmax(neg_inf[has_ni], axis=1)
    allowed[none | has_ni] = False
    allowed[rows, want] = True
    return want.astype(np.int64), allowed.sum(axis=1) == 1, allowed


def check_assignment(got, want, definite, allowed):
    got = np.asarray(got, np.int64)
    bad = np.flatnonzero(~allowed[np.arange(len(got)), got])
    assert bad.size == 0, "rows in a list the rule does not allow, first (row, got, want): %s" % [(int(r), int(got[r]), int(want[r])) for r in bad[:5]]
    assert (got[definite] == want[definite]).all()


# ---------------------------------------------------------------------------------------- the reference: codes

def sq_encode(x, c, vmin, vmax, bits):
    """test_sq_bits.encode with the rule for a NaN t written down: code 0 (C's fmaxf(0, NaN) = 0).  +-inf clamp as any value does.
    For rows without a NaN residual it IS test_sq_bits.encode (asserted in the CPU test)."""
    if bits == 16:
        return sqb.encode(x, c, vmin, vmax, 16)
    top = 15 if bits == 4 else 255
    step = sqb.step_of(vmin, vmax, bits)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (x - c).astype(F)
        t = ((r - vmin).astype(F) / step).astype(F)
        code = np.where(np.isnan(t), 0, np.clip(np.rint(t), 0, top))
    code[:, step == 0] = 0
    return code.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def codebooks(bits):
    """sub-codebooks drawn by hand, as test_pq_ivf.by_hand's"""
    return pq.random_codebooks(np.random.default_rng(900 + bits), PQ_M, ROWS_D // PQ_M)[:, :1 << bits].copy()


# ---------------------------------------------------------------------------------------- the inputs

@functools.lru_cache(maxsize=None)
def fed(metric, level):
    """rows_data(level) as the coded indexes get it: the centroids of the metric, the rows (one ordinary row left out where the list
    that the last row closes would have an even length by the rule), labels 3 * i shuffled with the largest on the last row, the
    queries, and the rule's list of every row."""
    cents, x, kind_of, q = rows_data(level)
    cent = np.ascontiguousarray(rows_centroids(metric, cents), F)
    for _ in range(2):
        want, definite, allowed = assign_rule(sq.stored(x, metric), cent, metric != L2)
        members = np.flatnonzero(want == want[-1])
        if len(members) % 2 == 1:
            break
        drop = next(int(r) for r in members if int(r) not in kind_of)
        x = np.delete(x, drop, axis=0)
        kind_of = {r - (r > drop): kind for r, kind in kind_of.items()}
    n = len(x)
    perm = np.random.default_rng(2024).permutation(n)
    perm[np.flatnonzero(perm == n - 1)[0]], perm[-1] = perm[-1], n - 1
    return cent, x, kind_of, (3 * perm).astype(np.int64), q, want, definite, allowed


def export_of(form, metric, level, lists, labels):
    """What export() of the index must return, from the rows, their lists and their labels: the reference encode in list-major order,
    rows of a list by ascending label."""
    kind, bits, _ = form
    cent, x, _, _, _, _, _, _ = fed(metric, level)
    order = np.lexsort((labels, lists))
    off = np.zeros(len(cent) + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=len(cent)), out=off[1:])
    xs, c = sq.stored(x, metric)[order], cent[lists[order]]
    if kind == "sq":
        lo, hi = np.full(ROWS_D, VMIN, F), np.full(ROWS_D, VMAX, F)
        return cent, lo, hi, off, sq_encode(xs, c, lo, hi, bits), labels[order]
    return cent, codebooks(bits), off, pq.encode(xs, c, codebooks(bits)), labels[order]


class Reference:
    """the expected export of one (form, metric, level, lists, labels), its decoded matrix and its searches, each computed once"""

    def __init__(self, form, metric, level, lists, labels):
        self.form, self.metric = form, metric
        self.exp = export_of(form, metric, level, lists, labels)
        if form[0] == "sq":
            cent, lo, hi, off, codes, _ = self.exp
            self.xh = sqb.decode(codes, cent[sq.lists_of(off)], lo, hi, form[1])
        else:
            self.xh = pq.decoded(self.exp)
        self.done = {}
        self.adc = {}

    def search(self, q, nprobe, k, alive=None, tag=None):
        key = (tag, len(q), nprobe, k, None if alive is None else alive.tobytes())
        if key not in self.done or tag is None:
            self.done[key] = self.compute(q, nprobe, k, alive, tag)
        return self.done[key]

    def compute(self, q, nprobe, k, alive, tag):
        kind, _, qt = self.form
        if kind == "sq":
            return sq.ref_search(self.exp, self.xh, q, nprobe, k, self.metric, alive=alive)
        if qt:
            return tq.ref_search(self.exp, q, nprobe, k, self.metric, alive=alive)
        return self.pq_search(q, nprobe, k, alive, tag)

    def pq_search(self, q, nprobe, k, alive, tag):
        """test_pq_ivf.ref_search with its ADC matrix (the costly part, which does not depend on nprobe, k or the filter) kept"""
        cent, cb, off, codes, labels = self.exp
        ip = self.metric != L2
        q = np.ascontiguousarray(o.normalize_rows(q) if self.metric == COS else q, F)
        _, _, probes = o.ivf_search(cent, off, self.xh, labels, q, nprobe, 1, o.METRIC_IP if ip else o.METRIC_L2)
        if tag is None or tag not in self.adc:
            self.adc[tag] = pq.adc(self.xh, q, cb.shape[0], ip)
        dis = self.adc[tag]
        lists = pq.lists_of(off)
        ids = np.full((len(q), k), -1, np.int64)
        out = np.full((len(q), k), -FLT_MAX if ip else FLT_MAX, F)
        ok_row = np.ones(len(labels), bool) if alive is None else np.array([l < len(alive) and alive[l] for l in labels], bool)
        for i in range(len(q)):
            d = dis[i]
            with np.errstate(invalid="ignore"):
                better = (d > -FLT_MAX) if ip else (d < FLT_MAX)
            cand = np.flatnonzero(np.isin(lists, probes[i]) & ok_row & better)
            key = pq.ordered(d[cand])
            order = cand[np.lexsort((labels[cand], ~key if ip else key))][:k]
            ids[i, :len(order)] = labels[order]
            out[i, :len(order)] = d[order]
        return ids, ((F(1) - out).astype(F) if self.metric == COS else out)


@functools.lru_cache(maxsize=None)
def _reference(form, metric, level, lists_bytes, labels_bytes):
    return Reference(form, metric, level, np.frombuffer(lists_bytes, np.int64), np.frombuffer(labels_bytes, np.int64))


def reference(form, metric, level, lists=None):
    """lists: the lists the index gave the rows (checked against the rule by the caller); None: the rule's own"""
    f = fed(metric, level)
    return _reference(form, metric, level, np.ascontiguousarray(f[5] if lists is None else lists, np.int64).tobytes(), f[3].tobytes())


def probes_of(ref, q, nprobe):
    cent, off, labels = ref.exp[0], ref.exp[-3], ref.exp[-1]
    ip = ref.metric != L2
    qs = o.normalize_rows(q) if ref.metric == COS else q
    return o.ivf_search(cent, off, ref.xh, labels, qs, nprobe, 1, o.METRIC_IP if ip else o.METRIC_L2)[2]


# ---------------------------------------------------------------------------------------- 0. the inputs against the reference (CPU)

# The kinds of special row that the reference's top-16 of some query holds (nprobe = 4 or nprobe = nlist, the two searches of
# test_search_over_special_rows), per form and metric on the extreme level -- derived on the CPU from the reference alone (run this
# module's derive_found()) and kept here as the kinds NOT found.  Why they are not:
#   - SQ 8 / 4 bits: every special row decodes to an ordinary in-range row.  A NaN element has code 0 and decodes to c + vmin: a
#     nan_one / nan_all row under L2 and inner product lies 1.5 below its centroid in one / in every column, behind every ordinary
#     row of its list for every query; cosine stores both as all-NaN rows, which sit in list 0 at c - 1.5 with the zero rows.
#   - SQ 16 bits: NaN and inf survive decode.  L2 distances to rows with such an element are NaN or inf, and the huge finite rows are
#     far from every query that probes their list; inner products with the +-inf rows are +inf for a query element of their sign
#     (found), NaN with flt_max_row (every column +inf); cosine stores inf and NaN rows as NaN rows.
#   - cosine, 4 bits: 24 rows are stored as zero or all but zero (pos_zero, neg_zero, x1e-41, x1e-20, and e3e19 and flt_max_row, whose
#     sum of squares overflows) and all sit in list 0; with a step of 0.2 against centroid elements of 0.1 their decoded rows differ
#     by the rounding alone and compete for the same 16 slots: pos_zero, neg_zero and flt_max_row lose everywhere.  The same at the
#     16-entry IVFPQ under inner product.  (The four kinds asked of every case -- pos_zero, neg_zero, x1e-41, x1e-20 -- are found
#     in all but these two.)
#   - IVFPQ: the decoded rows are finite whatever the row was; which of the far-off kinds a query finds depends on the codebook.
NOT_FOUND = {
    ("sq", 8, 0): {L2: {"nan_one", "nan_all"}, IP: {"nan_one", "nan_all"}, COS: set()},
    ("sq", 4, 0): {L2: {"nan_one", "nan_all"}, IP: {"nan_one", "nan_all"}, COS: {"flt_max_row", "neg_zero", "pos_zero"}},
    ("sq", 16, 0): {L2: {"e1e19", "e1e5", "e2e15", "e3e19", "flt_max_row", "nan_all", "nan_one", "neg_inf", "pos_inf", "x7e4"},
                    IP: {"flt_max_row", "nan_all", "nan_one"}, COS: {"nan_all", "nan_one", "neg_inf", "pos_inf"}},
    ("pq", 8, 0): {L2: {"e1e19", "e2e15", "nan_one", "pos_inf"}, IP: set(), COS: {"x7e4"}},
    ("pq", 8, 1): {L2: {"flt_max_row", "nan_all"}, IP: set(), COS: {"x7e4"}},
    ("pq", 4, 0): {L2: {"e1e19", "e2e15", "flt_max_row", "nan_all", "nan_one", "pos_inf"},
                   IP: {"flt_max_row", "nan_all", "nan_one", "neg_zero", "pos_inf", "pos_zero"}, COS: set()},
    ("pq", 4, 1): {L2: {"e1e19", "e2e15", "flt_max_row", "nan_all", "nan_one", "pos_inf"},
                   IP: {"flt_max_row", "nan_all", "nan_one", "neg_zero", "pos_inf", "pos_zero"}, COS: set()},
}
FOUND_CODED = {form: {m: frozenset(EXTREME_ROWS) - missing for m, missing in per.items()} for form, per in NOT_FOUND.items()}
ALWAYS = {"pos_zero", "neg_zero", "x1e-41", "x1e-20"}
ALWAYS_BUT = {(("sq", 4, 0), COS), (("pq", 4, 0), IP), (("pq", 4, 1), IP)}  # (above: the zero-like rows of one list outnumber k)


def found_kinds(form, metric, level):
    _, _, kind_of, labels, q, _, _, _ = fed(metric, level)
    ref = reference(form, metric, level)
    ids = np.concatenate([ref.search(q, nprobe, ROWS_K, tag="all")[0] for nprobe in (NPROBE, ROWS_NLIST)])
    kind_of_label = {int(labels[r]): kind for r, kind in kind_of.items()}
    return {kind_of_label[int(i)] for i in ids[ids >= 0].tolist() if int(i) in kind_of_label}


def derive_found():
    for kind, bits, qt in FORMS:
        print((kind, bits, qt), {NAME[m]: sorted(found_kinds((kind, bits, qt), m, "extreme")) for m in (L2, IP, COS)})


@pytest.mark.parametrize("metric", METRICS)
def test_inputs_against_the_reference(metric):
    """No GPU: what the GPU tests rely on, checked on the reference alone, so that none of them passes by testing nothing."""
    for level in LEVELS:
        cent, x, kind_of, labels, q, want, definite, allowed = fed(metric, level)
        n = len(x)
        assert set(kind_of.values()) == set(MODERATE_ROWS if level == "moderate" else EXTREME_ROWS) and n in (ROWS_N, ROWS_N - 1)
        assert sorted(labels.tolist()) == list(range(0, 3 * n, 3)) and labels[-1] == 3 * (n - 1) and (np.diff(labels) < 0).any()
        # the assignment: the rule is definite for all but a few rows, and for every row without a finite score
        xs = sq.stored(x, metric)
        assert (~definite).sum() <= 8, "the rule leaves %d rows open" % (~definite).sum()
        not_finite = ~np.isfinite(xs).all(axis=1)
        assert definite[not_finite].all() and (not_finite.sum() >= 12 if level == "extreme" else not not_finite.any())
        assert kind_of[n - 1] == "x7e4" and definite[-1] and (want == want[-1]).sum() % 2 == 1, "the last row closes a list of odd length"
        holding = {int(want[r]) for r in kind_of}
        assert len(holding) >= 3
        for form in FORMS:
            kind, bits, qt = form
            ref = reference(form, metric, level)
            probes = probes_of(ref, q, NPROBE)
            assert holding <= set(probes[probes >= 0].tolist()), "a list with special rows is never probed"
            found = found_kinds(form, metric, level)
            must = FOUND_CODED[form][metric] & set(kind_of.values())
            assert must <= found, (form, level, sorted(must - found))
            assert level != "extreme" or found == must, (form, sorted(found - must))
            assert ALWAYS <= must or (form, metric) in ALWAYS_BUT
            assert {"x1e-41", "x1e-20"} <= must
            if kind == "sq" and bits != 16:  # clamped codes decode to ordinary in-range rows
                assert np.isfinite(ref.xh).all() and (np.abs(ref.xh - cent[sq.lists_of(ref.exp[3])]) <= F(1.5001)).all()
                assert set(kind_of.values()) - must <= {"nan_one", "nan_all"} or (form, metric) in ALWAYS_BUT
            if kind == "sq" and bits == 16 and metric == IP and level == "extreme":
                assert {"pos_inf", "neg_inf"} <= must
            if kind == "pq":
                assert np.isfinite(ref.xh).all()
        if level != "extreme":
            continue
        # the encode wrapper is test_sq_bits.encode wherever no residual is NaN, and code 0 where one is
        lists = want
        lo, hi = np.full(ROWS_D, VMIN, F), np.full(ROWS_D, VMAX, F)
        with np.errstate(invalid="ignore"):
            nan_res = np.isnan((xs - cent[lists]).astype(F))
        clean = ~nan_res.any(axis=1)
        assert nan_res.any() and clean.sum() > n - 40
        for bits in (8, 4):
            mine = sq_encode(xs, cent[lists], lo, hi, bits)
            with np.errstate(over="ignore"):
                assert (mine[clean] == sqb.encode(xs[clean], cent[lists][clean], lo, hi, bits)).all() and (mine[nan_res] == 0).all()
                if bits == 8:
                    assert (mine[clean] == sq.encode(xs[clean], cent[lists][clean], lo, hi)).all()
            if metric != COS:
                assert (mine[xs == np.inf] == (15 if bits == 4 else 255)).all() and (mine[xs == -np.inf] == 0).all() and (xs == -np.inf).sum() == 4
        # 16 bits: NaN and inf survive decode, and a query meets them with 0 * inf or inf - inf
        ref = reference(("sq", 16, 0), metric, level)
        xh = ref.xh
        assert np.isnan(xh).any()
        h = ref.exp[4][np.isnan(xh)]
        assert set(h.tolist()) <= {0x7e00, 0xfe00}, "quiet NaNs only"
        if metric != COS:  # (cosine stores an inf row as a NaN row and an overflowing one as zeros: no inf reaches its codes)
            assert (xh == np.inf).any() and (xh == -np.inf).any()
            probes = probes_of(ref, q, NPROBE)
            lists_x = sq.lists_of(ref.exp[3])
            inf_rows = np.flatnonzero(np.isinf(xh).any(axis=1))
            met = False
            for i in range(len(q)):
                for r in inf_rows[np.isin(lists_x[inf_rows], probes[i])]:
                    at = np.isinf(xh[r])
                    met |= metric == L2 or bool((q[i][at] == 0).any())
            # (L2: a query with an infinite element is at distance inf from every centroid and probes nothing, so inf - inf never
            # meets a probed row; what the scan sees of such a row is the distance +inf, which is not admitted)
            assert met, "no query multiplies an inf by 0 (inner product) / meets a row with an inf element in a probed list (L2)"
        # a sub-vector with a NaN element has NaN sub-scores against every entry: code 0
        for bits in (8, 4):
            cref = reference(("pq", bits, 0), metric, level)
            order = np.lexsort((labels, lists))
            sub_nan = nan_res[order].reshape(n, PQ_M, -1).any(axis=2)
            assert sub_nan.any() and (cref.exp[3][sub_nan] == 0).all() and (cref.exp[3][~sub_nan] != 0).any()
        # the signed probes under inner product at 16 bits: several rows score +inf, others NaN
        if metric == IP:
            with np.errstate(invalid="ignore", over="ignore"):
                sc = q[128 + len(kind_of):128 + len(kind_of) + 8].astype(np.float64) @ np.where(np.isinf(xh), np.sign(xh) * 1e300, xh).astype(np.float64).T
                assert ((sc > 1e299).sum(axis=1) >= 2).all() and np.isnan(xh @ q[0]).sum() >= 4


# ---------------------------------------------------------------------------------------- the indexes (GPU)

def new_index(form, metric):
    kind, bits, qt = form
    if kind == "sq":
        return capi.SqIndex(metric, ROWS_D, sqb.params(bits))
    return capi.PqIndex(metric, ROWS_D, "m=%d,bit_size=%d,query_tables=%d" % (PQ_M, bits, qt))


def build(form, metric, level, order=None, chunks=CHUNKS, labelled=True):
    """-> (index, export): the codebook by hand, the rows fed in `chunks` (in `order`: a permutation of the rows, labels travelling
    with them)"""
    cent, x, _, labels, _, _, _, _ = fed(metric, level)
    ix = new_index(form, metric)
    if form[0] == "sq":
        ix.set_codebook(cent, np.full(ROWS_D, VMIN, F), np.full(ROWS_D, VMAX, F))
    else:
        ix.set_codebook(cent, codebooks(form[1]))
    order = np.arange(len(x)) if order is None else order
    for a, b in chunks:
        ix.add(x[order[a:b]], labels[order[a:b]] if labelled else None)
    ix.build()
    return ix, ix.export()


def lists_of_export(exp, labels):
    """the list of every fed row from an export's offsets and labels"""
    off, elab = exp[-3], exp[-1]
    at = np.empty(int(labels.max()) + 1, np.int64)
    at[elab] = sq.lists_of(off)
    return at[labels]


@functools.lru_cache(maxsize=None)
def case(form, metric, level):
    """One index per (form, metric, level), its export checked against the rule and the reference encode, and its reference."""
    _, _, _, labels, _, want, definite, allowed = fed(metric, level)
    ix, exp = build(form, metric, level)
    assert sorted(exp[-1].tolist()) == sorted(labels.tolist())
    lists = lists_of_export(exp, labels)
    check_assignment(lists, want, definite, allowed)
    ref = reference(form, metric, level, lists)
    for got, exp_ref in zip(exp, ref.exp):
        assert got.dtype == exp_ref.dtype and got.shape == exp_ref.shape
        assert got.tobytes() == exp_ref.tobytes(), "rows %s" % np.unique(np.argwhere(got != exp_ref)[:, 0])[:8].tolist()
    return ix, ref


# ---------------------------------------------------------------------------------------- 1. codes and assignment

@gpu
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("metric", METRICS)
def test_codes_lists_and_assignment(metric, level, form):
    """export(): every row in the list the rule gives it (the rows without a finite score included), codes and offsets equal to the
    reference encode of the fed rows against their lists' centroids, byte for byte (inside case()).  The rows that carry a NaN: code
    0 in every column (SQ 8 / 4) or sub-space (PQ) that holds one."""
    ix, ref = case(form, metric, level)
    cent, x, kind_of, labels, _, want, _, _ = fed(metric, level)
    assert ix.ready and ix.num_data == len(x) and ix.num_lists == ROWS_NLIST
    codes, elab = ref.exp[-2], ref.exp[-1]
    if level == "extreme" and form[1] != 16:
        row_of_label = {int(l): r for r, l in enumerate(labels)}
        xs = sq.stored(x, metric)[[row_of_label[int(l)] for l in elab]]
        nan_at = np.isnan(xs)
        assert nan_at.any()
        if form[0] == "sq":
            assert (codes[nan_at] == 0).all()
        else:
            assert (codes[nan_at.reshape(len(xs), PQ_M, -1).any(axis=2)] == 0).all()


@gpu
@pytest.mark.parametrize("bits", [8, 4, 16])
def test_codes_of_special_elements_by_hand(bits):
    """Zero centroids, vmin = -1.5, vmax = 1.5, one special element per row in column 3 (a whole block at no width: d = 40) and in
    the last column: NaN, +inf, -inf, FLT_MAX, 1e-41 and -1e-41.  8 / 4 bits: 0 (the NaN rule), top, 0, top, and the code of a zero
    residual: t = fl(1.5 / fl(3 / 255)) = 127.5 and fl(1.5 / fl(3 / 15)) = 7.5, both exactly, ties that go to the even codes 128 and 8
    (worked out with numpy's f32 arithmetic, not taken from the library).  16 bits: the quiet NaN, +inf, -inf, +inf (FLT_MAX
    overflows binary16) and +-0 (1e-41 is below half of the smallest binary16 subnormal)."""
    dim = 40
    vals = np.array([np.nan, np.inf, -np.inf, FLT_MAX, 1e-41, -1e-41], F)
    want = {8: [0, 255, 0, 255, 128, 128], 4: [0, 15, 0, 15, 8, 8], 16: [0x7e00, 0x7c00, 0xfc00, 0x7c00, 0x0000, 0x8000]}[bits]
    rng = np.random.default_rng(bits)
    x = (F(0.3) * rng.standard_normal((50, dim), dtype=F)).astype(F)
    x[:len(vals), 3] = vals
    x[:len(vals), dim - 1] = vals[::-1]
    cent = np.zeros((2, dim), F)
    lo, hi = np.full(dim, VMIN, F), np.full(dim, VMAX, F)
    ix = capi.SqIndex(L2, dim, sqb.params(bits))
    ix.set_codebook(cent, lo, hi)
    ix.add(x)
    ix.build()
    _, _, _, off, codes, labels = ix.export()
    assert off.tolist() == [0, 50, 50], "zero centroids: every score is 0, NaN or inf -> list 0"
    assert (labels == np.arange(50)).all()
    assert [int(c) for c in codes[:len(vals), 3]] == want and [int(c) for c in codes[:len(vals), dim - 1]] == want[::-1]
    assert codes.tobytes() == sq_encode(x, cent[:1], lo, hi, bits).tobytes()
    ix.close()


@gpu
@pytest.mark.parametrize("form", [("sq", 16, 0), ("sq", 4, 0), ("pq", 8, 1)], ids=["sq16", "sq4", "pq8qt"])
@pytest.mark.parametrize("metric", METRICS)
def test_extreme_rows_fed_in_a_chunk_of_their_own(metric, form):
    """Ordinary rows first, then every extreme row in one last add, labels travelling with their rows: the same index, byte for byte."""
    _, x, kind_of, _, q, _, _, _ = fed(metric, "extreme")
    _, ref = case(form, metric, "extreme")
    special = np.array(sorted(kind_of))
    order = np.concatenate([np.setdiff1d(np.arange(len(x)), special), special])
    n0 = len(x) - len(special)
    ix, exp = build(form, metric, "extreme", order=order, chunks=((0, n0), (n0, None)))
    for got, want in zip(exp, ref.exp):
        assert got.tobytes() == want.tobytes()
    same(*ix.search(q, ROWS_K, "nprobe=%d" % NPROBE), *ref.search(q, NPROBE, ROWS_K, tag="all"))
    ix.close()


# ---------------------------------------------------------------------------------------- 2. search, host and device entry

@gpu
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("metric", METRICS)
def test_search_over_special_rows(metric, level, form):
    ix, ref = case(form, metric, level)
    q = fed(metric, level)[4]
    for nprobe in (NPROBE, ROWS_NLIST):
        want = ref.search(q, nprobe, ROWS_K, tag="all")
        same(*ix.search(q, ROWS_K, "nprobe=%d" % nprobe), *want, "host entry, nprobe %d:" % nprobe)
        same(*device_search(ix, q, ROWS_K, nprobe), *want, "device entry, nprobe %d:" % nprobe)


# ---------------------------------------------------------------------------------------- 3. rank rounds

@gpu
@pytest.mark.parametrize("form,metric", [(("sq", 16, 0), L2), (("sq", 16, 0), IP), (("sq", 16, 0), COS), (("pq", 8, 1), IP)],
                         ids=["sq16-l2", "sq16-ip", "sq16-cosine", "pq8qt-ip"])
def test_rank_rounds_over_special_rows(form, metric):
    """k = 600: three rounds, each behind the last (distance, label) of the one before; under inner product at 16 bits the signed
    queries' first ranks score +inf and other rows NaN."""
    ix, ref = case(form, metric, "extreme")
    q = fed(metric, "extreme")[4]
    ids, dis = ix.search_rounds(q, 600, "nprobe=%d" % ROWS_NLIST)
    same(ids, dis, *ref.search(q, ROWS_NLIST, 600, tag="all"))
    i256, d256 = ix.search(q, 256, "nprobe=%d" % ROWS_NLIST)
    same(ids[:, :256], dis[:, :256], i256, d256, "the first round against search(k = 256):")
    for row in ids:
        filled = row[row >= 0]
        assert len(set(filled.tolist())) == len(filled), "a label returned twice"
        assert (row[len(filled):] == -1).all()


# ---------------------------------------------------------------------------------------- 4. filter

@gpu
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_filter_over_special_rows(metric):
    form = ("sq", 16, 0)
    ix, ref = case(form, metric, "extreme")
    _, x, kind_of, labels, q, _, _, _ = fed(metric, "extreme")
    top = int(labels.max()) + 1
    special = labels[sorted(kind_of)]
    without = np.ones(top, bool)
    without[special] = False
    only = ~without
    for name, alive in (("without the special rows", without), ("the special rows alone", only)):
        want = ref.search(q, ROWS_NLIST, ROWS_K, alive=alive, tag="all")
        same(*ix.search(q, ROWS_K, "nprobe=%d" % ROWS_NLIST, alive=alive), *want, name + ", host entry:")
        same(*device_search(ix, q, ROWS_K, ROWS_NLIST, alive=alive), *want, name + ", device entry:")
    assert not np.isin(ref.search(q, ROWS_NLIST, ROWS_K, alive=without, tag="all")[0], special).any()
    nbits = top // 2  # a bitmap shorter than the label space: labels at or beyond nbits are dead
    cut = np.ones(top, bool)
    cut[nbits:] = False
    got = ix.search(q, ROWS_K, "nprobe=%d" % NPROBE, alive=np.ones(nbits, bool), nbits=nbits)
    same(*got, *ref.search(q, NPROBE, ROWS_K, alive=cut, tag="all"), "short bitmap:")
    assert (got[0] < nbits).all()


# ---------------------------------------------------------------------------------------- 5. two-stage search

@gpu
@pytest.mark.parametrize("form", [("sq", 16, 0), ("pq", 4, 0)], ids=["sq16", "pq4"])
@pytest.mark.parametrize("metric", METRICS)
def test_refine_over_special_rows(metric, form):
    """labels = positions, the row store's rule.  search_refine is capi.refine of search's candidates, and both are the reference: the
    exact top-k among the first stage's candidates, strictly better than the neutral value, NaN never."""
    _, x, _, _, q, _, _, _ = fed(metric, "extreme")
    ix, _ = build(form, metric, "extreme", labelled=False)
    rows = store_of(x, metric)
    for kc, first, two_stage in ((64, ix.search, ix.search_refine), (300, ix.search_rounds, ix.search_refine_rounds)):
        cand = first(q, kc, "nprobe=%d" % NPROBE)[0]
        got = two_stage(rows, q, 10, kc, "nprobe=%d" % NPROBE)
        same(*got, *capi.refine(rows, metric, q, cand, 10), "kc %d, against refine of search:" % kc)
        same(*got, *ref_refine(x, q, cand, 10, metric), "kc %d, against the reference:" % kc)
    ix.close()


# ---------------------------------------------------------------------------------------- 6. training on non-finite rows

@gpu
@pytest.mark.parametrize("bad", ["nan", "inf", "both"])
@pytest.mark.parametrize("bits", [8, 4])
def test_pq_training_on_non_finite_rows_is_refused(bits, bad):
    """msvs_pq_index_train over 2000 rows with a NaN and / or an infinite row among them, every row in every trainer's sample
    (train_sample = n): the k-means puts such a row into a list whose mean is then not finite, and train refuses the codebook as set_codebook
    would: MSVS_ERR_INVALID_ARGUMENT, the index left without a codebook (include/msvs.h).  The same rows train once the two are gone."""
    rng = np.random.default_rng(31 + bits)
    n, dim, m = 2000, 20, 4
    _, x = pq.blobs(rng, n, dim, 8)
    x[:, 7] = np.abs(x[:, 7]) + F(1)
    xb = x.copy()
    if bad in ("nan", "both"):
        xb[700, 3] = np.nan
    if bad in ("inf", "both"):
        xb[1300, 7] = np.inf
    ix = capi.PqIndex(L2, dim, "ncentroids=8,kmeans_iters=4,train_sample=%d,m=%d,bit_size=%d" % (n, m, bits))
    with pytest.raises(capi.MsvsError) as e:
        ix.train(xb)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "not finite" in str(e.value)
    with pytest.raises(capi.MsvsError) as e:
        ix.add(x)
    assert e.value.code == capi.ERR_NOT_READY and ix.num_lists == 0
    ix.train(x)
    cent, cb = ix.export(with_lists=False)[:2]
    assert np.isfinite(cent).all() and np.isfinite(cb).all() and cb.shape == (m, 1 << bits, dim // m)
    ix.close()
