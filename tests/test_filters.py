"""The PREWHERE filter path at its edges: predicate constants outside the column type or inexact in it, bitmaps of unequal
length, offsets that repeat or fall outside the bitmap, and the compacted view at its chunk seams and past 1024 chunks.
Every expectation comes from numpy / Python integers or the CPU oracle; bitmaps and ids are compared exactly, distances by
their bits."""
import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
INT_DTYPES = (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64)
FLOAT_DTYPES = (np.float32, np.float64)
CMP = {"==": lambda c, lo, hi: c == lo, "!=": lambda c, lo, hi: c != lo, "<": lambda c, lo, hi: c < lo,
       "<=": lambda c, lo, hi: c <= lo, ">": lambda c, lo, hi: c > lo, ">=": lambda c, lo, hi: c >= lo,
       "between": lambda c, lo, hi: (c >= lo) & (c <= hi)}
SIZES = (1, 63, 64, 65, 1000)

# in range for some type, equal to a type's min / max, and one past each
INT_CONSTANTS = (0, 1, 3, 40, 44, 300, -1, 127, 128, -128, -129, 255, 256, 32767, 32768, -32768, -32769, 65535, 65536,
                 2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62, -2 ** 62, I64_MIN, I64_MAX)
# one or both ends out of range of the narrow types, lo > hi, entirely negative, entirely above 32 bits
INT_RANGES = ((-1, 300), (-129, 40), (3, 65536), (-2 ** 31 - 1, 2 ** 32), (I64_MIN, I64_MAX), (40, 3), (256, -1), (0, 255),
              (2 ** 32, 2 ** 32 + 5), (-5, -1), (I64_MIN, -1), (2 ** 62, I64_MAX), (-32769, 32768), (3, 40))
FLOAT_CONSTANTS = (0.1, 0.3, -0.1, 16777217.0, 1e39, -1e39, float("inf"), float("-inf"))
FLOAT_RANGES = ((0.1, 0.3), (-0.1, 0.1), (0.3, 0.1), (-1e39, 1e39), (float("-inf"), float("inf")), (0.1, 16777217.0),
                (1e39, float("inf")), (16777217.0, 1e39))


def int_column(dt, n):
    """Random values over the whole type with its corners planted: min, max, 0, +-1, every constant that fits, and for the
    64-bit types values around +-2^62 and (unsigned) at and above 2^63."""
    info = np.iinfo(dt)
    rng = np.random.default_rng(n * 31 + np.dtype(dt).num)
    special = [info.min, info.max, 0, 1, -1, info.min + 1, info.max - 1, 2 ** 62 - 1, 2 ** 62 + 1, -2 ** 62 - 1, -2 ** 62 + 1,
               2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2] + list(INT_CONSTANTS)
    special = list(dict.fromkeys(v for v in special if info.min <= v <= info.max))[:n]
    col = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    col[rng.permutation(n)[:len(special)]] = np.array(special, dtype=dt)
    return col


def float_column(dt, n):
    """Every constant rounded to float32 with its float32 neighbours on both sides (for Float64 also the constant itself and
    its float64 neighbours), NaN, +-inf, +-0.0, +-FLT_MAX; the rest random."""
    rng = np.random.default_rng(n * 37 + np.dtype(dt).num)
    special = []
    with np.errstate(over="ignore"):
        for c in FLOAT_CONSTANTS:
            f = np.float32(c)
            special += [f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))]
            if dt is np.float64:
                special += [np.float64(c), np.nextafter(np.float64(c), -np.inf), np.nextafter(np.float64(c), np.inf)]
    fmax = np.finfo(np.float32).max
    special += [np.nan, np.inf, -np.inf, 0.0, -0.0, fmax, -fmax]
    special = special[:n]
    col = (rng.standard_normal(n) * 50).astype(dt)
    col[rng.permutation(n)[:len(special)]] = np.array(special, dtype=np.float64).astype(dt)
    return col


def predicate_cases(dt):
    consts, ranges = (FLOAT_CONSTANTS, FLOAT_RANGES) if np.dtype(dt).kind == "f" else (INT_CONSTANTS, INT_RANGES)
    return [(op, c, 0) for c in consts for op in CMP if op != "between"] + [("between", lo, hi) for lo, hi in ranges]


def by_value(col):
    """The column as the values it holds: Python integers (exact whatever the constant), or doubles."""
    return col.astype(np.float64) if col.dtype.kind == "f" else col.astype(object)


def predicate_reference(values, op, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.asarray(CMP[op](values, lo, hi), dtype=bool)


def check_predicates(col, cases, make):
    values, bad = by_value(col), []
    for op, lo, hi in cases:
        want = predicate_reference(values, op, lo, hi)
        f = make(op, lo, hi)
        got, cnt = f.to_bool(), f.count()
        f.close()
        if not (np.array_equal(got, want) and cnt == (int(want.sum()), col.size)):
            bad.append("%s %r%s: %d rows differ" % (op, lo, " .. %r" % (hi,) if op == "between" else "",
                                                    int((got != want).sum()) if got.shape == want.shape else -1))
    assert not bad, "%s, n = %d: %d of %d predicates wrong:\n  %s" % (col.dtype, col.size, len(bad), len(cases), "\n  ".join(bad))


def on_device(a):
    """The bytes of a numpy array in device memory (a torch tensor: keep it alive while its data_ptr() is in use)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------- 1. predicate constants, by value

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dt", INT_DTYPES + FLOAT_DTYPES, ids=lambda t: np.dtype(t).name)
def test_predicate_compares_by_value(dt, n):
    """`column OP constant` means what it means in SQL: the VALUES are compared.  A constant outside the column type is not
    cast into it (UInt8 < 300 is true for every row, x > -1 for every unsigned row, x == 256 for none), a UInt64 value at or above
    2^63 is above every int64 constant, and a Float32 column is compared with the double constant in double (float32(0.1) <=
    0.1 is false).  NaN fails everything but !=."""
    col = int_column(dt, n) if np.dtype(dt).kind != "f" else float_column(dt, n)
    check_predicates(col, predicate_cases(dt), lambda op, lo, hi: capi.Filter.from_predicate(col, op, lo, hi))


@pytest.mark.parametrize("dt", INT_DTYPES + FLOAT_DTYPES, ids=lambda t: np.dtype(t).name)
def test_predicate_on_a_device_column(dt):
    """The MSVS_MEM_DEVICE branch of msvs_filter_from_predicate: the column is read where it lies."""
    n = 1000
    if np.dtype(dt).kind == "f":
        col, cases = float_column(dt, n), [("<=", 0.1, 0), ("!=", 0.3, 0), ("between", -0.1, 0.3), (">", -1e39, 0)]
    else:
        col, cases = int_column(dt, n), [(">", -1, 0), ("<", 300, 0), ("==", 256, 0), ("between", -129, 65536), (">=", I64_MIN, 0)]
    t = on_device(col)
    check_predicates(col, cases, lambda op, lo, hi: capi.Filter.from_predicate((col.dtype, n), op, lo, hi, device_ptr=t.data_ptr()))


def test_predicate_constant_outside_int64_is_an_error():
    """msvs_scalar_t carries an int64: a constant it cannot hold must not wrap."""
    for dt in (np.uint8, np.uint64, np.int64):
        col = np.arange(5).astype(dt)
        for lo, hi in ((2 ** 63, 0), (I64_MIN - 1, 0), (0, 2 ** 64), (2 ** 64 + 3, 2 ** 64 + 4)):
            with pytest.raises(ValueError):
                capi.Filter.from_predicate(col, "between", lo, hi)
    f = capi.Filter.from_predicate(np.arange(5).astype(np.uint64), "<=", I64_MAX)  # the ends themselves fit
    assert f.count() == (5, 5)
    f.close()


# ---------------------------------------------------------------------------------------- 2. unequal lengths

def extended(b, n):
    """b zero-extended or truncated to n bits."""
    out = np.zeros(n, bool)
    m = min(n, len(b))
    out[:m] = b[:m]
    return out


MODES = {capi.FILTER_AND: lambda a, b: a & b, capi.FILTER_OR: lambda a, b: a | b, capi.FILTER_AND_NOT: lambda a, b: a & ~b}
LENGTH_PAIRS = ((1000, 64), (1000, 65), (1000, 1), (64, 1000), (65, 1000), (130, 129), (1, 1))


@pytest.mark.parametrize("mode", sorted(MODES), ids=("and", "or", "and_not"))
@pytest.mark.parametrize("la,lb", LENGTH_PAIRS)
def test_combine_of_unequal_lengths(la, lb, mode):
    """a.combine(b): b counts as zero past its end and is ignored past a's; the result keeps a's length."""
    rng = np.random.default_rng(la * 1009 + lb)
    for a in (rng.random(la) < 0.5, np.ones(la, bool), np.zeros(la, bool)):
        for b in (rng.random(lb) < 0.5, np.ones(lb, bool)):
            want = MODES[mode](a, extended(b, la))
            f = capi.Filter.from_bool(a).combine(capi.Filter.from_bool(b), mode)
            assert f.to_bool().tolist() == want.tolist()
            assert f.count() == (int(want.sum()), la)


@pytest.mark.parametrize("mode", sorted(MODES), ids=("and", "or", "and_not"))
def test_combine_ignores_what_an_earlier_combine_left_past_the_end(mode):
    """OR with a longer bitmap must leave nothing behind past the shorter one's last bit: the short filter is combined into a
    long one afterwards, where those bits would be rows."""
    short = capi.Filter.from_bool(np.zeros(65, bool)).combine(capi.Filter.from_bool(np.ones(1000, bool)), capi.FILTER_OR)
    assert short.count() == (65, 65) and short.to_bool().all()
    a = np.arange(1000) % 3 == 0
    want = MODES[mode](a, extended(np.ones(65, bool), 1000))
    f = capi.Filter.from_bool(a).combine(short, mode)
    assert f.to_bool().tolist() == want.tolist()
    assert f.count() == (int(want.sum()), 1000)


N_SMALL, D_SMALL = 300, 8


@pytest.fixture(scope="module")
def small_flat():
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N_SMALL, D_SMALL), dtype=np.float32)
    # queries next to rows 200.. and 290..: a row past the filter's end that leaks through shows up first in the result
    q = (np.concatenate([x[200:204], x[290:294], x[:2]]) + np.float32(0.01) * rng.standard_normal((10, D_SMALL), dtype=np.float32))
    ix = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, D_SMALL)
    ix.add(x)
    ix.build()
    yield ix, x, q.astype(np.float32)
    ix.close()


def same(a_ids, a_dis, b_ids, b_dis):
    assert a_ids.shape == b_ids.shape
    assert (a_ids == b_ids).all(), np.argwhere(a_ids != b_ids)[:5]
    assert (a_dis.view(np.uint32) == b_dis.view(np.uint32)).all()


@pytest.mark.parametrize("k", (300, 10))  # 300: exact rounds over the bit test; 10: one pass, view or bit test
def test_search_never_sees_rows_past_the_filters_end(small_flat, k, opt):
    """200 bits OR-ed with 300 ones are 200 ones: rows 200.. stay dead whichever strategy reads the bitmap."""
    ix, x, q = small_flat
    rng = np.random.default_rng(5)
    for first in (np.zeros(200, bool), rng.random(200) < 0.5):
        flt = capi.Filter.from_bool(first).combine(capi.Filter.from_bool(np.ones(300, bool)), capi.FILTER_OR)
        assert flt.count() == (200, 200)
        oi, od = o.knn(q, x, k, o.METRIC_L2, alive=np.arange(N_SMALL) < 200)
        for below in ("1", "0"):
            opt("filter_compact_below", below)
            ids, dis = ix.search_filter(q, k, "", flt)
            assert ids.max() < 200
            same(ids, dis, oi, od)
        flt.close()


@pytest.mark.parametrize("k", (300, 10))
def test_filter_longer_than_the_index(small_flat, k, opt):
    """400 ones over 300 rows: the unfiltered result (the view's row map holds 300 rows, not 400)."""
    ix, x, q = small_flat
    flt = capi.Filter.from_bool(np.ones(400, bool))
    oi, od = o.knn(q, x, k, o.METRIC_L2)
    for below in ("1", "0"):
        opt("filter_compact_below", below)
        ids, dis = ix.search_filter(q, k, "", flt)
        same(ids, dis, oi, od)
    flt.close()


@pytest.mark.parametrize("filter_bits", (200, 300, 364))
@pytest.mark.parametrize("delete_bits", (150, 300, 364))
def test_delete_bitmap_and_filter_of_different_lengths(small_flat, delete_bits, filter_bits, opt):
    """A row is returned when its bit is set in the delete bitmap AND in the per-call filter, inside both lengths."""
    ix, x, q = small_flat
    rng = np.random.default_rng(delete_bits * 7 + filter_bits)
    for density in (0.6, 1.0):
        kept = rng.random(delete_bits) < density
        passing = rng.random(filter_bits) < density
        alive = extended(kept, N_SMALL) & extended(passing, N_SMALL)
        flt = capi.Filter.from_bool(passing)
        ix.set_delete_bitmap(kept)
        try:
            for k in (300, 10):
                oi, od = o.knn(q, x, k, o.METRIC_L2, alive=alive)
                for below in ("1", "0"):
                    opt("filter_compact_below", below)
                    ids, dis = ix.search_filter(q, k, "", flt)
                    same(ids, dis, oi, od)
                    same(*ix.search(q, k, "", alive=passing), oi, od)
                    if k == 300:
                        assert sorted(ids[0][ids[0] >= 0].tolist()) == np.flatnonzero(alive).tolist()
        finally:
            ix.set_delete_bitmap(None)
            flt.close()


# ---------------------------------------------------------------------------------------- 3. offsets

def offset_cases(nbits):
    rng = np.random.default_rng(nbits)
    mixed = np.concatenate([rng.integers(0, nbits, 3 * nbits // 2 + 3),  # more draws than bits: duplicates, unsorted
                            [nbits, nbits + 63, 2 ** 40, 0, nbits - 1, nbits - 1, nbits]]).astype(np.uint64)
    return [np.zeros(0, np.uint64), rng.permutation(mixed), np.array([nbits, nbits + 63, 2 ** 40], np.uint64)]


@pytest.mark.parametrize("where", ("host", "device"))
@pytest.mark.parametrize("nbits", (1, 64, 65, 1000))
def test_offsets_with_duplicates_and_out_of_range(nbits, where):
    """getFilterFromPipeline's scatter: an offset sets its bit however often and in whatever order it comes; offsets at or
    past nbits set nothing and touch nothing.  From host memory and from device memory."""
    for off in offset_cases(nbits):
        want = np.zeros(nbits, bool)
        want[off[off < nbits].astype(np.int64)] = True
        if where == "host":
            f = capi.Filter.from_offsets(off, nbits)
        else:
            t = on_device(off)
            f = capi.Filter.from_offsets(off.size, nbits, device_ptr=t.data_ptr())
        assert f.to_bool().tolist() == want.tolist()
        assert f.count() == (int(want.sum()), nbits)
        f.close()


# ---------------------------------------------------------------------------------------- 4. the compacted view at its seams

NLIST = 8


def seam_index(kind, n, permuted):
    """-> (index, oracle(q, k, alive by label), labels in storage order, list offsets or None).  IVF: eight far-apart centroids,
    lists 0 and 4 stay empty, every row sits next to the centroid of its list."""
    rng = np.random.default_rng(n * 3 + permuted)
    labels = rng.permutation(n).astype(np.int64) if permuted else None
    if kind == "flat":
        x = rng.standard_normal((n, D_SMALL), dtype=np.float32)
        ix = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, D_SMALL)
        ix.add(x, labels)
        ix.build()
        stored = labels if permuted else np.arange(n, dtype=np.int64)

        def oracle(q, k, alive):
            return o.knn(q, x, k, o.METRIC_L2, labels=labels, alive=alive[stored])
        return ix, oracle, stored, None, x
    cent = (np.eye(NLIST, D_SMALL) * 10).astype(np.float32)
    lists = rng.choice([1, 2, 3, 5, 6, 7], n)
    x = (cent[lists] + np.float32(0.1) * rng.standard_normal((n, D_SMALL), dtype=np.float32)).astype(np.float32)
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, D_SMALL, "ncentroids=%d" % NLIST)
    ix.set_centroids(cent)
    ix.add(x, labels)
    ix.build()
    c, off, vecs, stored = ix.export()
    assert off[1] == 0 and off[4] == off[5] and off[-1] == n  # lists 0 and 4 are empty
    assert sorted(stored.tolist()) == list(range(n))

    def oracle(q, k, alive):
        return o.ivf_search(c, off, vecs, stored, q, NLIST, k, o.METRIC_L2, alive=alive)[:2]
    return ix, oracle, stored, off, x


@pytest.mark.parametrize("n", (1, 2047, 2048, 2049, 4097))
@pytest.mark.parametrize("kind,permuted", (("flat", False), ("flat", True), ("ivf", False), ("ivf", True)),
                         ids=("flat", "flat-labels", "ivf", "ivf-labels"))
def test_compacted_view_at_chunk_seams(kind, permuted, n, opt):
    """The view (filter_compact_below = 1) against the bit test (0) and the oracle, for filters whose passing rows sit on the
    ends of the 2048-row chunks of the three compaction passes IN STORAGE ORDER: nothing, everything, the last stored row
    alone, the first alone, stored rows 2047 and 2048; IVF lists that are empty, pass nothing and pass everything."""
    ix, oracle, stored, off, x = seam_index(kind, n, permuted)
    rng = np.random.default_rng(n)
    q = np.concatenate([x[[0, n - 1, n // 2]], rng.standard_normal((3, D_SMALL), dtype=np.float32)]).astype(np.float32)
    rows = {"none": [], "all": list(range(n)), "last": [n - 1], "first": [0], "seam": [r for r in (2047, 2048) if r < n],
            "seam+ends": [r for r in (0, 2047, 2048, 4095, 4096) if r < n]}
    if off is not None:
        rows["lists 2 and 5"] = list(range(off[2], off[3])) + list(range(off[5], off[6]))  # 0, 4 empty; the others pass nothing
        rows["all but list 3"] = list(range(0, off[3])) + list(range(off[4], n))
    params = "nprobe=%d" % NLIST if kind == "ivf" else ""
    for name, r in rows.items():
        alive = np.zeros(n, bool)  # by label
        alive[stored[np.array(r, dtype=np.int64)]] = True
        flt = capi.Filter.from_bool(alive)
        for k in (10, 1):
            oi, od = oracle(q, k, alive)
            assert set(oi[oi >= 0].tolist()) <= set(np.flatnonzero(alive).tolist()), name
            for below in ("1", "0"):
                opt("filter_compact_below", below)
                ids, dis = ix.search_filter(q, k, params, flt)
                assert (ids == oi).all(), (name, below, k, ids[:2], oi[:2])
                assert (dis.view(np.uint32) == od.view(np.uint32)).all(), (name, below, k)
        flt.close()
    ix.close()


def test_compacted_view_past_1024_chunks(opt):
    """2.2M stored rows are 1075 chunks: the one-block scan of the chunk counts runs a second round and carries the total of
    the first 1024 chunks into it.  A wrong carry moves every view row of chunks 1024.. -- three queries are copies of passing
    rows up there.  The oracle sees the passing rows only."""
    n, d, k = 2_200_000, 4, 10
    rng = np.random.default_rng(2200)
    x = rng.standard_normal((n, d), dtype=np.float32)
    alive = np.zeros(n, bool)
    alive[::5000] = True
    alive[-300:] = True
    passing = np.flatnonzero(alive)
    q = rng.standard_normal((8, d), dtype=np.float32)
    q[5], q[6], q[7] = x[2_100_000], x[2_150_000], x[n - 1]
    assert alive[[2_100_000, 2_150_000, n - 1]].all() and 2_100_000 > 1024 * 2048
    oi, od = o.knn(q, x[passing], k, o.METRIC_L2, labels=passing.astype(np.int64))
    assert oi[5, 0] == 2_100_000 and oi[6, 0] == 2_150_000 and oi[7, 0] == n - 1
    ix = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, d)
    ix.add(x)
    ix.build()
    flt = capi.Filter.from_bool(alive)
    assert flt.count() == (passing.size, n)
    for below in ("1", "0"):
        opt("filter_compact_below", below)
        ids, dis = ix.search_filter(q, k, "", flt)
        same(ids, dis, oi, od)
    flt.close()
    ix.close()
