"""The IVFSQ candidate search (sq_cand_kernels.hpp, sq_candidates.hip) at the edges its own test file does not reach: the tile of 16
queries, selection buffers filled to their capacity, a second and a third pass of search_device's query loop, query values that break
the image's quantiser, short filter bitmaps, special stored rows and an empty probed list.

Part 1 of every section restates the switch in Python -- constants read from the headers -- and asserts, without a GPU, that each case
is in the state it was written for; a case that stays on the common path fails there.  Part 2 (marked gpu) runs the cases: ids == and
distances by their uint32 view against test_sq_candidates.ref_candidates, no tolerance anywhere."""
import functools
import os
import re

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_batch_chunks as tb
import test_sq_ivf as sq
from oracle import oracle as o
from test_large_dims import CSRC, MAX_DIM, ceil_div, header_const, round_up, sq_fits
from test_sq_candidates import COS, F, IP, L2, NLIST, SIZES, case, device_candidates, ref_candidates, ref_scores, same

gpu = pytest.mark.gpu
NAME = {L2: "l2", IP: "ip", COS: "cosine"}
METRICS = [pytest.param(m, id=NAME[m]) for m in (L2, IP, COS)]
MAX_K = capi.MAX_K
SQC_GROUP = header_const("sq_cand_kernels.hpp", "SQC_GROUP")
SQC_LDS_MAX = header_const("sq_cand_kernels.hpp", "SQC_LDS_MAX")
INT32_MAX = 2 ** 31 - 1


def float_const(header, name):
    """`constexpr float NAME = <integer>.f;` of a header of the library"""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+float\s+%s\s*=\s*([0-9]+)\.f;" % name, f.read())
    assert m, "%s: no constant %s" % (header, name)
    return int(m.group(1))


SQC_WMAX = float_const("sq_cand_kernels.hpp", "SQC_WMAX")


# ======================================================================================== the planners, restated

def sq_ld(dim):
    return round_up(dim, 16)


def sqc_record_bytes(ld):
    return 2 * ld + 16


def sqc_cap(kc):
    return (kc + SQC_GROUP + 63) // 64 * 64


def sqc_lds_bytes(TQ, ld, kc):
    return TQ * (sqc_record_bytes(ld) + sqc_cap(kc) * 8 + 24)


def sq_cand_tile(ld, kc):
    return 32 if sqc_lds_bytes(32, ld, kc) <= SQC_LDS_MAX else 16


def plan_segments(max_list_len, knob, row_step, P, k, fixed_per_q, nq):
    """device_ops.hpp -> (rpb, seg_max, per_q, chunk)"""
    want = int(knob) if knob >= 1 else max(2048, ceil_div(max_list_len, 8))
    rpb = min(round_up(want, row_step), 0x40000000)
    seg_max = max(1, ceil_div(max_list_len, rpb))
    per_q = P * seg_max * k * 8 + fixed_per_q
    return rpb, seg_max, per_q, max(1, min(nq, (256 << 20) // per_q, 0x7fffffff // (P * seg_max)))


def cand_fixed_per_q(ld, P, kc):
    """search_device's fixed_per_q as sq_candidates_device calls it: the padded row, probes and pairs, 64, the query's record, the
    probes' distances and the merged keys handed to the re-rank"""
    return ld * 4 + P * 8 + 64 + sqc_record_bytes(ld) + P * 4 + kc * 8


def image_of(x, step):
    """sq_query_image_kernel's quantiser -> (delta, w)"""
    with np.errstate(all="ignore"):
        u = (x * step).astype(F)
        delta = F(np.abs(u).max()) / F(SQC_WMAX)
        if not (np.isfinite(delta) and delta > 0):
            return F(0), np.zeros(len(u), np.int64)
        return delta, np.clip(np.rint((u / delta).astype(F)), -SQC_WMAX, SQC_WMAX).astype(np.int64)


def scored(q, metric):
    with np.errstate(all="ignore"):
        return o.normalize_rows(q) if metric == COS else np.ascontiguousarray(q, F)


def side_candidates(ix, q, k, kc, nprobe):
    """the device entry with the queries computed on a stream that is not the current one, outputs pre-filled with -7 / NaN"""
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).cuda()
    di = torch.full((len(q), k), -7, device="cuda", dtype=torch.int64)
    dd = torch.full((len(q), k), float("nan"), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    s = tb.side_stream()
    with torch.cuda.stream(s):
        q2 = dq * 1
        ix.search_candidates_device(q2.data_ptr(), len(q), k, kc, nprobe, di.data_ptr(), dd.data_ptr(), s.cuda_stream)
    s.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


def first(ref, nq, k):
    """the reference of the first nq queries at a smaller k: every query's list is a prefix of its longer one"""
    return ref[0][:nq, :k], ref[1][:nq, :k]


# ======================================================================================== A1. the tile of 16 queries

DIM_MAX = max(d for d in range(1, MAX_DIM + 1) if sq_fits(d))                                       # the largest dim the index admits
D256 = min(d for d in range(1, DIM_MAX + 1) if sq_cand_tile(sq_ld(d), MAX_K) == 16)                 # the first dim of tile 16 at kc = 256
DANY = min(d for d in range(1, DIM_MAX + 1) if all(sq_cand_tile(sq_ld(d), kc) == 16 for kc in range(1, MAX_K + 1)))  # ... at any kc
# (metric, dim, kc): just above the kc = 256 switch under every metric, just above the any-kc switch at kc = 32, the largest dim; and
# the last dim below each switch, which keeps the tile of 32
TILE = [(L2, D256, 256), (IP, D256, 256), (COS, D256, 256), (IP, DANY, 32), (L2, DIM_MAX, 256), (L2, D256 - 1, 256), (COS, DANY - 1, 32)]
TILE_IDS = ["%s-d%d-kc%d" % (NAME[m], d, kc) for m, d, kc in TILE]
NQS = [1, 15, 16, 17, 33, 70]


def test_tile_table_reaches_both_tiles():
    assert sqc_cap(MAX_K) == 6 * 64, "sqc_compact ranks six keys a lane"
    assert not sq_fits(DIM_MAX + 1) and sq_ld(DIM_MAX) == DIM_MAX
    assert sq_ld(D256) > 1004 >= sq_ld(D256 - 1) and sq_ld(DANY) > 1772 >= sq_ld(DANY - 1)
    tiles = [sq_cand_tile(sq_ld(d), kc) for _, d, kc in TILE]
    assert tiles == [16, 16, 16, 16, 16, 32, 32]
    assert sq_cand_tile(sq_ld(D256), 32) == 32, "at kc = 32 the first dim of the kc = 256 switch is still a tile of 32"
    assert sq_cand_tile(sq_ld(DANY), 1) == 16
    assert DIM_MAX in [d for _, d, _ in TILE]
    assert sqc_lds_bytes(16, sq_ld(DIM_MAX), MAX_K) <= SQC_LDS_MAX, "the largest case fits 16 queries at kc = 256"
    assert {m for m, d, kc in TILE if sq_cand_tile(sq_ld(d), kc) == 16} == {L2, IP, COS}
    # 70 queries on every list: several tiles a list, the last one partial; 15, 17 and 33 leave partial tiles of either width
    assert max(NQS) > 2 * 32 and {nq % 16 != 0 for nq in NQS} == {True, False}


@gpu
@pytest.mark.parametrize("metric,dim,kc", TILE, ids=TILE_IDS)
def test_tile_of_sixteen(metric, dim, kc, opt):
    """Every nq through the host entry (k = 10) and the device entry (k = kc), about half of the labels filtered, and the lists cut
    into segments of 32 rows; after every search the launch counter tells which instantiation ran."""
    ix, exp, q, labels = case(metric, dim)
    tile = sq_cand_tile(sq_ld(dim), kc)
    want = (1, 0) if tile == 32 else (0, 1)
    alive = np.random.default_rng(5).random(3 * len(labels)) < 0.5
    ref, ref_alive = ref_candidates(exp, q, kc, kc, NLIST, metric), ref_candidates(exp, q, kc, kc, NLIST, metric, alive)
    capi.debug_sq_cand_tiles()
    for nq in NQS:
        same(ix.search_candidates(q[:nq], 10, kc, "nprobe=%d" % NLIST), first(ref, nq, 10))
        assert capi.debug_sq_cand_tiles() == want, "nq %d, host entry: not the tile of %d" % (nq, tile)
        same(device_candidates(ix, q[:nq], kc, kc, NLIST), first(ref, nq, kc))
        assert capi.debug_sq_cand_tiles() == want, "nq %d, device entry: not the tile of %d" % (nq, tile)
    for nq in (17, 70):
        same(ix.search_candidates(q[:nq], 10, kc, "nprobe=%d" % NLIST, alive=alive), first(ref_alive, nq, 10))
        assert capi.debug_sq_cand_tiles() == want
    opt("sq_ivf_rpb", "32")
    for nq in (33, 70):
        same(ix.search_candidates(q[:nq], kc, kc, "nprobe=%d" % NLIST), first(ref, nq, kc))
        same(ix.search_candidates(q[:nq], 10, kc, "nprobe=%d" % NLIST, alive=alive), first(ref_alive, nq, 10))
        assert capi.debug_sq_cand_tiles() == tuple(2 * t for t in want)


# ======================================================================================== A2. full selection buffers

FULL_SIZES, FULL_DIM = [1000, 1, 129, 384], 16
FULL_KC = [193, 256]
ORDERS = ["ascending", "descending", "shuffled"]


@functools.lru_cache(maxsize=None)
def full_case(metric, order):
    """-> (centroids, vmin, vmax, rows as fed, the export they must give, 4 queries, a filter): lists of FULL_SIZES rows, labels =
    stored positions.  The long list's rows are placed by the score the definition gives them for query 0: worst first (every group
    of 128 better than all before it), best first, or shuffled."""
    rng = np.random.default_rng(40 + metric)
    dim, scale = FULL_DIM, F(1) if metric == COS else F(10)
    cent = np.zeros((len(FULL_SIZES), dim), F)
    for l in range(len(FULL_SIZES)):
        cent[l, l] = scale
    home = np.repeat(np.arange(len(FULL_SIZES)), FULL_SIZES)
    x = (F(10) / scale * cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    lo, hi = np.full(dim, -0.2 * scale, F), np.full(dim, 0.2 * scale, F)
    q = (F(10) / scale * cent[[0, 0, 2, 3]] + F(0.5) * rng.standard_normal((4, dim), dtype=F)).astype(F)
    q[1] = (q[0] + F(0.01) * rng.standard_normal(dim, dtype=F)).astype(F)

    def export_of(rows):
        off = np.zeros(len(FULL_SIZES) + 1, np.int64)
        np.cumsum(FULL_SIZES, out=off[1:])
        return cent, lo, hi, off, sq.encode(sq.stored(rows, metric), cent[home], lo, hi), np.arange(len(rows), dtype=np.int64)

    _, pos, worse, _ = ref_scores(export_of(x), q[:1], len(FULL_SIZES), metric)[1][0]
    by_pos = np.empty(len(x), F)
    by_pos[pos] = worse
    best_first = np.argsort(by_pos[:FULL_SIZES[0]], kind="stable")
    perm = {"ascending": best_first[::-1], "descending": best_first, "shuffled": rng.permutation(FULL_SIZES[0])}[order]
    x[:FULL_SIZES[0]] = x[perm]
    return cent, lo, hi, x, export_of(x), q, rng.random(len(x)) < 0.5


def buffer_model(worse, alive, kc):
    """sq_cand_scan_kernel's buffer of one query over one work item: worse[r] the scores of the item's rows in stored order ->
    (per group of 128 rows: rows offered, keys appended, the count after them, whether the buffer was cut; the item's kc best keys)"""
    cap, keys, thr, trace = sqc_cap(kc), [], None, []
    for g0 in range(0, len(worse), SQC_GROUP):
        offered = [(float(worse[r]), r) for r in range(g0, min(len(worse), g0 + SQC_GROUP)) if alive[r] and not np.isnan(worse[r])]
        new = [key for key in offered if thr is None or key < thr]
        keys += new
        assert len(keys) <= cap, "the model's buffer overflows: the kernel's would"
        cut = len(keys) + SQC_GROUP > cap
        trace.append((len(offered), len(new), len(keys), cut))
        if cut:
            keys.sort()
            thr = keys[kc - 1] if len(keys) >= kc else thr
            del keys[kc:]
    return trace, sorted(keys)[:kc]


def long_list_model(metric, order, kc, filtered):
    """query 0 over the long list (one work item at the default segment length)"""
    *_, exp, q, alive = full_case(metric, order)
    _, pos, worse, _ = ref_scores(exp, q[:1], len(FULL_SIZES), metric)[1][0]
    by_pos = np.empty(len(pos), F)
    by_pos[pos] = worse
    n = FULL_SIZES[0]
    return buffer_model(by_pos[:n], alive[:n] if filtered else np.ones(n, bool), kc)


@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_buffer_states_of_the_full_cases(metric):
    rpb, seg_max, _, _ = plan_segments(max(FULL_SIZES), 0, 32, len(FULL_SIZES), MAX_K, 0, 4)
    assert rpb >= max(FULL_SIZES) and seg_max == 1, "the long list is one work item at the default segment length"
    sat = []
    for kc in FULL_KC:
        cap = sqc_cap(kc)
        assert cap == 384 and max(FULL_SIZES) > cap and FULL_SIZES[3] == cap and FULL_SIZES[2] == SQC_GROUP + 1
        # ascending: every group appends all its rows, every boundary from the third group on compacts, the last group's rows stay
        trace, keys = long_list_model(metric, "ascending", kc, False)
        assert [t[1] for t in trace] == [t[0] for t in trace] and max(t[2] for t in trace) == cap == 384
        assert sum(t[3] for t in trace) >= 6
        last_group = (FULL_SIZES[0] - 1) // SQC_GROUP * SQC_GROUP
        assert sum(r >= last_group for _, r in keys) == FULL_SIZES[0] - last_group
        *_, exp, q, _ = full_case(metric, "ascending")
        ids = ref_candidates(exp, q[:1], kc, kc, len(FULL_SIZES), metric)[0][0]
        assert ((ids >= last_group) & (ids < FULL_SIZES[0])).sum() == FULL_SIZES[0] - last_group, "the reference's final kc holds the last group"
        # descending: after the first cut the threshold rejects whole groups
        trace, keys = long_list_model(metric, "descending", kc, False)
        first_cut = [t[3] for t in trace].index(True)
        assert all(t[0] == min(SQC_GROUP, FULL_SIZES[0] - SQC_GROUP * i) and t[1] == 0 for i, t in enumerate(trace) if i > first_cut)
        assert len(trace) - first_cut - 1 >= 4 and [r for _, r in keys] == list(range(kc))
        # shuffled: the threshold rejects some keys of a group and admits others
        trace, _ = long_list_model(metric, "shuffled", kc, False)
        assert any(0 < t[1] < t[0] for t in trace[3:])
        for order in ORDERS:  # the filter: irregular counts; a buffer that sat at or below cap - 128 uncut fills beyond it in one group
            trace, _ = long_list_model(metric, order, kc, True)
            assert all(t[0] < SQC_GROUP for t in trace)
            sat += [(order, kc, i) for i in range(1, len(trace))
                    if not trace[i - 1][3] and 0 < trace[i - 1][2] and trace[i][3] and cap - SQC_GROUP < trace[i][2] <= cap and trace[i][2] % 64]
    assert sat, "no filtered case takes a buffer from at most cap - 128 keys to more in one group"
    assert {s[0] for s in sat} >= {"ascending"}


@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_full_buffers(metric, order, opt):
    cent, lo, hi, x, exp, q, alive = full_case(metric, order)
    nlist = len(FULL_SIZES)
    ix = capi.SqIndex(metric, FULL_DIM)
    ix.set_codebook(cent, lo, hi)
    ix.add(x)
    ix.build()
    ix.prepare_candidates()
    try:
        for got, want in zip(ix.export(), exp):
            assert got.tobytes() == want.tobytes(), "the index does not hold the rows where the case put them"
        for rpb in (None, "32"):
            opt("sq_ivf_rpb", rpb)
            for kc in FULL_KC:
                for a in (None, alive):
                    ref = ref_candidates(exp, q, kc, kc, nlist, metric, a)
                    for k in (1, kc):
                        same(ix.search_candidates(q, k, kc, "nprobe=%d" % nlist, alive=a), first(ref, len(q), k))
                same(device_candidates(ix, q, kc, kc, nlist), ref_candidates(exp, q, kc, kc, nlist, metric))
    finally:
        ix.close()


# ======================================================================================== A3. a second and a third round

ROUND_SIZES, ROUND_DIM, ROUND_KC, ROUND_RPB, ROUND_NDIST = [3000, 5, 40, 0, 64, 33, 1, 100], 16, 256, 32, 200
ROUND_CUT = plan_segments(max(ROUND_SIZES), ROUND_RPB, 32, len(ROUND_SIZES), ROUND_KC,
                          cand_fixed_per_q(sq_ld(ROUND_DIM), len(ROUND_SIZES), ROUND_KC), 1 << 30)[3]
ROUND_NQ = 2 * ROUND_CUT + tb.TAIL


def test_rounds_case_takes_three_rounds():
    rpb, seg_max, per_q, cut = plan_segments(max(ROUND_SIZES), ROUND_RPB, 32, len(ROUND_SIZES), ROUND_KC,
                                             cand_fixed_per_q(sq_ld(ROUND_DIM), len(ROUND_SIZES), ROUND_KC), ROUND_NQ)
    assert (rpb, seg_max) == (32, ceil_div(max(ROUND_SIZES), 32)) and cut == ROUND_CUT
    assert 24 <= cut <= 400 and cut == (256 << 20) // per_q, "the 256 MiB of partial lists cut the batch, a few dozen to a few hundred queries"
    assert ROUND_NQ > cut and ceil_div(ROUND_NQ, cut) == 3 and ROUND_NQ % cut == tb.TAIL
    assert sq_cand_tile(sq_ld(ROUND_DIM), ROUND_KC) == 32


@functools.lru_cache(maxsize=None)
def rounds_case(metric):
    """-> (index, distinct queries, pick, reference of the distinct queries at k = kc)"""
    rng = np.random.default_rng(300 + metric)
    dim, scale, nlist = ROUND_DIM, F(1) if metric == COS else F(10), len(ROUND_SIZES)
    cent = np.zeros((nlist, dim), F)
    for l in range(nlist):
        cent[l, l] = scale
    home = np.repeat(np.arange(nlist), ROUND_SIZES)
    x = (F(10) / scale * cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    ix = capi.SqIndex(metric, dim)
    ix.set_codebook(cent, np.full(dim, -0.2 * scale, F), np.full(dim, 0.2 * scale, F))
    ix.add(x, rng.permutation(3 * len(x))[:len(x)].astype(np.int64))
    ix.build()
    ix.prepare_candidates()
    exp = ix.export()
    assert np.diff(exp[3]).tolist() == ROUND_SIZES
    qhome = rng.integers(0, nlist, ROUND_NDIST)
    dq = (F(10) / scale * cent[qhome] + F(0.5) * rng.standard_normal((ROUND_NDIST, dim), dtype=F)).astype(F)
    ref = ref_candidates(exp, dq, ROUND_KC, ROUND_KC, nlist, metric)
    pick = tb.straddle(rng, ROUND_NQ, ROUND_CUT, ROUND_NDIST)
    pick[2 * ROUND_CUT - 2:2 * ROUND_CUT + 3] = (4, 3, 2, 1, 0)  # the second cut as the first
    return ix, dq, pick, ref


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_three_rounds_of_the_query_loop(metric, opt):
    ix, dq, pick, ref = rounds_case(metric)
    nlist = len(ROUND_SIZES)
    q = np.ascontiguousarray(dq[pick])
    opt("sq_ivf_rpb", str(ROUND_RPB))
    with tb.profile() as run:
        for k in (10, ROUND_KC):
            want = first(ref, ROUND_NDIST, k)
            tb.answers_differ(want)
            for entry, fn in (("host", lambda: ix.search_candidates(q, k, ROUND_KC, "nprobe=%d" % nlist)),
                              ("device", lambda: side_candidates(ix, q, k, ROUND_KC, nlist))):
                capi.debug_sq_cand_tiles()
                got, count = run(fn)
                tb.check(got, want, pick, ROUND_CUT, "%s k %d %s entry" % (NAME[metric], k, entry))
                assert (count("sq_cand_scan"), count("sq_cand_rerank")) == (3, 3), "%s entry: not three rounds" % entry
                assert capi.debug_sq_cand_tiles() == (3, 0)
    capi.release_scratch()


# ======================================================================================== A4. query values

VALUE_DIMS = [5, 300]
VALUE_NQ = 40  # a tile of 32 and a partial one
KINDS = {"nan": 2, "+inf": 5, "-inf": 8, "overflow": 11, "zeros": 14, "-zeros": 17, "flush": 20, "subnormal": 23, "dominant": 26, "equal": 29,
         "-equal": 33}


def value_steps(metric, dim):
    """steps that are powers of two (products with them are exact), the last column's 2^9 times the others' and above 1"""
    step = np.full(dim, 2.0 ** -9 if metric == COS else 2.0 ** -6, F)
    step[dim - 1] = 8
    return step


def value_queries(metric, dim, base):
    """the ordinary queries `base` with one special query at every position of KINDS"""
    step = value_steps(metric, dim)
    sign = np.where(np.arange(dim) % 2 == 0, 1, -1).astype(F)
    q = base[:VALUE_NQ].copy()
    q[KINDS["nan"], 1 % dim] = np.nan
    q[KINDS["+inf"], 0] = np.inf
    q[KINDS["-inf"], dim - 2] = -np.inf
    q[KINDS["overflow"], dim - 1] = 1e38               # finite; times the step of 8 it is not
    q[KINDS["zeros"]] = 0
    q[KINDS["-zeros"]] = -0.0
    q[KINDS["flush"]] = F(1e-40) * sign                # |u| ~ 1.6e-42: u / 16256 is below half of the smallest subnormal
    q[KINDS["subnormal"]] = F(3e-37) * sign            # |u| ~ 4.7e-39, subnormal; delta ~ 2.9e-43, subnormal and not 0
    q[KINDS["flush"], dim - 1] = q[KINDS["subnormal"], dim - 1] = 0
    q[KINDS["dominant"], 0] = F(2.0 ** 50) * np.abs(q[KINDS["dominant"]]).max()
    q[KINDS["equal"]] = sign / (step / step[0])        # every |q_j step_j| = step_0
    q[KINDS["-equal"]] = -q[KINDS["equal"]]
    return q


def value_base(metric, dim):
    rng = np.random.default_rng(700 + dim + metric)
    scale = F(1) if metric == COS else F(10)
    cent = np.zeros((NLIST, dim), F)
    for l in range(NLIST):
        cent[l, l % 4] = scale if l < 4 else -scale
    base = (F(10) / scale * cent[rng.integers(0, NLIST, VALUE_NQ)] + F(0.5) * rng.standard_normal((VALUE_NQ, dim), dtype=F)).astype(F)
    return rng, scale, cent, base


@pytest.mark.parametrize("dim", VALUE_DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_value_queries_are_in_their_states(metric, dim):
    _, _, _, base = value_base(metric, dim)
    step = value_steps(metric, dim)
    assert sq.step_of((F(-127.5) * step).astype(F), (F(127.5) * step).astype(F)).tobytes() == step.tobytes()
    q = value_queries(metric, dim, base)
    assert sorted(KINDS.values()) == sorted(set(KINDS.values())) and max(KINDS.values()) < VALUE_NQ
    assert min(KINDS.values()) < 32 <= max(KINDS.values()), "special queries in the full tile and in the partial one"
    assert all(np.isfinite(q[i]).all() and np.abs(q[i]).max() > 0.1 for i in range(VALUE_NQ) if i not in KINDS.values())
    assert np.isfinite(q[KINDS["overflow"]]).all()
    img = {kind: image_of(scored(q[i:i + 1], metric)[0], step) for kind, i in KINDS.items()}
    for kind in ("-equal", "equal"):  # cosine too: the normalisation scales every element alike
        assert (np.abs(img[kind][1]) == SQC_WMAX).all() and img[kind][0] > 0
    assert (img["equal"][1] == -img["-equal"][1]).all() and {int(w) for w in img["equal"][1]} == {-SQC_WMAX, SQC_WMAX}
    for kind in ("nan", "zeros", "-zeros"):
        assert img[kind][0] == 0 and not img[kind][1].any()
    assert np.count_nonzero(img["dominant"][1]) == 1 and abs(img["dominant"][1][0]) == SQC_WMAX
    if metric != COS:  # (the normalisation takes these to NaN rows or to ordinary ones)
        for kind in ("+inf", "-inf", "overflow"):
            assert img[kind][0] == 0 and not img[kind][1].any()
        u = np.abs(q[KINDS["flush"]] * step).max()
        assert 0 < u and img["flush"][0] == 0 and not img["flush"][1].any()
        u = np.abs(q[KINDS["subnormal"]] * step).max()
        # (a subnormal delta has some eight bits: u / delta lands near 16256, not on it)
        assert 0 < img["subnormal"][0] < u < np.finfo(F).tiny and 0.99 * SQC_WMAX < np.abs(img["subnormal"][1]).max() <= SQC_WMAX


@functools.lru_cache(maxsize=None)
def value_case(metric, dim):
    rng, scale, cent, base = value_base(metric, dim)
    step = value_steps(metric, dim)
    home = np.repeat(np.arange(NLIST), SIZES)
    x = (F(10) / scale * cent[home] + F(0.5) * rng.standard_normal((len(home), dim), dtype=F)).astype(F)
    ix = capi.SqIndex(metric, dim)
    ix.set_codebook(cent, (F(-127.5) * step).astype(F), (F(127.5) * step).astype(F))
    ix.add(x, rng.permutation(3 * len(x))[:len(x)].astype(np.int64))
    ix.build()
    ix.prepare_candidates()
    return ix, ix.export(), value_queries(metric, dim, base)


def planes_inside_int32(exp, q, nprobe, metric):
    with np.errstate(all="ignore"):
        for _, _, _, planes in ref_scores(exp, q, nprobe, metric)[1]:
            assert all(np.abs(p).max(initial=0) <= INT32_MAX for p in planes)


@gpu
@pytest.mark.parametrize("dim", VALUE_DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_query_values(metric, dim):
    ix, exp, q = value_case(metric, dim)
    assert sq.step_of(exp[1], exp[2]).tobytes() == value_steps(metric, dim).tobytes()
    planes_inside_int32(exp, q, NLIST, metric)
    with np.errstate(all="ignore"):
        ref = ref_candidates(exp, q, MAX_K, MAX_K, NLIST, metric)
        ref32 = ref_candidates(exp, q, 10, 32, 3, metric)
    assert (ref[0][KINDS["nan"]] == -1).all() and (ref32[0][KINDS["nan"]] == -1).all(), "a NaN query has no candidate"
    ordinary = [i for i in range(VALUE_NQ) if i not in KINDS.values()]
    assert (ref[0][ordinary, 0] >= 0).all()
    same(ix.search_candidates(q, MAX_K, MAX_K, "nprobe=%d" % NLIST), ref)
    same(device_candidates(ix, q, 10, MAX_K, NLIST), first(ref, VALUE_NQ, 10))
    same(ix.search_candidates(q, 10, 32, "nprobe=3"), ref32)
    same(device_candidates(ix, q, 10, 32, 3), ref32)


def test_saturated_planes_stay_inside_int32_by_the_formula():
    h_max, l_max, s_max = SQC_WMAX >> 7, 127, 128
    assert h_max * s_max * sq_ld(DIM_MAX) <= INT32_MAX and l_max * s_max * sq_ld(DIM_MAX) <= INT32_MAX
    assert SQC_WMAX * s_max * DIM_MAX > INT32_MAX, "the sum of both planes at the largest dim is beyond int32: the kernel forms it in 64 bits"


@gpu
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(IP, id="ip")])
def test_saturated_images_against_saturated_codes(metric):
    """The largest admitted dim, rows far below and far above [vmin, vmax] (codes all 0, all 255) among ordinary ones, and queries
    whose every w is +-16256 among ordinary ones: |S| reaches 16256 x 128 x dim."""
    rng = np.random.default_rng(900 + metric)
    dim, nlist = DIM_MAX, 2
    step = np.full(dim, 2.0 ** -6, F)
    cent = np.zeros((nlist, dim), F)
    cent[0, 0], cent[1, 1] = 10, 10
    home = rng.integers(0, nlist, 90)
    x = (cent[home] + F(0.5) * rng.standard_normal((90, dim), dtype=F)).astype(F)
    x[10:13] -= F(1000)
    x[13:16] += F(1000)
    ix = capi.SqIndex(metric, dim)
    ix.set_codebook(cent, (F(-127.5) * step).astype(F), (F(127.5) * step).astype(F))
    ix.add(x)
    ix.build()
    ix.prepare_candidates()
    try:
        exp = ix.export()
        codes = exp[4]
        assert (codes == 0).all(axis=1).sum() == 3 and (codes == 255).all(axis=1).sum() == 3
        q = (cent[rng.integers(0, nlist, 20)] + F(0.5) * rng.standard_normal((20, dim), dtype=F)).astype(F)
        sign = np.where(np.arange(dim) % 2 == 0, 1, -1).astype(F)
        q[3], q[4], q[9], q[17] = 1, -1, sign, -sign
        for i in (3, 4, 9, 17):
            assert (np.abs(image_of(q[i], step)[1]) == SQC_WMAX).all()
        planes_inside_int32(exp, q, nlist, metric)
        total = [128 * a + b for _, _, _, (a, b) in ref_scores(exp, q, nlist, metric)[1]]
        assert max(np.abs(t).max() for t in total) == SQC_WMAX * 128 * dim > INT32_MAX
        assert sq_cand_tile(sq_ld(dim), MAX_K) == 16
        capi.debug_sq_cand_tiles()
        for k, kc in ((MAX_K, MAX_K), (5, 32)):
            ref = ref_candidates(exp, q, k, kc, nlist, metric)
            same(ix.search_candidates(q, k, kc, "nprobe=%d" % nlist), ref)
            same(device_candidates(ix, q, k, kc, nlist), ref)
        assert capi.debug_sq_cand_tiles() == (0, 4)
    finally:
        ix.close()


# ======================================================================================== A5. small edges

@gpu
@pytest.mark.parametrize("metric", [pytest.param(L2, id="l2"), pytest.param(COS, id="cosine")])
def test_bitmaps_shorter_than_the_labels(metric):
    ix, exp, q, labels = case(metric, 64)
    top = int(labels.max()) + 1
    rng = np.random.default_rng(11)
    for nbits in (top - 1, int(np.sort(labels)[len(labels) // 2]), 65, 64, 1):
        assert nbits <= labels.max()
        bits = rng.random(nbits) < 0.7
        bits[0] = True
        alive = np.zeros(top, bool)
        alive[:nbits] = bits
        for k, kc, nprobe in ((10, 32, 3), (MAX_K, MAX_K, NLIST)):
            ref = ref_candidates(exp, q, k, kc, nprobe, metric, alive)
            got = ix.search_candidates(q, k, kc, "nprobe=%d" % nprobe, alive=bits, nbits=nbits)
            same(got, ref)
            assert (got[0] < nbits).all()
    assert (labels == 0).any() == (ref[0] >= 0).any(), "nbits = 1: label 0 or nothing"


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_nprobe_one_on_the_empty_list(metric):
    ix, exp, q, labels = case(metric, 64)
    empty = SIZES.index(0)
    q = q[:20].copy()
    q[[0, 7, 19]] = exp[0][empty]  # the empty list's own centroid: nearest by L2, largest by inner product
    ref = ref_candidates(exp, q, 10, 32, 1, metric)
    assert (ref[0][[0, 7, 19]] == -1).all() and (ref[0][:, 0] >= 0).sum() >= 10
    same(ix.search_candidates(q, 10, 32, "nprobe=1"), ref)
    same(device_candidates(ix, q, 10, 32, 1), ref)
    same(ix.search_candidates(q[:1], 1, 1, "nprobe=1"), first(ref, 1, 1))


@gpu
@pytest.mark.parametrize("level", ["moderate", "extreme"])
@pytest.mark.parametrize("metric", METRICS)
def test_special_stored_rows_through_the_candidate_search(metric, level):
    """The 8-bit index of test_coded_special_rows over its non-finite, overflowing, zero and subnormal rows, every list probed, a
    filter that keeps every special row and so few ordinary ones that kc = 256 covers all the alive rows: the candidate pass drops
    nothing, so the result is search's wherever the candidate score is a number -- the definition drops a NaN score, and the
    reference says for which queries it has one."""
    import test_coded_special_rows as csr
    form = ("sq", 8, 0)
    _, x, kind_of, labels, q, _, _, _ = csr.fed(metric, level)
    ix, exp = csr.build(form, metric, level)
    try:
        ix.prepare_candidates()
        ref8 = csr.reference(form, metric, level, csr.lists_of_export(exp, labels))
        for got, want in zip(exp, ref8.exp):
            assert got.tobytes() == want.tobytes()
        k, nprobe = csr.ROWS_K, csr.ROWS_NLIST
        alive = np.random.default_rng(3).random(int(labels.max()) + 1) < 0.04
        alive[labels[sorted(kind_of)]] = True
        assert len(kind_of) < alive[labels].sum() <= MAX_K
        with np.errstate(all="ignore"):
            ref = ref_candidates(exp, q, k, MAX_K, nprobe, metric, alive)
            numbers = np.array([not np.isnan(worse).any() for _, _, worse, _ in ref_scores(exp, q, nprobe, metric)[1]])
            unfiltered = ref_candidates(exp, q, k, MAX_K, nprobe, metric)
        exact = ref8.search(q, nprobe, k, alive=alive)
        assert numbers[:128].all(), "the ordinary queries"
        assert (ref[0][numbers] == exact[0][numbers]).all() and (ref[1][numbers].view(np.uint32) == exact[1][numbers].view(np.uint32)).all()
        got = ix.search_candidates(q, k, MAX_K, "nprobe=%d" % nprobe, alive=alive)
        same(got, ref)
        same(device_candidates(ix, q, k, MAX_K, nprobe), unfiltered)
        plain = ix.search(q, k, "nprobe=%d" % nprobe, alive=alive)
        assert (got[0][numbers] == plain[0][numbers]).all() and (got[1][numbers].view(np.uint32) == plain[1][numbers].view(np.uint32)).all()
    finally:
        ix.close()
