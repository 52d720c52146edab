"""The graph index (graph_kernels.hpp, graph_index.hip) at the edges its own test file does not reach: dimensions up to 8192 and the
largest LDS image the API can ask for, a batch beyond one query chunk, query values that are not ordinary numbers, and rounds that
fill all 256 places of a round.

Part 1 of every section restates the launcher's formulas in Python -- constants read from the sources -- and asserts, without a GPU,
that each case is in the state it was written for.  Part 2 (marked gpu) runs the cases: ids == and distances by their uint32 view
against test_graph_index.ref_search, no tolerance anywhere."""
import functools
import os
import re

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_batch_chunks as tb
import test_graph_index as tg
from oracle import oracle as o
from test_graph_index import COS, F, IP, L2, NONE, code_of, ref_search, same, store_of, stored
from test_large_dims import CSRC, MAX_DIM, ceil_div, header_const

gpu = pytest.mark.gpu
NAME = {L2: "l2", IP: "ip", COS: "cosine"}
METRICS = [pytest.param(m, id=NAME[m]) for m in (L2, IP, COS)]
MAX_K = capi.MAX_K
GRAPH_ROUND = header_const("graph_kernels.hpp", "GRAPH_ROUND")
GRAPH_CTL = header_const("graph_kernels.hpp", "GRAPH_CTL")
GRAPH_LDS_MAX = header_const("graph_index.hip", "GRAPH_LDS_MAX")
GRAPH_QUERY_CHUNK = header_const("graph_index.hip", "GRAPH_QUERY_CHUNK")


def visited_max():
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "msvs.h")) as f:
        return int(re.search(r"#define\s+MSVS_GRAPH_VISITED_MAX\s+([0-9]+)", f.read()).group(1))


VISITED_MAX = visited_max()


# ======================================================================================== the launcher, restated

def graph_lds_bytes(ld4, tab):
    return ld4 * 16 + GRAPH_ROUND * (8 + 8 + 4 + 4) + GRAPH_CTL * 4 + tab * 4


def graph_tab(P, width, R, ef, max_iters=None):
    """graph_search_device: the visited table's slots, twice what the search can score at most"""
    max_iters = max_iters or ceil_div(2 * ef, width) + 8
    reach = min(VISITED_MAX, P + min(max_iters, VISITED_MAX) * width * R)
    return 2 * max(reach, 32)


def small_graph(rng, n, R, head):
    """any graph will do: the neighbours by the first columns, then self loops, a label twice and holes in every other row"""
    order = o.knn(head, head, R + 1, o.METRIC_L2)[0]
    nbr = order[:, 1:R + 1].astype(np.uint32)
    odd = np.arange(n) % 2 == 1
    nbr[odd, 0] = np.arange(n)[odd]
    nbr[odd, 5] = nbr[odd, 3]
    nbr[odd[:, None] & (rng.random((n, R)) < 0.2)] = NONE
    return nbr


def device_search(ix, q, k, **kw):
    """the device entry with the queries computed on a stream that is not the current one, outputs pre-filled with -7 / NaN"""
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).cuda()
    di = torch.full((len(q), k), -7, device="cuda", dtype=torch.int64)
    dd = torch.full((len(q), k), float("nan"), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    s = tb.side_stream()
    with torch.cuda.stream(s):
        q2 = dq * 1
        ix.search_device(q2.data_ptr(), len(q), k, di.data_ptr(), dd.data_ptr(), stream=s.cuda_stream, **kw)
    s.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


# ======================================================================================== B1. dimensions

DIM_N, DIM_NLIST, DIM_NQ = 300, 16, 5
DIMS = [2049, 4096, 8191, 8192]
DIM_CASES = [((L2, IP, COS)[c % 3], DIMS[c % 4], (16, 64)[(c // 4) % 2], (1, 2)[(c // 3) % 2], (None, 3)[(c // 5) % 2]) for c in range(12)]
TOP = dict(dim=MAX_DIM, R=64, width=4, ef=MAX_K, k=MAX_K, nprobe=DIM_NLIST, max_iters=5000)  # the largest image


def test_dimension_cases_and_the_largest_image():
    assert {(m, d) for m, d, _, _, _ in DIM_CASES} == {(m, d) for m in (L2, IP, COS) for d in DIMS}
    assert {(d, R) for _, d, R, _, _ in DIM_CASES} == {(d, R) for d in DIMS for R in (16, 64)}
    assert {c[3] for c in DIM_CASES} == {1, 2} and {c[4] for c in DIM_CASES} == {None, 3}
    assert max(DIMS) == MAX_DIM and DIM_N * MAX_DIM * 4 <= 20 << 20
    assert VISITED_MAX == capi.GRAPH_VISITED_MAX and MAX_K == GRAPH_ROUND
    t = TOP
    tab = graph_tab(t["nprobe"], t["width"], t["R"], t["ef"], t["max_iters"])
    assert tab == 2 * VISITED_MAX, "the visited table at its maximum"
    top = graph_lds_bytes(ceil_div(t["dim"], 4), tab)
    assert top <= GRAPH_LDS_MAX and top > 128 << 10
    # nothing the API admits asks for more: the image grows with the dimension and with the table, and both are at their limit
    assert top == max(graph_lds_bytes(ceil_div(d, 4), graph_tab(P, w, R, ef, it))
                      for d in (1, 2049, MAX_DIM) for P in (1, MAX_K) for w in (1, 4) for R in (16, 32, 64) for ef in (1, MAX_K)
                      for it in (None, 1, 47, 48, 5000, 1 << 40))
    assert graph_tab(MAX_K, 4, 64, MAX_K, 1 << 40) == tab
    for _, d, R, width, max_iters in DIM_CASES:  # the table cases: smaller tables, every image far beyond 64 KiB only at the top
        assert graph_lds_bytes(ceil_div(d, 4), graph_tab(8, width, R, 16, max_iters)) <= GRAPH_LDS_MAX


@functools.lru_cache(maxsize=None)
def dim_data(dim):
    rng = np.random.default_rng(8000 + dim)
    _, x = tg.blobs(rng, DIM_N, dim, DIM_NLIST, sigma=0.6)
    x[-20:] = x[:20]  # equal rows: equal distances, the labels decide
    q = (x[rng.integers(0, DIM_N, DIM_NQ)] + F(0.3) * rng.standard_normal((DIM_NQ, dim), dtype=F)).astype(F)
    cent = x[rng.permutation(DIM_N)[:DIM_NLIST]].copy()
    seeds = rng.integers(0, DIM_N, DIM_NLIST).astype(np.int32)
    seeds[3] = -1
    return x, q, cent, seeds, {R: small_graph(rng, DIM_N, R, np.ascontiguousarray(x[:, :8])) for R in (16, 64)}, rng.random(DIM_N) < 0.5


@gpu
@pytest.mark.parametrize("metric,dim,R,width,max_iters", DIM_CASES)
def test_dimensions(metric, dim, R, width, max_iters):
    x, q, cent, seeds, graphs, half = dim_data(dim)
    nbr = graphs[R]
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d" % R)
    try:
        ix.set_graph(cent, seeds, nbr)
        for ef, k, alive in ((16, 10, None), (16, 16, half)):
            ends = []
            exp = ref_search(stored(x, metric), cent, seeds, nbr, q, k, metric, ef, 8, width, max_iters, alive, ends)
            if max_iters:
                assert "iters" in ends
            params = "ef=%d,nprobe=8,width=%d" % (ef, width) + (",max_iters=%d" % max_iters if max_iters else "")
            same(ix.search(q, k, params, alive=alive), exp)
            same(tg.device_search(ix, q, k, alive, ef=ef, nprobe=8, width=width, max_iters=max_iters or 0), exp)
    finally:
        ix.close()
        rows.close()


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_the_largest_lds_image(metric):
    t = TOP
    x, q, cent, seeds, graphs, _ = dim_data(t["dim"])
    nbr = graphs[t["R"]]
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d" % t["R"])
    try:
        ix.set_graph(cent, seeds, nbr)
        exp = ref_search(stored(x, metric), cent, seeds, nbr, q, t["k"], metric, t["ef"], t["nprobe"], t["width"], t["max_iters"])
        assert (exp[0][:, 100] >= 0).all()
        same(ix.search(q, t["k"], "ef=%d,nprobe=%d,width=%d,max_iters=%d" % (t["ef"], t["nprobe"], t["width"], t["max_iters"])), exp)
        same(device_search(ix, q, t["k"], ef=t["ef"], nprobe=t["nprobe"], width=t["width"], max_iters=t["max_iters"]), exp)
    finally:
        ix.close()
        rows.close()


# ======================================================================================== B2. past one query chunk

CHUNK_NQ = GRAPH_QUERY_CHUNK + tb.TAIL
CHUNK_N, CHUNK_DIM, CHUNK_NLIST, CHUNK_NDIST = 500, 8, 16, 300
CHUNK_SEARCH = dict(ef=8, nprobe=4, width=2)
CHUNK_K = 5


def test_chunk_case_is_two_chunks():
    assert GRAPH_QUERY_CHUNK == 16384 and GRAPH_QUERY_CHUNK < CHUNK_NQ < 2 * GRAPH_QUERY_CHUNK and CHUNK_NQ % GRAPH_QUERY_CHUNK == tb.TAIL


@functools.lru_cache(maxsize=None)
def chunk_case(metric):
    rng = np.random.default_rng(500 + metric)
    centres, x, dq = tb.int_blobs(rng, CHUNK_NLIST, CHUNK_N, CHUNK_NDIST, CHUNK_DIM)
    cent = np.ascontiguousarray(o.normalize_rows(centres) if metric == COS else centres, F)
    seeds = rng.integers(0, CHUNK_N, CHUNK_NLIST).astype(np.int32)
    nbr = small_graph(rng, CHUNK_N, 16, np.ascontiguousarray(x[:, :8]))
    ref = ref_search(stored(x, metric), cent, seeds, nbr, dq, CHUNK_K, metric, **CHUNK_SEARCH)
    return x, cent, seeds, nbr, dq, tb.straddle(rng, CHUNK_NQ, GRAPH_QUERY_CHUNK, CHUNK_NDIST), ref


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_batch_beyond_one_query_chunk(metric):
    x, cent, seeds, nbr, dq, pick, ref = chunk_case(metric)
    tb.answers_differ(ref)
    q = np.ascontiguousarray(dq[pick])
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=16")
    try:
        ix.set_graph(cent, seeds, nbr)
        params = "ef=%d,nprobe=%d,width=%d" % (CHUNK_SEARCH["ef"], CHUNK_SEARCH["nprobe"], CHUNK_SEARCH["width"])
        with tb.profile() as run:
            for entry, fn in (("host", lambda: ix.search(q, CHUNK_K, params)), ("device", lambda: device_search(ix, q, CHUNK_K, **CHUNK_SEARCH))):
                got, count = run(fn)
                tb.check(got, ref, pick, GRAPH_QUERY_CHUNK, "%s %s entry" % (NAME[metric], entry))
                assert count("graph_search") == 2, "%s entry: %d launches of graph_search_kernel" % (entry, count("graph_search"))
    finally:
        ix.close()
        rows.close()
        capi.release_scratch()


# ======================================================================================== B3. query values

VALUE_AT = {"nan": 2, "+inf": 5, "-inf": 8, "overflow": 11, "huge": 13, "zeros": 16, "-zeros": 19, "subnormal": 22, "tiny": 25}


def value_queries(base):
    q = base.copy()
    dim = q.shape[1]
    sign = np.where(np.arange(dim) % 2 == 0, 1, -1).astype(F)
    q[VALUE_AT["nan"], 1] = np.nan
    q[VALUE_AT["+inf"], 0] = np.inf
    q[VALUE_AT["-inf"], dim - 1] = -np.inf
    q[VALUE_AT["overflow"]] = F(3e38) * sign   # every product and every difference overflows
    q[VALUE_AT["huge"], 3] = 1e30              # finite, its square is not
    q[VALUE_AT["zeros"]] = 0
    q[VALUE_AT["-zeros"]] = -0.0
    q[VALUE_AT["subnormal"]] = F(1e-40) * sign
    q[VALUE_AT["tiny"], :] = 0
    q[VALUE_AT["tiny"], 4] = 1e-45
    return q


def test_value_queries_sit_among_ordinary_ones():
    at = sorted(VALUE_AT.values())
    assert all(b - a >= 2 for a, b in zip(at, at[1:])) and at[-1] < 33
    q = value_queries(np.ones((33, 67), F))
    assert sum(not np.isfinite(r).all() for r in q) == 3 and np.isfinite(q[VALUE_AT["overflow"]]).all()
    assert 0 < np.abs(q[VALUE_AT["subnormal"]]).max() < np.finfo(F).tiny and np.count_nonzero(q[VALUE_AT["tiny"]]) == 1


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_query_values(metric):
    x, q, cent, _, half = tg.data(67)
    q = value_queries(q)
    ix, (seeds, nbr) = tg.handed(metric, 67, 16, "knn"), tg.graph(67, 16, "knn")
    for ef, k, width, alive in ((64, 10, 1, None), (32, 32, 4, half)):
        with np.errstate(all="ignore"):
            exp = ref_search(stored(x, metric), cent, seeds, nbr, q, k, metric, ef, 8, width, None, alive)
        assert (exp[0][VALUE_AT["nan"]] == -1).all(), "a NaN query admits no row"
        ordinary = [i for i in range(len(q)) if i not in VALUE_AT.values()]
        assert (exp[0][ordinary, 0] >= 0).all()
        same(ix.search(q, k, "ef=%d,width=%d" % (ef, width), alive=alive), exp)
        same(tg.device_search(ix, q, k, alive, ef=ef, width=width), exp)


# ======================================================================================== B4. full rounds

FULL_NLIST, FULL_R, FULL_WIDTH, FULL_DIM = 300, 64, 4, 8
FULL_N = FULL_NLIST + FULL_NLIST * FULL_R


@functools.lru_cache(maxsize=None)
def full_case():
    """300 lists whose seeds are the labels 0 .. 299; seed s points at the 64 labels 300 + 64 s ..., which nobody else points at"""
    rng = np.random.default_rng(77)
    x = rng.standard_normal((FULL_N, FULL_DIM), dtype=F)
    cent = rng.standard_normal((FULL_NLIST, FULL_DIM), dtype=F)
    q = rng.standard_normal((6, FULL_DIM), dtype=F)
    seeds = np.arange(FULL_NLIST, dtype=np.int32)
    nbr = rng.integers(0, FULL_N, (FULL_N, FULL_R)).astype(np.uint32)
    nbr[:FULL_NLIST] = FULL_NLIST + np.arange(FULL_NLIST * FULL_R, dtype=np.uint32).reshape(FULL_NLIST, FULL_R)
    return x, cent, q, seeds, nbr


def test_full_case_fills_the_rounds():
    x, cent, q, seeds, nbr = full_case()
    assert min(MAX_K, FULL_NLIST) == GRAPH_ROUND == FULL_WIDTH * FULL_R
    for metric in (L2, IP, COS):
        om = o.METRIC_L2 if metric == L2 else o.METRIC_IP
        lists = o.knn(o.normalize_rows(q) if metric == COS else q, cent, GRAPH_ROUND, om)[0]
        for row in lists:  # the seed round stages 256 distinct valid labels
            assert (row >= 0).all() and len(set(seeds[row].tolist())) == GRAPH_ROUND
    # whichever four seeds are the first parents: 256 neighbour words, no hole, no repeat, none of them a seed (so none visited)
    first = nbr[:FULL_NLIST].ravel()
    assert len(set(first.tolist())) == FULL_NLIST * FULL_R and first.min() >= FULL_NLIST and first.max() < FULL_N
    assert GRAPH_ROUND + GRAPH_ROUND <= VISITED_MAX


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_full_rounds(metric):
    x, cent, q, seeds, nbr = full_case()
    cent = np.ascontiguousarray(o.normalize_rows(cent) if metric == COS else cent, F)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d" % FULL_R)
    try:
        for same_seed in (False, True):
            s = np.full(FULL_NLIST, 7, np.int32) if same_seed else seeds
            ix.set_graph(cent, s, nbr)
            for max_iters in (1, 6):
                ends = []
                exp = ref_search(stored(x, metric), cent, s, nbr, q, MAX_K, metric, MAX_K, GRAPH_ROUND, FULL_WIDTH, max_iters, None, ends)
                assert ends == ["iters"] * len(q)
                if not same_seed:
                    assert (exp[0] >= 0).all(), "a beam of 256 out of 512 scored rows"
                    if max_iters == 1:  # the first parents' neighbours did get into the beam
                        assert ((exp[0] >= FULL_NLIST) & (exp[0] < FULL_N)).any(axis=1).all()
                params = "ef=%d,nprobe=%d,width=%d,max_iters=%d" % (MAX_K, GRAPH_ROUND, FULL_WIDTH, max_iters)
                same(ix.search(q, MAX_K, params), exp)
                same(device_search(ix, q, MAX_K, ef=MAX_K, nprobe=GRAPH_ROUND, width=FULL_WIDTH, max_iters=max_iters), exp)
            # 300 probes: beyond the coarse quantiser's top-k limit
            assert code_of(lambda: ix.search(q, 10, "nprobe=%d" % FULL_NLIST)) == capi.ERR_UNSUPPORTED_K
            assert code_of(lambda: device_search(ix, q, 10, nprobe=FULL_NLIST)) == capi.ERR_UNSUPPORTED_K
    finally:
        ix.close()
        rows.close()
