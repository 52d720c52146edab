"""Dimensions 2049 .. 8192 on every path that sizes its LDS image by d.

Every float entry point admits 1 <= dim <= 8192, and between 2049 and 8192 the planners do not run the same kernels on longer
rows: each one that keeps a query tile in LDS changes tile or path there.  Part 1 restates the planners' formulas in Python, with the
constants read from the headers, and asserts for every GPU case below which side of which switch it lands on and that the case
tables reach both sides of every switch; it needs no GPU.  Part 2 runs the cases: ids and distance bits against the oracle on the
exported structure (the coded indexes: against the references of their own test files), and the path each case was written for, seen
through prefilter_stats / coarse_stats deltas, profile scopes, the record of the last shadow list scan (msvs_debug_h16_keys /
msvs_debug_h16_items), the pre-pruning's record (msvs_debug_prune_first) and the canonical planners' last query tiles
(msvs_debug_planned_tiles, a counter read added with this module: nothing else tells a tile of 8 from one of 4).

Data: sigma-0.3 blobs around the centroids, the last eighth of the rows copies of the first eighth (equal distances, the ids
decide).  A few hundred to a few thousand rows: the largest table, 8192 rows of 2560 floats, is 84 MB."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
OM = {L2: o.METRIC_L2, IP: o.METRIC_IP}
NAME = {L2: "L2", IP: "IP", COS: "cosine"}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myscaledb_amd", "csrc")
gpu = pytest.mark.gpu


# ======================================================================================== 1. the planners, restated

def header_const(header, name):
    """`constexpr <type> NAME = <integer expression>;` of a header of the library"""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+[\w:]+\s+%s\s*=\s*([0-9*+() ]+);" % name, f.read())
    assert m, "%s: no constant %s" % (header, name)
    return int(eval(m.group(1), {"__builtins__": {}}))


def option_default(name):
    """`double NAME = <number>;` of the options in common.hpp"""
    with open(os.path.join(CSRC, "common.hpp")) as f:
        m = re.search(r"double\s+%s\s*=\s*([0-9.eE+-]+);" % name, f.read())
    assert m, "common.hpp: no option %s" % name
    return float(m.group(1))


H_NW = header_const("h16_scan_kernels.hpp", "H_NW")
H_STAGE = header_const("h16_scan_kernels.hpp", "H_STAGE")
H_CHUNK = header_const("h16_scan_kernels.hpp", "H_CHUNK")
H8_CHUNK = header_const("h16_scan_kernels.hpp", "H8_CHUNK")
H_ROWS = header_const("h16_scan_kernels.hpp", "H_ROWS")
BLOCK = header_const("scan_kernels.hpp", "BLOCK")
HEADS_CAP = header_const("scan_kernels.hpp", "HEADS_CAP")
SCAN_LDS_BUDGET = header_const("scan_kernels.hpp", "SCAN_LDS_BUDGET")
PQ_LDS_BUDGET = header_const("pq_ivf_kernels.hpp", "PQ_LDS_BUDGET")
LAT_MAX_K = header_const("latency_kernels.hpp", "LAT_MAX_K")
LAT_MAX_Q = header_const("latency_kernels.hpp", "LAT_MAX_Q")
H16_MIN_PAIRS = option_default("h16_min_pairs")
H16_LDS_BUDGET = 160 * 1024  # the literal of plan_ivf's and the FLAT passes' gates (msvs_capi.hip): the LDS of a CU
MAX_DIM = 8192
MAX_K = capi.MAX_K
MI355X_CUS = 256  # lat_shape sizes its grid by the device's compute units


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def padded_dim(d):
    return round_up(d, 4)


def scan_lds_bytes(T, ld4, k):
    return T * ld4 * 16 + T * 5 * k * 8


def h16_lds_bytes(ncb, nch, i8=False):
    tq = 32 * ncb
    return tq * nch * 128 + 4 * tq * 4 + H_NW * H_STAGE * 12 + 16 + (4 * tq if i8 else 0)


def tile_nch(d, form):
    """128-byte chunks of a query's image in the list scan's tile: fp16 (form 2), or the hi and lo images of an i8r pair (form 3)"""
    return 2 * ceil_div(d, H8_CHUNK) if form == 3 else ceil_div(d, H_CHUNK)


def shadow_serves(d, form=2):
    return h16_lds_bytes(1, tile_nch(d, form), form == 3) <= H16_LDS_BUDGET


def list_scan_ncb(d, form, pairs, nlist):
    ncb = min(4, max(2, ceil_div(2 * ceil_div(pairs, nlist), 32)))
    while ncb > 1 and h16_lds_bytes(ncb, tile_nch(d, form), form == 3) > H16_LDS_BUDGET:
        ncb -= 1
    return ncb


def flat_T(nq, ld, k):
    t = 1 if nq <= 1 else 2 if nq <= 2 else 4 if nq <= 4 else 8
    while t > 1 and scan_lds_bytes(t, ld // 4, k) > SCAN_LDS_BUDGET:
        t //= 2
    return t


def ivf_T(pairs, nlist, ld, k):
    t = 8 if pairs >= 16 * nlist else 4 if pairs >= 2 * nlist else 2 if pairs >= nlist else 1
    while t > 1 and scan_lds_bytes(t, ld // 4, k) > SCAN_LDS_BUDGET:
        t //= 2
    return t


def candidate_pass(d, form, k, pairs, nlist, mode):
    """plan_ivf's first branch for an index with finite norms -> None (the canonical scan), "shadow" or "split-bf16"."""
    h16 = form != 0 and shadow_serves(d, form)
    eligible = k <= 40 or (h16 and k <= 128)
    min_pairs = H16_MIN_PAIRS if h16 else 4.0
    if mode != 0 and eligible and (pairs >= min_pairs * nlist or mode >= 2):
        return "shadow" if h16 else "split-bf16"
    return None


def coarse_shadow_eligible(nlist, nq, nprobe, min_q=option_default("coarse_h16_min_q")):
    return nprobe <= 40 and nlist >= 256 and nq >= min_q and nq * round_up(nlist, H_ROWS) * 4 <= 128 << 20


def lat_merge_lds(n_lists, k):
    total = n_lists * k
    return total * 8 + k * 8 + n_lists * 2 + 16 if total <= HEADS_CAP else 5 * k * 8


def lat_lds(d, nlist, nq, k, nprobe, cus):
    """lat_shape's two LDS sizes"""
    ld = padded_dim(d)
    c_rows = 32 * ceil_div(nlist * nprobe, 32 * HEADS_CAP)
    c_blocks = ceil_div(nlist, c_rows)
    items = max(nprobe, 2 * cus // nq - nprobe if 2 * cus // nq > nprobe else nprobe)
    grid_x = items + nprobe
    return ld * 4 + max(5 * nprobe * 8, lat_merge_lds(c_blocks, nprobe)), ld * 4 + max(5 * k * 8, lat_merge_lds(grid_x, k))


def lat_eligible(d, nlist, nq, k, nprobe, cus):
    nprobe = min(max(nprobe, 1), nlist)
    if not 1 <= nq <= min(LAT_MAX_Q, 2) or not 1 <= k <= LAT_MAX_K or nprobe > LAT_MAX_K:
        return False
    lds1, lds2 = lat_lds(d, nlist, nq, k, nprobe, cus)
    return lds1 <= SCAN_LDS_BUDGET and lds2 <= SCAN_LDS_BUDGET


def refine_lds_bytes(ld4, kc):
    return ld4 * 16 + kc * 8


def pq_lds_bytes(bits, T, m, ld, k, form=0):
    tables, merge = T * m * (4 << bits), T * 5 * k * 8
    return tables + merge + T * 4 if form else tables + (T + 1) * ld * 4 + merge


def pq_fits(dim, m, bits):
    if bits not in (4, 8) or not 1 <= dim <= MAX_DIM or not 1 <= m <= 1024 // bits or dim % m:
        return False
    return pq_lds_bytes(bits, 1, m, padded_dim(dim), MAX_K) <= PQ_LDS_BUDGET


def pq_T(bits, m, ld, k, pairs, nlist, form=0):
    t = 8 if pairs >= 16 * nlist else 4 if pairs >= 2 * nlist else 2 if pairs >= nlist else 1
    while t > 1 and pq_lds_bytes(bits, t, m, ld, k, form) > PQ_LDS_BUDGET:
        t //= 2
    return t


def sq_fits(dim):
    ld4 = round_up(dim, 16) // 4
    return 1 <= dim <= MAX_DIM and (2 + 3) * ld4 * 16 + 2 * 5 * MAX_K * 8 <= SCAN_LDS_BUDGET


# ---------------------------------------------------------------------------------------- the case tables

# a. (d, shadow form at build, k) -> the list scan's pass under ivf_pass = 2; nq = 64, 4 lists, all probed
EDGE_NQ, EDGE_NLIST = 64, 4
EDGE = [(d, form, k, "shadow" if d == 2432 else "split-bf16") for d in (2432, 2433) for form in (2, 3) for k in (10, 40)] \
    + [(2433, form, k, None) for form in (2, 3) for k in (41, 128)]
# b. d -> the tile width (column blocks of 32 queries) of 300 queries on each of 4 lists, per shadow form
WIDTH_NQ, WIDTH_LENGTHS = 300, [0, 20, 33, 1000]
WIDTH = {576: {2: 4, 3: 3}, 640: {2: 3, 3: 3}, 832: {2: 2, 3: 2}, 1216: {2: 2, 3: 1}, 1280: {2: 1, 3: 1}}
# c. the coarse quantiser through the centroid shadow in front of a list scan that cannot use its own
MIXED = dict(d=2560, nlist=256, n=8192, nq=200, nprobe=8, k=10)
# d. (d, k) -> the canonical tile: T of plan_flat for 17 queries and of plan_ivf for 17 x 4 pairs on 4 lists (both ask for 8)
HALVING_NQ, HALVING_NLIST = 17, 4
HALVING = [(1948, 10, 8), (1952, 10, 4), (3996, 10, 4), (4000, 10, 2), (8092, 10, 2), (8192, 10, 1),
           (1536, 256, 4), (1540, 256, 2), (5632, 256, 2), (5636, 256, 1), (8192, 256, 1)]
# e. the few-query path: every (nq, k, nprobe) at every d; 16 lists
LAT_DIMS, LAT_NLIST = (2048, 8188, 8192), 16
LAT = [(nq, k, nprobe) for nq in (1, 2) for k in (1, 10, LAT_MAX_K) for nprobe in (1, 8)]
# f. the FLAT index's shadow passes
FLAT_SHADOW = {2432: True, 2496: False}
# h. IVFPQ at the top: (bits, dim, m, query_tables) -> T of a batch of 40 queries x 4 probes on 4 lists at k = 10 and k = 256
PQ_TOP = {(8, 8192, 64, 0): (1, 1), (8, 8184, 66, 0): (1, 1), (4, 8192, 256, 0): (2, 2), (8, 8192, 64, 1): (2, 2)}
PQ_NQ, PQ_NLIST = 40, 4


def test_formulas_give_the_thresholds():
    """The last dimension on the near side of every switch, from the formulas alone."""
    def last(pred, lo=1, hi=MAX_DIM):
        return max(d for d in range(lo, hi + 1) if pred(d))

    for form in (2, 3):
        assert last(lambda d: shadow_serves(d, form)) == 2432
        assert all(shadow_serves(d, form) for d in range(1, 2433)) and not any(shadow_serves(d, form) for d in range(2433, MAX_DIM + 1))
    assert tile_nch(2432, 2) == tile_nch(2432, 3) == 38 and tile_nch(2433, 2) == 39 and tile_nch(2433, 3) == 40
    many = 300 * 4
    assert [last(lambda d: list_scan_ncb(d, 2, many, 4) >= w) for w in (4, 3, 2)] == [576, 768, 1216]
    assert [last(lambda d: list_scan_ncb(d, 3, many, 4) >= w) for w in (4, 3, 2)] == [512, 768, 1152]  # whole 128-element chunks
    assert [last(lambda d: flat_T(17, padded_dim(d), 10) >= t) for t in (8, 4, 2)] == [1948, 3996, 8092]
    assert [last(lambda d: flat_T(17, padded_dim(d), 256) >= t) for t in (4, 2)] == [1536, 5632] and flat_T(17, 4, 256) == 4
    assert flat_T(17, 8192, 10) == flat_T(17, 8192, 256) == 1
    assert scan_lds_bytes(8, 1948 // 4, 10) == SCAN_LDS_BUDGET  # the tile of eight fits to the byte
    assert scan_lds_bytes(1, MAX_DIM // 4, MAX_K) <= SCAN_LDS_BUDGET  # one query of the largest dimension and k always fits
    assert last(sq_fits) == 2240 and not sq_fits(2241)
    assert refine_lds_bytes(MAX_DIM // 4, capi.REFINE_MAX_CAND) <= SCAN_LDS_BUDGET
    assert max(m for m in range(1, 129) if pq_fits(MAX_DIM, m, 8)) == 64 and not pq_fits(MAX_DIM, 128, 8)
    assert pq_fits(MAX_DIM, 256, 4) and not pq_fits(MAX_DIM + 1, 1, 8)
    # the 8-bit encoder stages a row and its centroid beside 64 static bytes: beyond 64 KiB in all from dim 8185 on
    assert last(lambda d: 2 * d * 4 + 64 <= 64 * 1024) == 8184


def test_case_tables_land_on_the_intended_side_of_every_switch():
    # a. the shadow's eligibility edge
    for d, form, k, want in EDGE:
        assert candidate_pass(d, form, k, EDGE_NQ * EDGE_NLIST, EDGE_NLIST, mode=2) == want, (d, form, k)
        if want is None:
            assert ivf_T(EDGE_NQ * EDGE_NLIST, EDGE_NLIST, padded_dim(d), k) >= 1
    assert {c[3] for c in EDGE} == {"shadow", "split-bf16", None}
    assert {(c[0], c[1]) for c in EDGE if c[3] == "shadow"} == {(2432, 2), (2432, 3)}
    # b. every tile width, the last dimension of 4 and of 2 among them
    for d, by_form in WIDTH.items():
        for form, ncb in by_form.items():
            assert list_scan_ncb(d, form, WIDTH_NQ * len(WIDTH_LENGTHS), len(WIDTH_LENGTHS)) == ncb, (d, form)
    assert {v[2] for v in WIDTH.values()} == {4, 3, 2, 1} and {v[3] for v in WIDTH.values()} == {3, 2, 1}
    assert WIDTH[576][2] == 4 and list_scan_ncb(577, 2, 1200, 4) == 3 and WIDTH[1216][2] == 2 and list_scan_ncb(1217, 2, 1200, 4) == 1
    # c. coarse shadow yes, list shadow no, candidate pass yes (the split-bf16 one) under default settings
    m = MIXED
    assert coarse_shadow_eligible(m["nlist"], m["nq"], m["nprobe"]) and not coarse_shadow_eligible(m["nlist"], 191, m["nprobe"])
    assert not shadow_serves(m["d"])
    assert candidate_pass(m["d"], 2, m["k"], m["nq"] * m["nprobe"], m["nlist"], mode=1) == "split-bf16"
    assert m["n"] * m["d"] * 4 <= 84 << 20
    # d. canonical tile halving: the batch asks for eight, d and k alone decide
    assert HALVING_NQ * HALVING_NLIST >= 16 * HALVING_NLIST
    for d, k, T in HALVING:
        assert d % 4 == 0 and flat_T(HALVING_NQ, d, k) == T and ivf_T(HALVING_NQ * HALVING_NLIST, HALVING_NLIST, d, k) == T, (d, k)
    assert {c[2] for c in HALVING if c[1] == 10} == {8, 4, 2, 1} and {c[2] for c in HALVING if c[1] == 256} == {4, 2, 1}
    for a, b in zip(HALVING[0:6:2] + HALVING[6:10:2], HALVING[1:6:2] + HALVING[7:10:2]):
        assert a[1] == b[1] and a[2] == 2 * b[2] and b[0] - a[0] <= 100  # each pair straddles one halving
    # e. the few-query path: eligible and not, and not monotonic in nq (two queries share the CUs: half the partial lists each)
    side = {(d, c): lat_eligible(d, LAT_NLIST, c[0], c[1], c[2], MI355X_CUS) for d in LAT_DIMS for c in LAT}
    assert all(side[(2048, c)] for c in LAT)
    for d in (8188, 8192):
        assert not side[(d, (1, 10, 1))] and not side[(d, (1, 10, 8))] and side[(d, (2, 10, 8))]
        assert side[(d, (1, 1, 8))] and side[(d, (1, LAT_MAX_K, 8))] and side[(d, (2, LAT_MAX_K, 1))]
    assert not lat_eligible(8192, LAT_NLIST, 1, LAT_MAX_K + 1, 8, MI355X_CUS)
    # f. the FLAT passes' gate is the list scan's at one column block
    for d, serves in FLAT_SHADOW.items():
        assert shadow_serves(d, 2) == serves
    # h. IVFPQ: admitted, and the tile of the batch
    for (bits, dim, m, form), (t10, t256) in PQ_TOP.items():
        assert pq_fits(dim, m, bits)
        pairs = PQ_NQ * PQ_NLIST
        assert pairs >= 16 * PQ_NLIST
        assert (pq_T(bits, m, padded_dim(dim), 10, pairs, PQ_NLIST, form), pq_T(bits, m, padded_dim(dim), 256, pairs, PQ_NLIST, form)) == (t10, t256)
    assert {2 * dim * 4 + 64 > 64 * 1024 for bits, dim, m, form in PQ_TOP if bits == 8} == {True, False}


# ======================================================================================== 2. on the device

def same(a_ids, a_dis, b_ids, b_dis, what=""):
    assert a_ids.shape == b_ids.shape, what
    assert np.array_equal(a_ids, b_ids), "%s: ids differ at %s" % (what, np.argwhere(a_ids != b_ids)[:4].tolist())
    assert np.array_equal(a_dis.view(np.uint32), b_dis.view(np.uint32)), "%s: distances differ" % what


def blobs(seed, n, d, nlist, nq, sigma=0.3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((nlist, d), dtype=F)
    x = (centers[rng.integers(0, nlist, n)] + F(sigma) * rng.standard_normal((n, d), dtype=F)).astype(F)
    x[n - n // 8:] = x[:n // 8]  # ties: equal distances, the ids decide
    q = (centers[rng.integers(0, nlist, nq)] + F(sigma) * rng.standard_normal((nq, d), dtype=F)).astype(F)
    return centers, x, q


def build_ivf(x, metric, centers):
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, x.shape[1], "ncentroids=%d" % len(centers))
    ix.set_centroids(centers)
    half = x.shape[0] // 2
    ix.add(x[:half])
    ix.add(x[half:])
    ix.build()
    return ix


def build_flat(x, metric):
    ix = capi.Index(capi.INDEX_FLAT, metric, x.shape[1], "")
    ix.add(x)
    ix.build()
    return ix


def oracle_on_exported(ix, q, nprobe, k, metric, alive=None):
    cent, off, vecs, lids = ix.export()
    if metric == COS:
        oi, od, _ = o.ivf_search(cent, off, vecs, lids, o.normalize_rows(q), nprobe, k, o.METRIC_IP, alive=alive)
        return oi, (F(1) - od).astype(F)
    oi, od, _ = o.ivf_search(cent, off, vecs, lids, q, nprobe, k, OM[metric], alive=alive)
    return oi, od


def oracle_flat(ix, q, k, metric, alive=None):
    _, _, vecs, lids = ix.export()
    assert np.array_equal(lids, np.arange(len(lids)))  # a FLAT index keeps its rows in id order
    if metric == COS:
        oi, od = o.knn(o.normalize_rows(q), vecs, k, o.METRIC_IP, alive=alive)
        return oi, (F(1) - od).astype(F)
    return o.knn(q, vecs, k, OM[metric], alive=alive)


def device_search(ix, q, k, nprobe):
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    di = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    dd = torch.empty((len(q), k), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), len(q), k, nprobe, di.data_ptr(), dd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


def shadow_form(ix):
    capi.lib().msvs_debug_shadow_form.restype = C.c_int
    return capi.lib().msvs_debug_shadow_form(ix._h)


def shadow_scan_on_record(nq):
    """msvs_debug_h16_keys: whether this thread's last recorded shadow list scan was one of nq queries; the call retires the record"""
    keys, cnt = np.zeros((nq, 1), np.uint64), np.zeros(nq, np.uint32)
    return capi.lib().msvs_debug_h16_keys(keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_size_t(1), cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          C.c_size_t(nq)) == 0


def plan_items():
    """msvs_debug_h16_items of the last shadow list scan -> (work items of the main launch, the blocks per row segment its plan chose
    (0: one segment a list), work items of the sample launch)"""
    out = np.zeros(9, np.uint32)
    rc = capi.lib().msvs_debug_h16_items(out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, capi.lib().msvs_last_error()
    assert out[4] == 0 and out[8] == 0, "item records that do not fit the plan: %s" % out.tolist()
    return int(out[2]), int(out[3]), int(out[7])


def planned_tiles():
    """msvs_debug_planned_tiles -> (query tile of this thread's last canonical table scan, of its last canonical list scan); 0: none
    since the last read"""
    out = np.zeros(2, np.uint32)
    rc = capi.lib().msvs_debug_planned_tiles(out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, capi.lib().msvs_last_error()
    return int(out[0]), int(out[1])


def plan_nseg(blocks, sb):
    """plan_items.hpp: row segments of a list of `blocks` 32-row blocks at sb blocks a segment"""
    return 0 if blocks == 0 else (1 if sb == 0 else max(1, (blocks + sb // 2) // sb))


@pytest.fixture
def calls():
    """-> f(scope names, fn): fn's result and how often each ProfileScope ran inside it"""
    capi.profile_enable(True)

    def run(names, fn):
        capi.profile_reset()
        res = fn()
        return res, {n: capi.profile_get(n)[0] for n in names}

    yield run
    capi.profile_enable(False)
    capi.profile_reset()


def other_metric(i):
    return (IP, COS)[i % 2]


def force_form(opt, form, metric):
    """h16_form: 2 = fp16; 3 = i8r for L2 and 4 = i8r whatever the metric"""
    opt("h16_form", "2" if form == 2 else "3" if metric == L2 else "4")


# ---------------------------------------------------------------------------------------- a. the shadow's eligibility edge

@gpu
@pytest.mark.parametrize("d,form", [(d, f) for d in (2432, 2433) for f in (2, 3)])
def test_shadow_eligibility_edge(d, form, opt):
    """d = 2432 (38 chunks): the shadow list scan serves all 64 queries; 2433: it serves none and the split-bf16 candidate pass
    does (k <= 40), or the canonical scan (k = 41, 128) -- prefilter_stats counts the queries of either pass, the record of the last
    shadow list scan tells them apart."""
    nq, nlist = EDGE_NQ, EDGE_NLIST
    for metric in (L2, other_metric(d + form)):
        centers, x, q = blobs(100 * d + form, 1200, d, nlist, nq)
        force_form(opt, form, metric)
        ix = build_ivf(x, metric, centers)
        assert shadow_form(ix) == form
        opt("ivf_pass", "2")
        for _, _, k, want in [c for c in EDGE if c[0] == d and c[1] == form]:
            oi, od = oracle_on_exported(ix, q, nlist, k, metric)
            shadow_scan_on_record(nq)
            p0 = capi.prefilter_stats()
            ids, dis = ix.search(q, k, "nprobe=%d" % nlist)
            p1 = capi.prefilter_stats()
            what = "d=%d form=%d %s k=%d" % (d, form, NAME[metric], k)
            same(ids, dis, oi, od, what)
            assert p1[0] - p0[0] == (nq if want else 0), "%s: the candidate passes served %d queries" % (what, p1[0] - p0[0])
            assert shadow_scan_on_record(nq) == (want == "shadow"), "%s: shadow list scan ran / did not run" % what
            print("%s: %s, %d fallbacks" % (what, want, p1[1] - p0[1]))
        opt("ivf_pass", None)
        ix.close()


# ---------------------------------------------------------------------------------------- b. the tile width

@gpu
@pytest.mark.parametrize("d", sorted(WIDTH))
def test_tile_width(d, opt):
    """300 queries on each of four lists of 0, 20, 33 and 1000 rows (no pruning, every list probed) ask for tiles of 128 queries;
    d decides what fits.  The main launch has one work item per (row segment behind a list's block 0, tile of 32 ncb queries), the
    sample launch one per (list with rows, 32 queries): the plan's own counts tell the width."""
    nq, lengths = WIDTH_NQ, WIDTH_LENGTHS
    nlist, n = len(lengths), sum(lengths)
    for form, metric in ((2, L2), (2, other_metric(d // 64)), (3, L2)):
        rng = np.random.default_rng(d + form)
        centers = rng.standard_normal((nlist, d), dtype=F)
        home = np.repeat(np.arange(nlist), lengths)
        rng.shuffle(home)
        x = (centers[home] + F(0.3) * rng.standard_normal((n, d), dtype=F)).astype(F)
        long_list = np.flatnonzero(home == 3)
        x[long_list[-100:]] = x[long_list[:100]]  # ties inside the long list
        q = (centers[rng.integers(1, nlist, nq)] + F(0.3) * rng.standard_normal((nq, d), dtype=F)).astype(F)
        centers[0] = F(50) * rng.standard_normal(d, dtype=F) if metric == L2 else F(0)  # the list no row goes to
        force_form(opt, form, metric)
        ix = build_ivf(x, metric, centers)
        assert shadow_form(ix) == form
        got = np.diff(ix.export()[1]).tolist()
        assert got == lengths, "the lists have the chosen lengths: %s" % got
        opt("ivf_pass", "2")
        opt("h16_preprune", "0")
        opt("h16_prune", "0")
        oi, od = oracle_on_exported(ix, q, nlist, 10, metric)
        p0 = capi.prefilter_stats()
        ids, dis = ix.search(q, 10, "nprobe=%d" % nlist)
        assert capi.prefilter_stats()[0] - p0[0] == nq, "the shadow list scan did not run"
        main, sb, sample = plan_items()
        same(ids, dis, oi, od, "d=%d form=%d %s" % (d, form, NAME[metric]))
        ncb = WIDTH[d][form]
        print("d=%d form=%d %s: %d main items (segments of %d blocks), %d sample items, ncb %d" % (d, form, NAME[metric], main, sb, sample, ncb))
        assert sample == sum(1 for l in got if l) * ceil_div(nq, 32), "the sample launch: one item per (list with rows, 32 queries)"
        segments = sum(plan_nseg(ceil_div(max(l - H_ROWS, 0), H_ROWS), sb) for l in got)  # of the rows behind every list's block 0
        assert main == segments * ceil_div(nq, 32 * ncb), "%d main items over %d segments: not tiles of %d queries" % (main, segments, 32 * ncb)
        for knob in ("ivf_pass", "h16_preprune", "h16_prune"):
            opt(knob, None)
        ix.close()


# ---------------------------------------------------------------------------------------- c. coarse shadow, list scan without one

@gpu
@pytest.mark.parametrize("metric", [L2, COS, IP])
def test_coarse_shadow_in_front_of_a_list_scan_without_one(metric, opt):
    """d = 2560, 256 lists, 200 queries: the coarse quantiser runs over the fp16 centroid shadow (coarse_stats counts the queries),
    leaves its words to the pre-pruning, and the list scan is the split-bf16 candidate pass -- the shadow list scan the words were
    written for cannot hold a query tile.  Host and device entry, with the pre-pruning and without (an inner-product index has
    none either way).  (Measured on an MI355X: the pre-pruning keeps one probe of eight per query; 149 of the 200 L2 queries and
    110 of the cosine ones miss the split-bf16 pass's certificate on these blobs and are served, exactly, by its canonical
    fallback -- a cost, not an error, and not asserted.)"""
    m = MIXED
    d, nlist, n, nq, nprobe, k = (m[key] for key in ("d", "nlist", "n", "nq", "nprobe", "k"))
    centers, x, q = blobs(2560 + metric, n, d, nlist, nq)
    # (cosine: unit centroids beside the unit rows -- a centroid table far beyond every stored row goes without a shadow)
    ix = build_ivf(x, metric, o.normalize_rows(centers) if metric == COS else centers)
    assert shadow_form(ix) != 0
    oi, od = oracle_on_exported(ix, q, nprobe, k, metric)
    for preprune in (None, "0"):
        opt("h16_preprune", preprune)
        for entry in ("host", "device"):
            for debug in (None, "1"):  # the plain search first, then the same with the pre-pruning's record kept
                opt("coarse_prune_debug", debug)
                shadow_scan_on_record(nq)
                c0, p0 = capi.coarse_stats(), capi.prefilter_stats()
                ids, dis = ix.search(q, k, "nprobe=%d" % nprobe) if entry == "host" else device_search(ix, q, k, nprobe)
                c1, p1 = capi.coarse_stats(), capi.prefilter_stats()
                what = "%s h16_preprune=%s %s debug=%s" % (NAME[metric], preprune, entry, debug)
                same(ids, dis, oi, od, what)
                assert c1[0] - c0[0] == nq, "%s: the coarse pass over the centroid shadow served %d queries" % (what, c1[0] - c0[0])
                assert p1[0] - p0[0] == nq, "%s: the candidate pass served %d queries" % (what, p1[0] - p0[0])
                assert not shadow_scan_on_record(nq), "%s: the shadow list scan ran" % what
                if debug and entry == "host":
                    have, probes, _, flags = capi.debug_prune_first(nq, nprobe)
                    assert have == (preprune is None and metric != IP), "%s: pre-pruning ran = %s" % (what, have)  # (L2 and cosine have one)
                    if have:
                        kept = (probes >= 0).sum(1)
                        assert (kept >= 1).all() and kept.mean() < nprobe, "the pre-pruning dropped nothing on clustered data"
                        print("%s: %.2f of %d probes kept, %d queries pruned first" % (what, kept.mean(), nprobe, int((flags & 1).sum())))
                print("%s: coarse fallbacks %d, result fallbacks %d" % (what, c1[1] - c0[1], p1[1] - p0[1]))
    ix.close()


# ---------------------------------------------------------------------------------------- d. canonical tile halving

FILTERED = {(1948, 10), (3996, 10), (4000, 10), (8192, 10), (5636, 256)}  # one per tile and kernel


@gpu
@pytest.mark.parametrize("d,k,T", HALVING)
def test_canonical_tile_halving(d, k, T, opt, calls):
    """The canonical scans with every candidate pass off: msvs_knn_f32, the FLAT index and IVFFLAT, 17 queries (17 x 4 pairs on 4
    lists: the planners ask for tiles of 8), on both sides of every halving.  k = 256 exceeds every probed list (~175 rows).
    The tile each planner chose is read back (msvs_debug_planned_tiles) and, for IVFFLAT, the kernel behind it is told by the
    grouping plan's scope: "ivf_plan" runs in front of the list-batched kernel only, never in front of ivf_scan_kernel (T = 1)."""
    i = HALVING.index((d, k, T))
    nq, nlist, n = HALVING_NQ, HALVING_NLIST, 700
    centers, x, q = blobs(d + k, n, d, nlist, nq)
    alive = np.random.default_rng(d).random(n) < 0.6 if (d, k) in FILTERED else None
    opt("ivf_pass", "0")
    opt("flat_mfma", "0")
    opt("flat_few", "0")
    opt("h16_preprune", "0")  # (its launch shares the grouping plan's scope, "ivf_plan")
    scopes = ("flat_scan", "ivf_scan", "ivf_plan", "flat_pass", "flat_shadow_scan", "lat_search")
    assert flat_T(nq, d, k) == T and ivf_T(nq * nlist, nlist, d, k) == T
    for metric in (L2, IP):
        for a in (None, alive) if alive is not None else (None,):
            planned_tiles()
            (ids, dis), c = calls(scopes, lambda: capi.knn(q, x, k, metric, alive=a))
            same(ids, dis, *o.knn(q, x, k, OM[metric], alive=a), what="knn %s d=%d k=%d" % (NAME[metric], d, k))
            assert c["flat_scan"] == 1 and c["flat_pass"] == 0, c
            assert planned_tiles()[0] == T, "knn %s d=%d k=%d: not the tile of %d queries" % (NAME[metric], d, k, T)
    for metric in (L2, other_metric(i)):
        ix = build_flat(x, metric)
        for a in (None, alive) if alive is not None else (None,):
            p0 = capi.prefilter_stats()
            planned_tiles()
            (ids, dis), c = calls(scopes, lambda: ix.search(q, k, "", alive=a))
            same(ids, dis, *oracle_flat(ix, q, k, metric, a), what="FLAT %s d=%d k=%d" % (NAME[metric], d, k))
            assert c["flat_scan"] >= 1 and c["flat_pass"] == 0 and c["flat_shadow_scan"] == 0, c
            assert capi.prefilter_stats()[0] == p0[0]
            assert planned_tiles()[0] == T, "FLAT %s d=%d k=%d: not the tile of %d queries" % (NAME[metric], d, k, T)
        ix.close()
    for metric in (L2, other_metric(i + 1)):
        ix = build_ivf(x, metric, centers)
        assert np.diff(ix.export()[1]).max() < 256
        for a in (None, alive) if alive is not None else (None,):
            p0 = capi.prefilter_stats()
            planned_tiles()
            (ids, dis), c = calls(scopes, lambda: ix.search(q, k, "nprobe=%d" % nlist, alive=a))
            what = "IVFFLAT %s d=%d k=%d%s" % (NAME[metric], d, k, "" if a is None else " filtered")
            same(ids, dis, *oracle_on_exported(ix, q, nlist, k, metric, a), what=what)
            assert c["ivf_scan"] >= 1 and c["lat_search"] == 0, c
            assert capi.prefilter_stats()[0] == p0[0], "a candidate pass ran"
            assert planned_tiles()[1] == T, "%s: not the tile of %d queries" % (what, T)
            # one query a block is another kernel with no grouping plan in front of it
            assert (c["ivf_plan"] == 0) == (T == 1), "%s: T = %d with %d grouping plans" % (what, T, c["ivf_plan"])
        if k == 256:  # one probe: fewer rows than k, the results end in -1; 17 pairs on 4 lists ask for a tile of 4
            oi, od = oracle_on_exported(ix, q, 1, k, metric)
            assert (oi < 0).any()
            planned_tiles()
            same(*ix.search(q, k, "nprobe=1"), oi, od, what="IVFFLAT %s d=%d k=%d nprobe=1" % (NAME[metric], d, k))
            assert planned_tiles()[1] == ivf_T(nq, nlist, d, k)
        ix.close()


# ---------------------------------------------------------------------------------------- e. the few-query path

@gpu
@pytest.mark.parametrize("d", LAT_DIMS)
def test_few_query_path(d, opt, calls):
    """One and two queries through the host entry: where lat_shape's two LDS images fit 64 KiB the two-launch path serves the
    call ("lat_search" ran once), elsewhere the general path; the results are the oracle's either way and with lat_path = 0."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nlist = LAT_NLIST
    for metric in (L2, other_metric(LAT_DIMS.index(d))):
        centers, x, q = blobs(d + metric, 800, d, nlist, 2)
        ix = build_ivf(x, metric, centers)
        ran = set()
        for nq, k, nprobe in LAT:
            oi, od = oracle_on_exported(ix, q[:nq], nprobe, k, metric)
            want = lat_eligible(d, nlist, nq, k, nprobe, cus)
            what = "d=%d %s nq=%d k=%d nprobe=%d" % (d, NAME[metric], nq, k, nprobe)
            (ids, dis), c = calls(("lat_search",), lambda: ix.search(q[:nq], k, "nprobe=%d" % nprobe))
            same(ids, dis, oi, od, what)
            assert c["lat_search"] == (1 if want else 0), "%s: the few-query path ran %d times, eligible = %s" % (what, c["lat_search"], want)
            opt("lat_path", "0")
            (ids, dis), c = calls(("lat_search",), lambda: ix.search(q[:nq], k, "nprobe=%d" % nprobe))
            opt("lat_path", None)
            same(ids, dis, oi, od, what + " lat_path=0")
            assert c["lat_search"] == 0
            ran.add(want)
        if cus == MI355X_CUS:
            assert ran == ({True} if d == 2048 else {True, False})
        ix.close()


# ---------------------------------------------------------------------------------------- f. the FLAT index's shadow passes

@gpu
@pytest.mark.parametrize("d", sorted(FLAT_SHADOW))
def test_flat_index_shadow_passes(d, opt, calls):
    """The few-query form (flat_few = 2, three queries) and the batch form (200 queries over 4800 rows) of the FLAT index's fp16
    shadow pass: at d = 2432 both run ("flat_shadow_scan"), at 2496 a tile of 32 queries no longer fits and neither does."""
    n, k = 4800, 10
    for metric in (L2, other_metric(d // 64)):
        _, x, q = blobs(d + metric, n, d, 8, 200)
        ix = build_flat(x, metric)
        assert shadow_form(ix) == 2
        for nq, knob in ((3, "2"), (200, None)):
            opt("flat_few", knob)
            oi, od = oracle_flat(ix, q[:nq], k, metric)
            (ids, dis), c = calls(("flat_shadow_scan", "flat_scan"), lambda: ix.search(q[:nq], k, ""))
            what = "FLAT %s d=%d nq=%d" % (NAME[metric], d, nq)
            same(ids, dis, oi, od, what)
            assert (c["flat_shadow_scan"] >= 1) == FLAT_SHADOW[d], "%s: %s" % (what, c)
            print(what, c)
        opt("flat_few", None)
        ix.close()


# ---------------------------------------------------------------------------------------- g. the limit itself

def code_of(fn):
    with pytest.raises(capi.MsvsError) as e:
        fn()
    return e.value.code


def error_of(fn):
    """-> (code, the library's message)"""
    with pytest.raises(capi.MsvsError) as e:
        fn()
    return e.value.code, str(e.value)


@gpu
@pytest.mark.parametrize("d", [8191, 8192])
def test_normalize_and_resident_blocks_at_the_limit(d):
    rng = np.random.default_rng(d)
    n, nq, k = 600, 5, 10
    _, x, q = blobs(d, n, d, 4, nq)
    x[7] = 0  # below the epsilon: left alone
    a, b = capi.normalize(x[:40]), o.normalize_rows(x[:40])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    cache = capi.Cache(128 << 20)
    raw, unit = cache.upload("large/raw", 0, x), cache.upload("large/unit", 0, x, normalize=True)
    alive = rng.random(n) < 0.5
    for metric in (L2, IP):
        same(*capi.knn_resident(raw, q, k, metric, d), *o.knn(q, x, k, OM[metric]), what="resident %s" % NAME[metric])
        same(*capi.knn_resident(raw, q, MAX_K, metric, d, alive=alive), *o.knn(q, x, MAX_K, OM[metric], alive=alive), what="resident, filtered")
    qn = o.normalize_rows(q)
    same(*capi.knn_resident(unit, qn, k, IP, d), *o.knn(qn, o.normalize_rows(x), k, o.METRIC_IP), what="normalised block")
    cache.release(raw)
    cache.release(unit)
    cache.close()


@gpu
@pytest.mark.parametrize("placement", [capi.ROWS_DEVICE, capi.ROWS_HOST_PINNED])
@pytest.mark.parametrize("d", [8191, 8192])
def test_refine_at_the_limit(d, placement):
    from test_refine import device_refine, ref_refine, store_of
    rng = np.random.default_rng(d + placement)
    n, nq = 1100, 3
    _, x, q = blobs(d + 1, n, d, 4, nq)
    cand = np.stack([rng.permutation(n)[:1024] for _ in range(nq)]).astype(np.int64)
    for i, (kc, k) in enumerate(((10, 10), (1024, 256), (1024, 10))):
        metric = (L2, IP, COS)[(i + d + placement) % 3]
        rows = store_of(x, metric, placement)
        c = np.ascontiguousarray(cand[:, :kc])
        want = ref_refine(x, q, c, k, metric)
        same(*capi.refine(rows, metric, q, c, k), *want, what="refine %s kc=%d" % (NAME[metric], kc))
        same(*device_refine(rows, metric, q, c, k), *want, what="refine_device %s kc=%d" % (NAME[metric], kc))
        rows.close()


@gpu
@pytest.mark.parametrize("d,m", [(8191, 1), (8192, 64)])
def test_search_refine_of_an_ivfpq_index_at_the_limit(d, m):
    """8191 is prime: one sub-quantiser of 8191 dimensions."""
    import test_pq_ivf as pq
    from test_refine import ref_refine, store_of
    rng = np.random.default_rng(d)
    n, nq, nlist = 600, 5, 4
    for metric in (L2, other_metric(d)):
        centres, x = pq.blobs(rng, n, d, nlist)
        q = (x[:nq] + F(0.1)).astype(F)
        ix = capi.PqIndex(metric, d, "m=%d" % m)
        ix.set_codebook(centres, pq.random_codebooks(rng, m, d // m))
        ix.add(x)  # labels are the staging positions: row i of the store
        ix.build()
        exp = ix.export()
        first = ix.search(q, 100, "nprobe=%d" % nlist)
        pq.same(first, pq.ref_search(exp, pq.decoded(exp), q, nlist, 100, metric))
        rows = store_of(x, metric)
        got = ix.search_refine(rows, q, 10, 100, "nprobe=%d" % nlist)
        same(*got, *ref_refine(x, q, first[0], 10, metric), what="search_refine %s d=%d" % (NAME[metric], d))
        rows.close()
        ix.close()


@gpu
def test_index_files_at_the_limit_and_a_header_beyond_it():
    import test_coded_index_files as cf
    d, n, nlist, nq, k = MAX_DIM, 300, 4, 5, 10
    centers, x, q = blobs(81, n, d, nlist, nq)
    for typ in (capi.INDEX_FLAT, capi.INDEX_IVFFLAT):
        ix = build_flat(x, L2) if typ == capi.INDEX_FLAT else build_ivf(x, L2, centers)
        params = "" if typ == capi.INDEX_FLAT else "nprobe=2"
        want = ix.search(q, k, params)
        ref = oracle_flat(ix, q, k, L2) if typ == capi.INDEX_FLAT else oracle_on_exported(ix, q, 2, k, L2)
        same(*want, *ref, what="before the round trip")
        store = {}
        ix.serialize_io(store)
        ix.close()
        ld = capi.Index.load_io(store, typ, L2, d)
        same(*ld.search(q, k, params), *ref, what="after the round trip")
        ld.close()
        head = bytes(store["data_bin"][:56])
        assert head[:8] == b"MSVSIDX2" and struct.unpack_from("<Q", head, 32)[0] == d  # DataHeader: dim behind six 32-bit words
        store["data_bin"][32:40] = struct.pack("<Q", d + 1)
        # the header check itself refuses it: a loader that read on would meet shifted offsets and fail with another message
        code, msg = error_of(lambda: capi.Index.load_io(store, typ, L2, d + 1))
        assert code == capi.ERR_IO and "corrupt msvs index header" in msg, msg
    # the coded indexes' loader (header_ranges_ok): the same header with dim = 8193 and a fresh checksum
    rng = np.random.default_rng(82)
    ix = capi.PqIndex(L2, d, "m=64")
    ix.set_codebook(centers, (F(0.5) * rng.standard_normal((64, 256, d // 64), dtype=F)).astype(F))
    ix.add(x)
    ix.build()
    store = {}
    ix.serialize_io(store)
    ix.close()
    head = bytes(store["pq_data"][:56])
    assert head[:8] == b"MSVSPQ01" and struct.unpack_from("<Q", head, 16)[0] == d and bytes(store["pq_data"][:64]) == cf.with_check(head)
    capi.PqIndex.load_io(store, L2, d, 64).close()
    store["pq_data"][:64] = cf.with_check(head[:16] + struct.pack("<Q", d + 1) + head[24:])
    code, msg = error_of(lambda: capi.PqIndex.load_io(store))
    assert code == capi.ERR_IO and "corrupt msvs IVFPQ index header" in msg, msg  # (magic, version and checksum are right: the range is not)


@gpu
def test_dimensions_beyond_the_limit_are_refused():
    d = MAX_DIM + 1
    for typ, params in ((capi.INDEX_FLAT, ""), (capi.INDEX_IVFFLAT, "ncentroids=4")):
        assert code_of(lambda: capi.Index(typ, L2, d, params)) == capi.ERR_INVALID_ARGUMENT
        capi.Index(typ, L2, MAX_DIM, params).close()
    assert code_of(lambda: capi.Rows(d, 10)) == capi.ERR_INVALID_ARGUMENT
    capi.Rows(MAX_DIM, 10).close()
    cache = capi.Cache(1 << 20)
    assert code_of(lambda: cache.upload("too/wide", 0, np.zeros((1, d), F))) == capi.ERR_INVALID_ARGUMENT
    cache.close()
    assert code_of(lambda: capi.PqIndex(L2, d, "m=1")) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.PqIndex(L2, MAX_DIM, "m=128")) == capi.ERR_INVALID_ARGUMENT  # 128 KiB of tables beside 64 KiB of staging
    capi.PqIndex(L2, MAX_DIM, "m=64").close()
    capi.PqIndex(L2, MAX_DIM, "m=256,bit_size=4").close()
    capi.SqIndex(L2, 2240).close()
    assert code_of(lambda: capi.SqIndex(L2, 2241)) == capi.ERR_INVALID_ARGUMENT  # ld = 2256: 65600 bytes for the smallest tile


# ---------------------------------------------------------------------------------------- h. IVFPQ at the top

@gpu
@pytest.mark.parametrize("bits,dim,m,form", sorted(PQ_TOP))
def test_ivfpq_at_the_top(bits, dim, m, form):
    """The largest admitted shapes, over a codebook set by hand: ~600 rows in 4 lists, the codes of every ninth row (every position
    of the encoder's 8-row blocks) against the reference encoder, and a batch of 40 queries x 4 probes (a tile of 8 by the pairs;
    1 or 2 by the LDS) at k = 256, whose first ten are the k = 10 search.  dim 8192 makes the 8-bit encoder raise its LDS attribute,
    8184 is the last dimension that does not.  The scan's tile is not observable on the device: which tile each shape takes is
    asserted from the restated formula alone (test_case_tables_land_on_the_intended_side_of_every_switch); here the results are."""
    import test_pq_ivf as pq
    import test_pq_query_tables as qt
    rng = np.random.default_rng(bits * 1000 + dim + m + form)
    n, nlist, nq = 600, PQ_NLIST, PQ_NQ
    for metric in (L2, other_metric(m + form)):
        centres, x = pq.blobs(rng, n, dim, nlist)
        x[-60:] = x[:60]  # ties
        cb = (F(0.5) * rng.standard_normal((m, 1 << bits, dim // m), dtype=F)).astype(F)
        ix = capi.PqIndex(metric, dim, "m=%d,bit_size=%d%s" % (m, bits, ",query_tables=1" if form else ""))
        assert ix.bits == bits and ix.query_tables == form
        ix.set_codebook(centres, cb)
        ix.add(x[:301])
        ix.add(x[301:])
        ix.build()
        exp = ix.export()
        cent, cb2, off, codes, labels = exp
        assert cb2.tobytes() == cb.tobytes() and codes.shape == (n, m) and (np.diff(off) > 0).all()
        pick = np.arange(0, n, 9)
        xs = pq.stored(x, metric)[labels[pick]]
        assert (codes[pick] == pq.encode(xs, cent[pq.lists_of(off)[pick]], cb)).all(), "codes differ from the reference encoder"
        q = (x[:nq] + F(0.1)).astype(F)
        ref = qt.ref_search(exp, q, nlist, MAX_K, metric) if form else pq.ref_search(exp, pq.decoded(exp), q, nlist, MAX_K, metric)
        pq.same(ix.search(q, MAX_K, "nprobe=%d" % nlist), ref)
        pq.same(pq.device_search(ix, q, 10, nlist), (ref[0][:, :10], ref[1][:, :10]))
        ix.close()


# ---------------------------------------------------------------------------------------- i. build

@gpu
@pytest.mark.parametrize("metric", [L2, IP])
def test_train_and_add_at_the_limit(metric):
    """train + add of 600 integer-valued rows of 8192 dimensions in 8 lists against ivf_build_ref: the seeds, one Lloyd step to the
    bit, and every row in the list of its nearest centroid."""
    import ivf_build_ref as R
    from test_ivf_build import SEED, trained
    n, d, nlist = 600, MAX_DIM, 8
    x = R.int_rows(np.random.default_rng(8), n, d, -8, 8)
    c0, stored, lists0, ix = trained(metric, x, nlist, 0)
    ix.close()
    assert (stored == x).all()
    xs = stored[R.train_sample(n, n, SEED)]
    R.check_bit_equal(c0, xs[:nlist])
    R.check_exact(lists0, R.exact_assign(x, c0, metric == IP))  # integer seeds: the assignment of add() is exact
    want1, cnt1, touched1 = R.lloyd_step(xs, c0)
    assert (cnt1 > 0).all() and not touched1.any()
    c1, stored1, lists1, ix = trained(metric, x, nlist, 1)
    R.check_bit_equal(c1, want1)
    R.check_float_assign(lists1, stored1, c1, metric != L2)
    q = (x[:5] + F(0.25)).astype(F)
    same(*ix.search(q, 10, "nprobe=3"), *oracle_on_exported(ix, q, 3, 10, metric), what="search after the build")
    ix.close()
