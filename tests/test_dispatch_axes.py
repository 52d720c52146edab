"""Every axis of the launchers' run-time -> template dispatch (csrc/dispatch.hpp), walked at the smallest shapes that reach it: metric,
query tile T, top-k class R (k <= 64 / <= 128 / > 128), lanes per row G of the binary kernels.  A value sent to a neighbouring
instantiation can pass a parity test when the neighbour copes, so each case here is meant to land in ONE instantiation; which ones a
run reached is read off a kernel trace of this file.  Public API and existing knobs only; every search is compared with the oracle:
ids ==, distances by their uint32 view."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_bin_ivf as bi
import test_pq_ivf as pq
import test_sq_ivf as sq
from oracle import oracle as o

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP = capi.METRIC_L2, capi.METRIC_IP
OM = {L2: o.METRIC_L2, IP: o.METRIC_IP}
KS = [10, 100, 200]  # R = 1, 2, 4
N, D, NLIST, NPROBE = 2000, 24, 8, 4


def same(got, exp):
    (gi, gd), (ei, ed) = got, exp
    assert gi.shape == ei.shape
    assert (gi == ei).all(), np.argwhere(gi != ei)[:5]
    assert (gd.view(np.uint32) == ed.view(np.uint32)).all(), np.argwhere(gd.view(np.uint32) != ed.view(np.uint32))[:5]


@functools.lru_cache(maxsize=None)
def float_data():
    rng = np.random.default_rng(2024)
    centres = (2 * rng.standard_normal((NLIST, D), dtype=F)).astype(F)
    x = (centres[rng.integers(0, NLIST, N)] + rng.standard_normal((N, D), dtype=F)).astype(F)
    q = (centres[rng.integers(0, NLIST, 40)] + rng.standard_normal((40, D), dtype=F)).astype(F)
    return x, q


# ---------------------------------------------------------------------------------------- IVFFLAT: canonical list scans

@functools.lru_cache(maxsize=None)
def ivf_case(metric):
    x, q = float_data()
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, D, "ncentroids=%d,kmeans_iters=4" % NLIST)
    ix.train(x)
    ix.add(x)
    ix.build()
    cent, off, vecs, lids = ix.export()
    refs = {nq: o.ivf_search(cent, off, vecs, lids, q[:nq], NPROBE, max(KS), OM[metric])[:2] for nq in (40, 5)}
    return ix, q, refs


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_ivfflat_tile_and_k_class(metric, k, opt):
    """ivf_batched_scan_kernel<METRIC, T, R> for T in {2, 4, 8} (option ivf_t) over 40 queries; 5 queries with one query per block
    (ivf_t = 1: the planner itself takes it below one pair per list), ivf_scan_kernel<METRIC, R>; ivf_merge_kernel<METRIC, R> behind
    both."""
    ix, q, refs = ivf_case(metric)
    opt("ivf_pass", "0")
    opt("lat_path", "0")
    oi, od = refs[40]
    for t in (2, 4, 8):
        assert t * (D // 4) * 16 + t * 40 * k <= 160 * 1024  # scan_lds_bytes: the launcher takes the tile the knob sets
        opt("ivf_t", str(t))
        same(ix.search(q, k, "nprobe=%d" % NPROBE), (oi[:, :k], od[:, :k]))
    opt("ivf_t", "1")
    oi, od = refs[5]
    same(ix.search(q[:5], k, "nprobe=%d" % NPROBE), (oi[:, :k], od[:, :k]))


# ---------------------------------------------------------------------------------------- FLAT: exhaustive canonical scan

@functools.lru_cache(maxsize=None)
def flat_case(metric):
    x, q = float_data()
    ix = capi.Index(capi.INDEX_FLAT, metric, D)
    ix.add(x)
    ix.build()
    return ix, q, o.knn(q[:9], x, max(KS), OM[metric])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_flat_tile_and_k_class(metric, k, opt):
    """flat_scan_kernel<METRIC, T, R>: 1, 2, 4 and 9 queries take T = 1, 2, 4, 8; merge_kernel<METRIC, R> behind it."""
    ix, q, (oi, od) = flat_case(metric)
    opt("flat_mfma", "0")
    for nq, t in ((1, 1), (2, 2), (4, 4), (9, 8)):
        assert t * (D // 4) * 16 + t * 40 * k <= 64 * 1024  # plan_flat: T by nq, not halved while scan_lds_bytes fits 64 KiB
        same(ix.search(q[:nq], k), (oi[:nq, :k], od[:nq, :k]))


# ---------------------------------------------------------------------------------------- binary: lanes per row

BIN_N, BIN_NLIST, BIN_NQ = 1500, 8, 20


@functools.lru_cache(maxsize=None)
def bin_case(metric, nbytes):
    rng = np.random.default_rng(nbytes * 3 + metric)
    centres = rng.integers(0, 256, (BIN_NLIST, nbytes), dtype=np.uint8)
    rows = bi.flip_noise(rng, centres, BIN_N)
    labels = rng.permutation(2 * BIN_N)[:BIN_N].astype(np.int64)
    q = bi.flip_noise(rng, centres, BIN_NQ, 0.15)
    flat = capi.BinIndex(nbytes, metric)
    flat.add(rows, labels)
    ivf = capi.BinIndex(nbytes, metric, "ncentroids=%d" % BIN_NLIST)
    ivf.set_centroids(centres)
    ivf.add(rows, labels)
    rows_s, labels_s, lists_s = bi.by_label(rows, labels, centres)
    fi, fd = o.knn_bin(q, rows_s, 100, bi.OM[metric])
    return flat, ivf, q, (labels_s[fi], fd), bi.ref_search(q, centres, rows_s, labels_s, lists_s, NPROBE, 100, metric)


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nbytes", [16, 32, 48, 64, 128, 256])  # G = 1, 2, 2, 4, 8, 16 lanes per row; 48: not in G registers (REG false)
@pytest.mark.parametrize("metric", [capi.METRIC_HAMMING, capi.METRIC_JACCARD])
def test_binary_lanes_and_k_class(metric, nbytes, k):
    """bin_scan_kernel<METRIC, G, R> (flat), bin_assign_kernel<G> and bin_ivf_scan_kernel<METRIC, G, T, R, REG> (partitioned): R = 1
    with tiles of 8 queries up to k = 64, R = 4 with tiles of 4 beyond."""
    flat, ivf, q, (fi, fd), (ri, rd) = bin_case(metric, nbytes)
    ids, dis = flat.search(q, k)
    bi.same(ids, dis, fi[:, :k], fd[:, :k])
    ids, dis = ivf.search(q, k, params="nprobe=%d" % NPROBE)
    bi.same(ids, dis, ri[:, :k], rd[:, :k])


# ---------------------------------------------------------------------------------------- IVFSQ, IVFPQ: tile by pairs per list

# pairs = nq * nprobe over 8 lists: tile 8 from 128 pairs, 4 from 16, 2 below (IVFSQ) or from 8, and (IVFPQ only) 1 below 8; at 5
# dimensions every tile fits its LDS budget up to k = 200
TILE_NQ = {1: 1, 2: 3, 4: 9, 8: 40}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_sq_tile_and_k_class(metric, k):
    """sq_ivf_scan_kernel<METRIC, T, R>, T in {2, 4, 8}: a single query has no tile of its own and takes T = 2."""
    ix, exp, xh, _, _, q = sq.case(metric, 5, "clustered")
    for t in (1, 2, 4, 8):
        nq = TILE_NQ[t]
        assert (max(t, 2) + 3) * 2 * 16 + max(t, 2) * 40 * k <= 64 * 1024  # sq_lds_bytes at ld4 = 2: the tile is not halved
        sq.same(ix.search(q[:nq], k, "nprobe=%d" % NPROBE), sq.ref_search(exp, xh, q[:nq], NPROBE, k, metric))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_pq_tile_and_k_class(metric, k):
    """pq_ivf_scan_kernel<METRIC, T, R>, T in {1, 2, 4, 8}."""
    ix, exp, xh, _, _, q = pq.case(metric, 5, 5, "clustered")
    for t in (1, 2, 4, 8):
        nq = TILE_NQ[t]
        assert pq.tile_class(5, 5, nq, k, NPROBE) == (t, 1 if k <= 64 else 2 if k <= 128 else 4)
        pq.same(ix.search(q[:nq], k, "nprobe=%d" % NPROBE), pq.ref_search(exp, xh, q[:nq], NPROBE, k, metric))
