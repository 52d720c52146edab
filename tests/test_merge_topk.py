"""msvs_merge_topk, msvs_merge_topk_device and msvs_merge_topk_device_strided against the sort reference of test_merge_topk_host.py,
at every boundary between the three code paths the size alone picks (shard.hip: merge_topk_device):
  nparts * k <= 256    merge_small_kernel, one wavefront per query (option merge_small=0 switches it off);
  <= 6144 keys         pack_keys_kernel + merge_kernel's heads merge, which walks the heads of SORTED lists;
  above                pack_keys_kernel + merge_kernel's WaveTopK<R> threshold pass and block_rank_merge, R = 1, 2, 4 for k <= 64, 128, 256.
Every list handed to the heads path is in canonical order with its holes at the end (the precondition msvs.h states); ids compare
with ==, distances on their uint32 view."""
import ctypes as C

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_merge_topk_host as mh
from test_merge_topk_host import IP, L2, METRICS, F, make_parts, neutral, reference_merge, same

pytestmark = pytest.mark.gpu

NQS = (1, 3, 4, 5, 9)  # the small kernel puts four queries in a block
SMALL = [(1, 1), (1, 256), (4, 64), (256, 1), (2, 100), (3, 85)]
ABOVE_SMALL = [(257, 1), (3, 86), (5, 52), (2, 129)]
HEADS = [(24, 256), (96, 64), (48, 128), (6144, 1), (70, 63), (47, 129)]
ABOVE_HEADS = [(6145, 1), (25, 256), (48, 129), (49, 128), (96, 65), (97, 64), (100, 63)]  # R = 1 | 4, 4 | 2, 2 | 1, 1
ALL_SHAPES = SMALL + ABOVE_SMALL + HEADS + ABOVE_HEADS
PATHS = {"small": (3, 85), "heads": (70, 63), "above": (48, 129)}  # one shape on each path for the input models


def nq_of(nparts, k):
    return NQS[ALL_SHAPES.index((nparts, k)) % len(NQS)]


def test_shapes_sit_where_the_paths_change():
    assert all(p * k <= 256 for p, k in SMALL) and sum(p * k == 256 for p, k in SMALL) >= 3
    assert all(256 < p * k <= 6144 for p, k in ABOVE_SMALL + HEADS) and min(p * k for p, k in ABOVE_SMALL) == 257
    assert sum(p * k == 6144 for p, k in HEADS) >= 4 and all(p * k > 6144 for p, k in ABOVE_HEADS) and (6145, 1) in ABOVE_HEADS
    assert {(k > 64) + (k > 128) for _, k in ABOVE_HEADS} == {0, 1, 2}  # every R
    assert {nq_of(p, k) for p, k in SMALL} == set(NQS)


# ---------------------------------------------------------------------------------------- the entries

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_rc(ids, dis, metric, nparts=None, nq=None, k=None, out=None):
    """msvs_merge_topk_device on [nparts, nq, k] arrays -> (return code, ids [nq, k], dis [nq, k])"""
    import torch
    P, Q, K = ids.shape
    nparts, nq, k = P if nparts is None else nparts, Q if nq is None else nq, K if k is None else k
    di, dd = _dev(ids), _dev(dis)
    oi, od = out if out is not None else (torch.full((nq, k), 77, dtype=torch.int64, device="cuda"),
                                          torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    rc = capi.lib().msvs_merge_topk_device(C.c_void_p(di.data_ptr()), C.c_void_p(dd.data_ptr()), C.c_size_t(nparts), C.c_size_t(nq),
                                           C.c_size_t(k), int(metric), C.c_void_p(oi.data_ptr()), C.c_void_p(od.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, oi.cpu().numpy(), od.cpu().numpy()


def device_merge(ids, dis, metric):
    rc, oi, od = device_rc(ids, dis, metric)
    capi._check(rc)
    return oi, od


def strided_rc(ids, dis, metric, part_bytes=None, ids_stride=None, dis_stride=None, nparts=None):
    """msvs_merge_topk_device_strided over the packed exchange layout: part p's {ids[nq * k] i64 | dis[nq * k] f32} at byte
    p * part_bytes (default: nq * k * 12 rounded up to 8, PackedExchange's); strides in elements."""
    import torch
    P, nq, k = ids.shape
    n = nq * k
    part_bytes = (n * 12 + 7) // 8 * 8 if part_bytes is None else part_bytes
    buf = np.full(P * part_bytes + 8, 0xA5, np.uint8)  # (filler a merge must not read as an entry: id 0xA5A5..., negative)
    for p in range(P):
        buf[p * part_bytes:p * part_bytes + n * 8] = ids[p].reshape(-1).view(np.uint8)
        buf[p * part_bytes + n * 8:p * part_bytes + n * 12] = dis[p].reshape(-1).view(np.uint8)
    g = _dev(buf)
    oi = torch.full((nq, k), 77, dtype=torch.int64, device="cuda")
    od = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = capi.lib().msvs_merge_topk_device_strided(
        C.c_void_p(g.data_ptr()), C.c_size_t(part_bytes // 8 if ids_stride is None else ids_stride), C.c_void_p(g.data_ptr() + n * 8),
        C.c_size_t(part_bytes // 4 if dis_stride is None else dis_stride), C.c_size_t(P if nparts is None else nparts), C.c_size_t(nq),
        C.c_size_t(k), int(metric), C.c_void_p(oi.data_ptr()), C.c_void_p(od.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, oi.cpu().numpy(), od.cpu().numpy()


def strided_merge(ids, dis, metric, part_bytes=None):
    rc, oi, od = strided_rc(ids, dis, metric, part_bytes)
    capi._check(rc)
    return oi, od


def host_rc(ids, dis, nparts, nq, k, metric, oi, od):
    """msvs_merge_topk (host pointers) -> return code"""
    return capi.lib().msvs_merge_topk(capi._p(ids, C.c_int64), capi._p(dis, C.c_float), C.c_size_t(nparts), C.c_size_t(nq), C.c_size_t(k),
                                      int(metric), capi._p(oi, C.c_int64), capi._p(od, C.c_float))


ENTRIES = {"host_pointers": capi.merge_topk, "device": device_merge, "strided": strided_merge}


# ---------------------------------------------------------------------------------------- shapes

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nparts,k", ALL_SHAPES)
def test_every_path_boundary_matches_the_reference(nparts, k, metric):
    """Ties between ids, the same (dis, id) in several parts and lists of every length at each shape; the device entry at all of
    them, the other two entries in turn."""
    nq = nq_of(nparts, k)
    ids, dis = make_parts("mixed", nparts, nq, k, metric)
    ref = reference_merge(ids, dis, metric)
    same(*device_merge(ids, dis, metric), *ref, what="device")
    other = ("host_pointers", "strided")[ALL_SHAPES.index((nparts, k)) % 2]
    same(*ENTRIES[other](ids, dis, metric), *ref, what=other)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nparts,k", SMALL)
def test_small_shapes_through_the_general_kernels(nparts, k, metric, opt):
    """merge_small=0: pack_keys_kernel + merge_kernel give the same bits as the one-wavefront kernel."""
    nq = nq_of(nparts, k)
    for model in ("mixed", "duplicates", "ragged"):
        ids, dis = make_parts(model, nparts, nq, k, metric)
        ref = reference_merge(ids, dis, metric)
        opt("merge_small", 0)
        general = device_merge(ids, dis, metric)
        opt("merge_small", 1)
        small = device_merge(ids, dis, metric)
        same(*general, *ref, what="%s merge_small=0" % model)
        same(*small, *ref, what="%s merge_small=1" % model)


@pytest.mark.parametrize("metric", METRICS)
def test_strided_form_on_padded_and_oversized_parts(metric):
    """The packed {ids | dis} layout of PackedExchange against the reference: nq * k odd (3 x 7: the part is padded to 8 bytes and
    the distances of part p start 4 bytes off an 8-byte boundary for odd p), and part strides larger than needed, on each path."""
    for nparts, nq, k, part_bytes in ((5, 3, 7, None), (36, 3, 7, None), (37, 3, 7, 3 * 7 * 12 + 20), (3, 5, 85, 5 * 85 * 12 + 1004),
                                      (70, 4, 63, 4 * 63 * 12 + 64), (880, 3, 7, None), (49, 1, 128, 49 * 128 * 12)):
        assert part_bytes is None or (part_bytes % 8 == 0 and part_bytes >= nq * k * 12)
        for model in ("mixed", "ragged"):
            ids, dis = make_parts(model, nparts, nq, k, metric)
            same(*strided_merge(ids, dis, metric, part_bytes), *reference_merge(ids, dis, metric),
                 what="%s %s" % (model, (nparts, nq, k, part_bytes)))


# ---------------------------------------------------------------------------------------- input models

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("model", mh.MODELS)
def test_input_models_on_each_path(model, path, metric):
    """distinct / ties / equal distances, duplicated keys, ragged, empty and short parts, subnormals, the infinity that comes first,
    NaN / the neutral value / the infinity beyond it with a valid id (dropped), ids 0 and 2^32 - 2: see make_parts."""
    nparts, k = PATHS[path]
    ids, dis = make_parts(model, nparts, 5, k, metric)
    ref = reference_merge(ids, dis, metric)
    for name, entry in ENTRIES.items():
        same(*entry(ids, dis, metric), *ref, what=name)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("path", list(PATHS) + ["general_small"])
def test_signed_zero_ties_and_the_id_decides(path, metric, opt):
    """-0 and +0 are one distance to the oracle's better(), so the id decides between them; an order on the key's bit pattern (f2ord)
    would put every -0 first.  The inputs hold (+0, id a) and (-0, id b) with the ids the way round that separates the two rules.
    Ids must be the reference's; distances compare BY VALUE here (the merge reports a -0 it took in as +0), everywhere else by bits.

    No search entry of the library writes -0, so the scans' make_key keeps its order on the bits: the canonical arithmetic
    (oracle/msvs_oracle.c: oracle_l2sqr, oracle_ip) starts each of its 64 accumulators at +0.0f and only adds to them; a
    round-to-nearest sum is -0 only when both addends are -0, so no accumulator and no node of the tree sum is -0 (L2 adds squares on
    top).  Cosine reports fl(1 - ip), and x - x is +0.  Every search path is held to those bits, with -0 queries and rows among the
    inputs, by test_special_values.py; h16_stream_cut (h16_scan_kernels.hpp) relies on the same fact for the L2 stream."""
    nparts, k = PATHS["small"] if path == "general_small" else PATHS[path]
    if path == "general_small":
        opt("merge_small", 0)
    ids, dis = mh.signed_zero_parts(nparts, 5, k, metric)
    ref = reference_merge(ids, dis, metric)
    for name, entry in ENTRIES.items():
        same(*entry(ids, dis, metric), *ref, what=name, by_value=True)


@pytest.mark.parametrize("metric", METRICS)
def test_unsorted_lists_on_the_order_free_paths(metric, opt):
    """merge_small_kernel ranks every key against every other and the path above 6144 keys selects by threshold: neither reads the
    order inside a list, and this test keeps it so.  (The heads path in between needs sorted lists -- msvs.h states the
    precondition -- and gets none here.)  The CPU form on the same inputs: test_merge_topk_host.py."""
    for nparts, k in (PATHS["small"], (1, 256), PATHS["above"], (97, 64), (49, 128)):
        for model in ("mixed", "nan", "ragged"):
            ids, dis = mh.shuffled(*make_parts(model, nparts, 5, k, metric))
            ref = reference_merge(ids, dis, metric)
            same(*device_merge(ids, dis, metric), *ref, what="device %s (%d, %d)" % (model, nparts, k))
            same(*mh.host.merge_topk(ids, dis, metric), *ref, what="host %s (%d, %d)" % (model, nparts, k))


# ---------------------------------------------------------------------------------------- properties

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nparts,k,group", [(4, 64, 2), (24, 256, 6), (97, 64, 25), (25, 256, 5), (6145, 1, 1000), (49, 128, 7)])
def test_two_levels_equal_one(nparts, k, group, metric):
    """Groups of parts merged first and their results merged again -- parts, then ranks -- give the one-level merge."""
    ids, dis = make_parts("mixed", nparts, 3, k, metric)
    ref = reference_merge(ids, dis, metric)
    level1 = [device_merge(ids[a:a + group], dis[a:a + group], metric) for a in range(0, nparts, group)]
    for (gi, gd), a in zip(level1, range(0, nparts, group)):
        same(gi, gd, *reference_merge(ids[a:a + group], dis[a:a + group], metric), what="group at %d" % a)
    li, ld = np.stack([g[0] for g in level1]), np.stack([g[1] for g in level1])
    same(*device_merge(li, ld, metric), *ref, what="second level")
    same(*device_merge(ids, dis, metric), *ref, what="one level")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [10, 100])
def test_merged_part_searches_equal_the_search_over_all_rows(k, metric):
    """4 parts of 300 rows, d = 8, searched one by one with global ids.  Disjoint parts: the merge is capi.knn over all rows.  With
    rows copied into two parts the merge keeps both copies: the reference merge of the four results."""
    rng = np.random.default_rng(11)
    x = (rng.integers(-8, 9, (1200, 8)) / 4).astype(F)  # (a coarse grid: equal distances between different rows)
    q = (rng.integers(-8, 9, (5, 8)) / 4).astype(F)

    def search_parts(rows_of_part):
        ids, dis = [], []
        for rows in rows_of_part:
            li, ld = capi.knn(q, x[rows], k, metric)
            ids.append(np.where(li >= 0, rows[np.maximum(li, 0)], -1))
            dis.append(ld)
        return np.stack(ids), np.stack(dis)

    disjoint = rng.permutation(1200).astype(np.int64).reshape(4, 300)
    disjoint.sort(axis=1)  # (ascending local index = ascending global id: a part's ties come out in global order)
    ids, dis = search_parts(disjoint)
    merged = device_merge(ids, dis, metric)
    same(*merged, *capi.knn(q, x, k, metric), what="disjoint parts against knn over all rows")
    same(*merged, *reference_merge(ids, dis, metric), what="disjoint parts against the reference")
    overlap = disjoint.copy()
    overlap[1, :150], overlap[3, 100:250] = disjoint[0, :150], disjoint[2, 5:155]
    overlap.sort(axis=1)
    ids, dis = search_parts(overlap)
    ref = reference_merge(ids, dis, metric)
    assert any(len(set(r)) < k for r in ref[0].tolist()), "a copied row must reach the merged lists"
    for name, entry in ENTRIES.items():
        same(*entry(ids, dis, metric), *ref, what="overlapping parts, " + name)


# ---------------------------------------------------------------------------------------- errors and limits

def _fresh(nq, k):
    return np.full((nq, k), 77, np.int64), np.full((nq, k), 7.0, F)


def test_cosine_is_not_implemented():
    ids, dis = make_parts("distinct", 2, 3, 4, L2)
    assert host_rc(ids, dis, 2, 3, 4, capi.METRIC_COSINE, *_fresh(3, 4)) == capi.ERR_NOT_IMPLEMENTED
    assert device_rc(ids, dis, capi.METRIC_COSINE)[0] == capi.ERR_NOT_IMPLEMENTED
    assert strided_rc(ids, dis, capi.METRIC_COSINE)[0] == capi.ERR_NOT_IMPLEMENTED


def test_k_above_256_is_unsupported():
    ids, dis = make_parts("distinct", 2, 3, 257, L2)
    assert host_rc(ids, dis, 2, 3, 257, L2, *_fresh(3, 257)) == capi.ERR_UNSUPPORTED_K
    assert device_rc(ids, dis, L2)[0] == capi.ERR_UNSUPPORTED_K
    assert strided_rc(ids, dis, IP)[0] == capi.ERR_UNSUPPORTED_K


def test_strided_refuses_a_stride_below_the_part():
    ids, dis = make_parts("distinct", 3, 3, 7, L2)
    assert strided_rc(ids, dis, L2, ids_stride=20)[0] == capi.ERR_INVALID_ARGUMENT
    assert strided_rc(ids, dis, L2, dis_stride=20)[0] == capi.ERR_INVALID_ARGUMENT
    rc, oi, od = strided_rc(ids[:1], dis[:1], L2, ids_stride=21, dis_stride=21)  # exactly nq * k
    assert rc == 0
    same(oi, od, *reference_merge(ids[:1], dis[:1], L2))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("small", [1, 0])
def test_no_queries_or_k_zero_is_a_no_op(small, metric, opt):
    opt("merge_small", small)
    ids, dis = make_parts("distinct", 2, 3, 4, metric)
    for nq, k in ((0, 4), (3, 0)):
        oi, od = _fresh(3, 4)
        assert host_rc(ids, dis, 2, nq, k, metric, oi, od) == 0 and (oi == 77).all() and (od == 7.0).all()
        rc, oi, od = device_rc(ids, dis, metric, nq=nq, k=k, out=(_dev(oi), _dev(od)))
        assert rc == 0 and (oi == 77).all() and (od == 7.0).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("small", [1, 0])
@pytest.mark.parametrize("entry", ["host_pointers", "device", "strided"])
def test_no_parts_writes_empty_slots(entry, small, metric, opt):
    """nparts = 0 with nq, k > 0: nq * k slots of id -1 at the neutral distance from every entry, with and without the small kernel
    (finding 5: msvs_merge_topk returned without writing its outputs)."""
    opt("merge_small", small)
    ids, dis = make_parts("distinct", 2, 3, 4, metric)
    if entry == "host_pointers":
        oi, od = _fresh(3, 4)
        rc = host_rc(None, None, 0, 3, 4, metric, oi, od)
    else:
        rc, oi, od = (device_rc if entry == "device" else strided_rc)(ids, dis, metric, nparts=0)
    assert rc == 0, capi.lib().msvs_last_error().decode()
    assert (oi == -1).all() and (od == neutral(metric)).all()


@pytest.mark.parametrize("metric", METRICS)
def test_host_pointer_form_refuses_ids_beyond_the_range(metric):
    """Merge ids lie in [0, 2^32 - 1) like every id of the library: the keys carry 32 bits.  msvs_merge_topk has its ids on the host
    and refuses a larger one (finding 1: it came back truncated); ids < 0 stay holes whatever their value; 2^32 - 2 passes."""
    ids, dis = make_parts("ties", 3, 4, 20, metric)
    for bad in (2 ** 32 - 1, 2 ** 32 + 5, 2 ** 40):
        big = ids.copy()
        big[1, 2, 3] = bad
        assert host_rc(big, dis, 3, 4, 20, metric, *_fresh(4, 20)) == capi.ERR_ID_RANGE, bad
    ok = ids.copy()
    ok[1, 2, 3], ok[2, 1, -1] = 2 ** 32 - 2, -2 ** 40
    ok, dis = mh.canonical(ok, dis, metric)
    same(*capi.merge_topk(ok, dis, metric), *reference_merge(ok, dis, metric))
