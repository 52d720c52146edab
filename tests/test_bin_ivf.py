"""The partitioned (IVF) binary index: k-majority centroids + list-major rows, searched by probing (msvs_bin_index_create_ivf
and friends).  Everything is integer popcounts, so every comparison is bit-exact.  The reference is composed here from the
oracle's knn_bin: probes = knn_bin(q, centroids, nprobe, Hamming); the rows of those lists, dead labels dropped, sorted by
label; knn_bin(q, rows, k, metric); indices mapped back to labels (the oracle breaks ties by index = by label)."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu
OM = {capi.METRIC_HAMMING: o.METRIC_HAMMING, capi.METRIC_JACCARD: o.METRIC_JACCARD}
FLT_MAX = np.finfo(np.float32).max


def same(a_ids, a_dis, b_ids, b_dis):
    assert a_ids.shape == b_ids.shape
    assert (a_ids == b_ids).all(), np.argwhere(a_ids != b_ids)[:5]
    assert (a_dis.view(np.uint32) == b_dis.view(np.uint32)).all()


def flip_noise(rng, centres, n, p=0.1):
    """n rows: a random centre each, every bit flipped with probability p."""
    nbytes = centres.shape[1]
    rows = centres[rng.integers(0, len(centres), n)].copy()
    flips = np.packbits(rng.random((n, nbytes * 8)) < p, axis=1, bitorder="little")
    return rows ^ flips


def assign(rows, cent):
    """list of every row: the smallest (Hamming distance, list id) -- the oracle's tie rule."""
    return o.knn_bin(rows, cent, 1, o.METRIC_HAMMING)[0][:, 0]


def by_label(rows, labels, cent):
    """rows, labels, lists in ascending label order"""
    order = np.argsort(labels, kind="stable")
    return rows[order], labels[order], assign(rows[order], cent)


def ref_search(q, cent, rows_s, labels_s, lists_s, nprobe, k, metric, alive_s=None):
    """The composed reference over label-sorted rows (rows_s, labels_s, their lists lists_s; alive_s: bool per sorted row)."""
    nq, nlist = len(q), len(cent)
    probes = o.knn_bin(q, cent, min(nprobe, nlist), o.METRIC_HAMMING)[0]
    ids = np.full((nq, k), -1, np.int64)
    dis = np.full((nq, k), FLT_MAX, np.float32)
    for i in range(nq):
        m = np.isin(lists_s, probes[i])
        if alive_s is not None:
            m &= alive_s
        sub, lab = rows_s[m], labels_s[m]
        if len(sub) == 0:
            continue
        si, sd = o.knn_bin(q[i:i + 1], sub, k, OM[metric])
        ok = si[0] >= 0
        ids[i, ok] = lab[si[0][ok]]
        dis[i] = sd[0]
    return ids, dis


def check_structure(ix, rows, labels, cent):
    """export: monotone offsets ending at n, the fed labels permuted, ascending inside each list, rows moved intact, every row in
    the list the oracle assigns it to"""
    n, nlist = len(rows), len(cent)
    ec, off, erows, elab = ix.export()
    assert (ec == cent).all()
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all() and len(off) == nlist + 1
    assert sorted(elab.tolist()) == sorted(labels.tolist())
    where = {int(l): i for i, l in enumerate(labels)}
    assert (erows == rows[[where[int(l)] for l in elab]]).all()
    lists = np.repeat(np.arange(nlist), np.diff(off))
    for l in range(nlist):
        assert (np.diff(elab[off[l]:off[l + 1]]) > 0).all()
    assert (lists == assign(erows, cent)).all()
    return off


# ---------------------------------------------------------------------------------------- 1. structure

def test_structure_exact_assignment_and_label_order():
    rng = np.random.default_rng(1)
    n, nbytes, nlist = 6000, 20, 24
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    centres[17] = centres[5]  # identical centroids: ties go to the lower id, list 17 stays empty
    rows = flip_noise(rng, centres, n)
    labels = 3 * np.arange(n, dtype=np.int64) + 1
    perm = rng.permutation(n)  # fed in no label order
    ix = capi.BinIndex(nbytes, capi.METRIC_HAMMING, "ncentroids=%d" % nlist)
    assert ix.num_lists == nlist and capi.BinIndex(nbytes, capi.METRIC_HAMMING).num_lists == 0
    ix.set_centroids(centres)
    ix.add(rows[perm[:2500]], labels[perm[:2500]])
    ix.add(rows[perm[2500:]], labels[perm[2500:]])
    assert ix.num_data == n
    off = check_structure(ix, rows, labels, centres)
    assert off[18] == off[17] and off[6] > off[5]
    ix.close()


# ---------------------------------------------------------------------------------------- 2. search parity

NLIST = 32


@functools.lru_cache(maxsize=None)
def parity_case(metric, nbytes, data):
    """Index, flat index, queries and the references of one (metric, nbytes, data) case, computed once: k = 100 per nprobe (the
    first k of it is the reference of a smaller k)."""
    rng = np.random.default_rng(nbytes * 31 + metric * 7 + len(data))
    n = 8000 + nbytes  # (odd sizes: no multiple of a wavefront step)
    centres = rng.integers(0, 256, (NLIST, nbytes), dtype=np.uint8)
    if data == "clustered":
        rows = flip_noise(rng, centres, n)
    else:  # 40 distinct vectors: every top-k is a tie broken by label
        rows = flip_noise(rng, centres, 40)[rng.integers(0, 40, n)]
    rows[::97] = 0  # all-zero rows: Jaccard against the zero query is 1 by definition
    labels = rng.permutation(2 * n)[:n].astype(np.int64)
    q = flip_noise(rng, centres, 300, 0.15)
    q[0] = 0
    ix = capi.BinIndex(nbytes, metric, "ncentroids=%d" % NLIST)
    ix.set_centroids(centres)
    ix.add(rows, labels)
    flat = capi.BinIndex(nbytes, metric)
    flat.add(rows, labels)
    rows_s, labels_s, lists_s = by_label(rows, labels, centres)
    refs = {p: ref_search(q, centres, rows_s, labels_s, lists_s, p, 100, metric) for p in (1, 4)}
    fi, fd = o.knn_bin(q, rows_s, 100, OM[metric])  # nprobe = nlist: every row
    refs[NLIST] = (labels_s[fi], fd)
    return ix, flat, q, refs


@pytest.mark.parametrize("data", ["clustered", "dup40"])
@pytest.mark.parametrize("nbytes", [5, 16, 64, 136])
@pytest.mark.parametrize("metric", [capi.METRIC_HAMMING, capi.METRIC_JACCARD])
def test_search_matches_composed_reference(metric, nbytes, data):
    ix, flat, q, refs = parity_case(metric, nbytes, data)
    for nq in (1, 3, 97, 300):
        for k in (1, 10, 100):
            for nprobe in (1, 4, NLIST):
                ids, dis = ix.search(q[:nq], k, params="nprobe=%d" % nprobe)
                ri, rd = refs[nprobe]
                same(ids, dis, ri[:nq, :k], rd[:nq, :k])
                if nprobe == NLIST:
                    fi, fd = flat.search(q[:nq], k)
                    same(ids, dis, fi, fd)
    # msvs_bin_index_search = search_params with the default nprobe (1, the float IVFFLAT default), "" too
    ids, dis = ix.search(q[:3], 10)
    same(ids, dis, refs[1][0][:3, :10], refs[1][1][:3, :10])
    ids, dis = ix.search(q[:3], 10, params="")
    same(ids, dis, refs[1][0][:3, :10], refs[1][1][:3, :10])
    # a flat index ignores nprobe
    fi, fd = flat.search(q[:3], 10)
    same(*flat.search(q[:3], 10, params="nprobe=4"), fi, fd)


@pytest.mark.parametrize("metric", [capi.METRIC_HAMMING, capi.METRIC_JACCARD])
def test_row_segments(metric):
    """Lists cut into several row segments (the bin_ivf_rpb knob: 64-row work items instead of the planned >= 2048)."""
    ix, flat, q, refs = parity_case(metric, 64, "clustered")  # 4 lanes per row: 64 rows per wavefront step of the block
    capi.set_option("bin_ivf_rpb", 64)
    try:
        for k, nprobe in ((10, 4), (100, NLIST), (1, 1)):
            ids, dis = ix.search(q[:97], k, params="nprobe=%d" % nprobe)
            same(ids, dis, refs[nprobe][0][:97, :k], refs[nprobe][1][:97, :k])
    finally:
        capi.set_option("bin_ivf_rpb")


# ---------------------------------------------------------------------------------------- 3. short lists

def test_short_lists_padding_and_clipped_nprobe():
    rng = np.random.default_rng(3)
    nbytes, nlist = 24, 8
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    sizes = [1, 0, 3, 70, 5, 1, 200, 2]  # a list with one row, an empty one, lists shorter than a wavefront step
    rows = np.concatenate([flip_noise(rng, centres[l:l + 1], s, 0.02) for l, s in enumerate(sizes)])
    n = len(rows)
    labels = rng.permutation(5 * n)[:n].astype(np.int64)
    ix = capi.BinIndex(nbytes, capi.METRIC_JACCARD, "ncentroids=%d" % nlist)
    ix.set_centroids(centres)
    ix.add(rows, labels)
    off = check_structure(ix, rows, labels, centres)
    assert np.diff(off).tolist() == sizes
    rows_s, labels_s, lists_s = by_label(rows, labels, centres)
    q = np.concatenate([centres, flip_noise(rng, centres, 9, 0.05)])  # query l probes list l first
    for k in (1, 10, 100):
        for nprobe in (1, 2, nlist, nlist + 5):  # beyond nlist: clipped
            ids, dis = ix.search(q, k, params="nprobe=%d" % nprobe)
            ri, rd = ref_search(q, centres, rows_s, labels_s, lists_s, nprobe, k, capi.METRIC_JACCARD)
            same(ids, dis, ri, rd)
    ids, dis = ix.search(q[:2], 10, params="nprobe=1")
    assert ids[0].tolist() == [labels[0]] + [-1] * 9 and (dis[0, 1:] == FLT_MAX).all()  # the one-row list, padded
    assert (ids[1] == -1).all() and (dis[1] == FLT_MAX).all()  # the empty list
    ix.close()


# ---------------------------------------------------------------------------------------- 4. filter

@pytest.mark.parametrize("metric", [capi.METRIC_HAMMING, capi.METRIC_JACCARD])
def test_filter_by_label(metric):
    ix, flat, q, refs = parity_case(metric, 64, "clustered")
    rng = np.random.default_rng(4)
    _, _, erows, elab = ix.export()
    order = np.argsort(elab, kind="stable")
    rows_s, labels_s = erows[order], elab[order]
    lists_s = assign(rows_s, ix.export()[0])
    nbits = int(labels_s.max()) - 1000  # smaller than the largest label: labels at or beyond nbits are dead
    alive = rng.random(nbits) < 0.5
    alive_s = np.zeros(len(labels_s), bool)
    inside = labels_s < nbits
    alive_s[inside] = alive[labels_s[inside]]
    assert 0 < alive_s.sum() < inside.sum() < len(labels_s)
    cent = ix.export()[0]
    for nq, k, nprobe in ((1, 10, 1), (97, 10, 4), (40, 100, NLIST), (300, 1, 4)):
        ids, dis = ix.search(q[:nq], k, alive=alive, params="nprobe=%d" % nprobe)
        ri, rd = ref_search(q[:nq], cent, rows_s, labels_s, lists_s, nprobe, k, metric, alive_s)
        same(ids, dis, ri, rd)
    fi, fd = flat.search(q[:40], 100, alive=alive)
    same(*ix.search(q[:40], 100, alive=alive, params="nprobe=%d" % NLIST), fi, fd)


# ---------------------------------------------------------------------------------------- 5. lifecycle

def test_lifecycle_and_error_codes():
    rng = np.random.default_rng(5)
    nbytes, nlist = 16, 8
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    rows = flip_noise(rng, centres, 900)
    q = flip_noise(rng, centres, 5)
    ix = capi.BinIndex(nbytes, capi.METRIC_HAMMING, "ncentroids=%d" % nlist)
    for call in (lambda: ix.search(q, 3), lambda: ix.search(q, 3, params="nprobe=2"), lambda: ix.add(rows)):
        with pytest.raises(capi.MsvsError) as e:
            call()
        assert e.value.code == capi.ERR_NOT_READY
    with pytest.raises(capi.MsvsError) as e:
        ix.set_centroids(centres[:nlist - 1])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    ix.set_centroids(centres)
    ix.add(rows[:500])  # labels = staging order
    lab = np.arange(900, dtype=np.int64)
    ids, dis = ix.search(q, 10, params="nprobe=3")
    same(ids, dis, *ref_search(q, centres, rows[:500], lab[:500], assign(rows[:500], centres), 3, 10, capi.METRIC_HAMMING))
    ix.add(rows[500:])  # after a search: the image is rebuilt, the new rows are found
    ids, dis = ix.search(q, 10, params="nprobe=3")
    same(ids, dis, *ref_search(q, centres, rows, lab, assign(rows, centres), 3, 10, capi.METRIC_HAMMING))
    hit = ix.search(rows[700:701], 1, params="nprobe=1")
    assert hit[1][0, 0] == 0 and hit[0][0, 0] >= 0 and (rows[hit[0][0, 0]] == rows[700]).all()
    for bad in ("nprobe=0", "nprobe=x", "nprobes=3"):
        with pytest.raises(capi.MsvsError) as e:
            ix.search(q, 3, params=bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.MsvsError) as e:
        ix.search(q, capi.MAX_K + 1, params="nprobe=2")
    assert e.value.code == capi.ERR_UNSUPPORTED_K
    # bad creation parameters: what msvs_index_create returns for them
    for bad in ("ncentroids=0", "ncentroids=abc", "ncentroids=4,niter=z"):
        with pytest.raises(capi.MsvsError) as e:
            capi.BinIndex(nbytes, capi.METRIC_HAMMING, bad)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
        with pytest.raises(capi.MsvsError) as f:
            capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, 8, bad.replace("niter", "kmeans_iters"))
        assert f.value.code == e.value.code
    with pytest.raises(capi.MsvsError) as e:
        capi.BinIndex(nbytes, capi.METRIC_L2, "ncentroids=4")
    assert e.value.code == capi.ERR_NOT_IMPLEMENTED
    with pytest.raises(capi.MsvsError) as e:
        ix.train(rows[:nlist - 1])  # fewer rows than lists
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    ix.close()


# ---------------------------------------------------------------------------------------- 6. training

def test_training_is_deterministic_and_lowers_the_distortion():
    rng = np.random.default_rng(6)
    n, nbytes, nlist = 8192, 32, 64
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    rows = flip_noise(rng, centres, n)

    def trained(niter):
        ix = capi.BinIndex(nbytes, capi.METRIC_HAMMING, "ncentroids=%d,niter=%d" % (nlist, niter))
        ix.train(rows)
        return ix

    def distortion(cent):
        return float(o.knn_bin(rows, cent, 1, o.METRIC_HAMMING)[1].astype(np.float64).sum())

    a, b, seeds = trained(10), trained(10), trained(0)
    ca, cb, cs = a.export()[0], b.export()[0], seeds.export()[0]
    assert (ca == cb).all()
    have = {r.tobytes() for r in rows}
    assert all(c.tobytes() in have for c in cs)  # niter = 0: the seeds, rows of the input
    assert (trained(0).export()[0] == cs).all()
    assert distortion(ca) < distortion(cs)
    # one round by hand from the seeds: exact assignment, then the per-bit majority (2 * ones > members), empty lists kept
    one = trained(1).export()[0]
    lists = assign(rows, cs)
    bits = np.unpackbits(rows, axis=1, bitorder="little")
    want = cs.copy()
    for l in range(nlist):
        m = lists == l
        if m.any():
            want[l] = np.packbits(2 * bits[m].sum(axis=0) > m.sum(), bitorder="little")
    assert (one == want).all()
    labels = 2 * np.arange(n, dtype=np.int64)
    a.add(rows[:3000], labels[:3000])
    a.add(rows[3000:], labels[3000:])
    check_structure(a, rows, labels, ca)
    for ix in (a, b, seeds):
        ix.close()


# ---------------------------------------------------------------------------------------- 7. serialise and load

def test_serialize_round_trip_and_corrupt_files():
    rng = np.random.default_rng(7)
    nbytes, nlist, n = 20, 16, 3000
    centres = rng.integers(0, 256, (nlist, nbytes), dtype=np.uint8)
    rows = flip_noise(rng, centres, n)
    labels = rng.permutation(4 * n)[:n].astype(np.int64)
    q = flip_noise(rng, centres, 20)
    ix = capi.BinIndex(nbytes, capi.METRIC_JACCARD, "ncentroids=%d" % nlist)
    ix.set_centroids(centres)
    ix.add(rows, labels)
    store = {}
    ix.serialize_io(store)
    data = bytes(store["data_bin"])
    assert data[:8] == b"MSVSBIN1" and int.from_bytes(data[8:12], "little") == 2
    assert int.from_bytes(data[32:40], "little") == nlist and len(data) == 48 + n * nbytes + nlist * nbytes
    assert data[48:48 + n * nbytes] == rows.tobytes()  # rows stay in insertion order
    iy = capi.BinIndex.load_io(store, nbytes, capi.METRIC_JACCARD)
    assert iy.num_lists == nlist and iy.num_data == n
    for x, y in zip(ix.export(), iy.export()):
        assert (x == y).all()
    same(*ix.search(q, 10, params="nprobe=3"), *iy.search(q, 10, params="nprobe=3"))
    # a flat index writes what it always wrote: version 1, reserved words zero, rows, nothing after them
    flat = capi.BinIndex(nbytes, capi.METRIC_JACCARD)
    flat.add(rows, labels)
    fs = {}
    flat.serialize_io(fs)
    header = b"MSVSBIN1" + (1).to_bytes(4, "little") + int(capi.METRIC_JACCARD).to_bytes(4, "little") + nbytes.to_bytes(8, "little") \
        + n.to_bytes(8, "little") + bytes(16)
    assert bytes(fs["data_bin"]) == header + rows.tobytes()
    assert bytes(fs["id_list"]) == n.to_bytes(8, "little") + labels.tobytes() == bytes(store["id_list"])
    fl = capi.BinIndex.load_io(fs, nbytes, capi.METRIC_JACCARD)  # version 1 loads as before
    assert fl.num_lists == 0
    same(*fl.search(q, 10), *flat.search(q, 10))
    # corrupt version-2 files
    cut = dict(store)
    cut["data_bin"] = bytearray(data[:48 + n * nbytes + 3 * nbytes + 7])  # truncated inside the centroids
    inflated = dict(store)
    inflated["data_bin"] = bytearray(data[:32] + (nlist * 1000).to_bytes(8, "little") + data[40:])
    both = dict(store)
    both["data_bin"] = bytearray(data[:32] + (nlist * 1000).to_bytes(8, "little") * 2 + data[48:])  # both list words inflated
    for bad in (cut, inflated, both):
        with pytest.raises(capi.MsvsError) as e:
            capi.BinIndex.load_io(bad, nbytes, capi.METRIC_JACCARD)
        assert e.value.code == capi.ERR_IO
    for i in (ix, iy, flat, fl):
        i.close()
