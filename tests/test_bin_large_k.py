"""Binary vectors with more than MSVS_MAX_K = 256 results (k <= MSVS_MAX_K_ROUNDS = 4096) and the device-pointer entries of the
binary index: msvs_knn_bin_rounds, msvs_bin_index_search_rounds, msvs_bin_index_search_device, msvs_bin_index_search_rounds_device.

Hamming distances are small integers: hundreds of rows share one distance, so the boundary between two rank rounds nearly always
falls inside a run of ties and the label half of the key has to carry the continuation.  The data here is built for that (TieData),
and the test asserts on its own reference that every boundary it uses lies strictly inside such a run before it looks at a device.

The reference is a numpy restatement of include/msvs.h: popcounts of x ^ y, x & y and x | y; Jaccard is ONE f32 division of the
exact counts and 1 for an empty union; the first k alive rows by np.lexsort((labels, d)); pads -1 / FLT_MAX.  Ids compare exactly,
distances as bit patterns."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi

pytestmark = pytest.mark.gpu
HAM, JAC = capi.METRIC_HAMMING, capi.METRIC_JACCARD
FLT_MAX = np.finfo(np.float32).max
POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)
NBYTES = (5, 16, 64, 136)  # lanes per row 1, 1, 4, 8; the last one is the only one whose row does not fit the group's registers
NLABEL = 4000
BOUNDARIES = (256, 512, 768, 1024, 1280)


# ---------------------------------------------------------------------------------------- the reference

def popc(a):
    return POP8[a].sum(axis=-1)


def distances(q, rows, metric):
    """q [nbytes], rows [n, nbytes] -> f32 [n]"""
    if metric == HAM:
        return popc(q ^ rows).astype(np.float32)
    inter, union = popc(q & rows), popc(q | rows)
    d = np.ones(len(rows), np.float32)
    nz = union > 0
    d[nz] = (union[nz] - inter[nz]).astype(np.float32) / union[nz].astype(np.float32)  # one f32 division of exact counts
    return d


def ref_topk(q, rows, labels, k, metric, alive=None):
    """The first k alive rows by (distance, label); alive: bool over LABELS (labels at or beyond its length are dead)."""
    q = np.asarray(q, np.uint8).reshape(-1, rows.shape[1])
    ids = np.full((len(q), k), -1, np.int64)
    dis = np.full((len(q), k), FLT_MAX, np.float32)
    keep = np.ones(len(rows), bool)
    if alive is not None:
        keep = labels < len(alive)
        keep[keep] = alive[labels[keep]]
    sub, lab = rows[keep], labels[keep]
    for i in range(len(q)):
        d = distances(q[i], sub, metric)
        order = np.lexsort((lab, d))[:k]
        ids[i, :len(order)] = lab[order]
        dis[i, :len(order)] = d[order]
    return ids, dis


def same(a_ids, a_dis, b_ids, b_dis):
    assert a_ids.shape == b_ids.shape and a_dis.shape == b_dis.shape
    assert (a_ids == b_ids).all(), np.argwhere(a_ids != b_ids)[:5]
    assert (a_dis.view(np.uint32) == b_dis.view(np.uint32)).all(), np.argwhere(a_dis.view(np.uint32) != b_dis.view(np.uint32))[:5]


# ---------------------------------------------------------------------------------------- tie data

def flip(v, positions):
    v = v.copy()
    for p in positions:
        v[p >> 3] ^= np.uint8(1 << (p & 7))
    return v


class TieData:
    """A random base vector; 200 rows with 1 flipped bit, 500 with 2, 800 with 3; then a few all-zero rows.  Labels are a
    permutation's head, so label order differs from storage order.  Queries: the base, the base with three bits flipped, all zero."""

    def __init__(self, nbytes):
        rng = np.random.default_rng(7)
        nbit = nbytes * 8
        self.nbytes = nbytes
        self.base = rng.integers(0, 256, nbytes, dtype=np.uint8)
        rows = [flip(self.base, rng.choice(nbit, f, replace=False)) for f, cnt in ((1, 200), (2, 500), (3, 800)) for _ in range(cnt)]
        perm = rng.permutation(NLABEL)
        self.n_tie = len(rows)
        rows += [np.zeros(nbytes, np.uint8)] * 4
        self.rows = np.stack(rows)
        self.labels = perm[:len(rows)].astype(np.int64)
        self.q = np.stack([self.base, flip(self.base, (0, 9, nbit - 1)), np.zeros(nbytes, np.uint8)])


@functools.lru_cache(maxsize=None)
def tie_data(nbytes):
    return TieData(nbytes)


def assert_boundaries_inside_ties(dis_row, ranks):
    """every rank r of `ranks`: result r - 1 and result r exist and share one distance"""
    for r in ranks:
        assert dis_row[r] != FLT_MAX and dis_row[r - 1].view(np.uint32) == dis_row[r].view(np.uint32), r


@functools.lru_cache(maxsize=None)
def flat_case(nbytes, metric):
    """(data, flat index with the labels, reference over labels for k = 4096, reference over row positions for k = 4096): the first
    k columns are the reference of a smaller k.  Asserts the property the data is made for."""
    t = tie_data(nbytes)
    ref = ref_topk(t.q, t.rows, t.labels, 4096, metric)
    pos = ref_topk(t.q, t.rows, np.arange(len(t.rows), dtype=np.int64), 4096, metric)
    for r in (ref, pos):
        assert_boundaries_inside_ties(r[1][0], BOUNDARIES)  # the base query: every round boundary inside a run of ties
    if metric == JAC:  # the all-zero query: every row ties at 1, the label alone orders them
        assert (ref[1][2][:len(t.rows)] == np.float32(1)).all() and (np.diff(ref[0][2][:len(t.rows)]) > 0).all()
    ix = capi.BinIndex(nbytes, metric)
    ix.add(t.rows[:700], t.labels[:700])
    ix.add(t.rows[700:], t.labels[700:])
    return t, ix, ref, pos


def head(ref, k):
    return ref[0][:, :k], ref[1][:, :k]


CASES = [(nb, m) for nb in NBYTES for m in (HAM, JAC)]


# ---------------------------------------------------------------------------------------- 1. flat index and knn_bin_rounds

@pytest.mark.parametrize("nbytes,metric", CASES)
def test_flat_rounds_match_the_sort(nbytes, metric):
    t, ix, ref, pos = flat_case(nbytes, metric)
    for k in (257, 512, 513, 1000, 4096):  # 4096 > n: the tail is padded
        same(*ix.search_rounds(t.q, k), *head(ref, k))
        same(*capi.knn_bin_rounds(t.q, t.rows, k, metric), *head(pos, k))
    n = len(t.rows)
    ids, dis = ix.search_rounds(t.q, 4096)
    assert (ids[:, n:] == -1).all() and (dis[:, n:] == FLT_MAX).all() and (ids[:, :n] >= 0).all()


@pytest.mark.parametrize("nbytes,metric", CASES)
def test_flat_rounds_with_filters(nbytes, metric):
    """512 alive rows: k = 512 ends on a full last round, k = 513 adds a round that finds nothing; 300 alive rows with k = 600:
    the second round comes back short and the third scan admits nothing."""
    t, ix, _, _ = flat_case(nbytes, metric)
    rng = np.random.default_rng(nbytes + metric)
    n = len(t.rows)
    for n_alive, ks in ((512, (512, 513)), (300, (600,))):
        rows_alive = np.zeros(n, bool)
        rows_alive[rng.choice(n, n_alive, replace=False)] = True
        by_label = np.zeros(NLABEL, bool)
        by_label[t.labels[rows_alive]] = True
        assert by_label.sum() == n_alive
        for k in ks:
            ri, rd = ref_topk(t.q, t.rows, t.labels, k, metric, alive=by_label)
            assert (ri[:, :n_alive] >= 0).all() and (ri[:, n_alive:] == -1).all()
            same(*ix.search_rounds(t.q, k, alive=by_label), ri, rd)
            pi, pd = ref_topk(t.q, t.rows, np.arange(n, dtype=np.int64), k, metric, alive=rows_alive)
            same(*capi.knn_bin_rounds(t.q, t.rows, k, metric, alive=rows_alive), pi, pd)


@pytest.mark.parametrize("nbytes,metric", CASES)
def test_rounds_entries_up_to_256_give_the_existing_bits(nbytes, metric):
    t, ix, ref, pos = flat_case(nbytes, metric)
    alive = np.random.default_rng(3).random(NLABEL) < 0.5
    for k in (1, 100, 256):
        a = ix.search(t.q, k)
        same(*ix.search_rounds(t.q, k), *a)
        same(*a, *head(ref, k))
        same(*ix.search_rounds(t.q, k, alive=alive), *ix.search(t.q, k, alive=alive))
        b = capi.knn_bin(t.q, t.rows, k, metric)
        same(*capi.knn_bin_rounds(t.q, t.rows, k, metric), *b)
        same(*b, *head(pos, k))


def test_flat_batch_beyond_one_launch_of_queries():
    """The flat scan keeps its queries on grid.y: 65535 + 2 queries run as two chunks.  2-byte vectors, every query value once."""
    rng = np.random.default_rng(2)
    n, k = 300, 10
    r16 = rng.integers(0, 1 << 16, n).astype(np.uint16)
    q16 = np.concatenate([np.arange(1 << 16), [0x1234]]).astype(np.uint16)
    labels = rng.permutation(NLABEL)[:n].astype(np.int64)
    pop16 = POP8[np.arange(1 << 16) & 255] + POP8[np.arange(1 << 16) >> 8]
    d = pop16[q16[:, None] ^ r16[None, :]]
    order = np.argsort(d * NLABEL + labels[None, :], axis=1)[:, :k]
    ix = capi.BinIndex(2, HAM)
    ix.add(r16.view(np.uint8).reshape(n, 2), labels)
    ids, dis = ix.search_rounds(q16.view(np.uint8).reshape(-1, 2), k)
    same(ids, dis, labels[order], np.take_along_axis(d, order, axis=1).astype(np.float32))
    ix.close()


# ---------------------------------------------------------------------------------------- 2. partitioned index

NLIST = 6


class IvfData:
    """6 centroids: the base, its complement, three with a fixed block of bytes inverted, one with every other byte inverted (far from
    every row: its list is empty).  Rows: the 1500 tie rows, 700 near the complement, 40 near the third centroid."""

    def __init__(self, nbytes):
        t = tie_data(nbytes)
        rng = np.random.default_rng(11)
        nbit = nbytes * 8
        base = t.base
        third = max(1, nbytes // 3)
        cent = [base, ~base]
        for b in range(3):
            c = base.copy()
            c[b * third:(b + 1) * third] ^= np.uint8(255)
            cent.append(c)
        far = base.copy()
        far[::2] ^= np.uint8(255)
        cent.append(far)
        self.cent = np.stack(cent).astype(np.uint8)
        near_c = [flip(self.cent[1], rng.choice(nbit, int(rng.integers(0, 4)), replace=False)) for _ in range(700)]
        near_3 = [flip(self.cent[2], rng.choice(nbit, int(rng.integers(0, 3)), replace=False)) for _ in range(40)]
        self.rows = np.concatenate([t.rows[:t.n_tie], np.stack(near_c), np.stack(near_3)])
        self.labels = rng.permutation(NLABEL)[:len(self.rows)].astype(np.int64)
        self.q = np.stack([base, flip(self.cent[2], (1, 10)), flip(self.cent[1], (5,)), np.zeros(nbytes, np.uint8)])
        # a row belongs to the list with the smallest (Hamming distance, list id); a query probes lists by the same key
        d = np.stack([popc(self.rows ^ c) for c in self.cent], axis=1)
        self.list_of = np.argmin(d * NLIST + np.arange(NLIST)[None, :], axis=1)
        dq = np.stack([popc(self.q ^ c) for c in self.cent], axis=1)
        self.probe_order = np.argsort(dq * NLIST + np.arange(NLIST)[None, :], axis=1)

    def ref(self, nprobe, k, metric, alive=None):
        ids = np.full((len(self.q), k), -1, np.int64)
        dis = np.full((len(self.q), k), FLT_MAX, np.float32)
        for i in range(len(self.q)):
            m = np.isin(self.list_of, self.probe_order[i, :nprobe])
            if m.any():
                ids[i], dis[i] = (r[0] for r in ref_topk(self.q[i], self.rows[m], self.labels[m], k, metric, alive))
        return ids, dis


@functools.lru_cache(maxsize=None)
def ivf_case(nbytes, metric):
    d = IvfData(nbytes)
    lens = np.bincount(d.list_of, minlength=NLIST)
    assert lens.tolist() == [1500, 700, 40, 0, 0, 0], lens
    assert d.probe_order[0, 0] == 0 and d.probe_order[1, 0] == 2 and d.probe_order[2, 0] == 1
    ix = capi.BinIndex(nbytes, metric, "ncentroids=%d" % NLIST)
    ix.set_centroids(d.cent)
    ix.add(d.rows[:1000], d.labels[:1000])
    ix.add(d.rows[1000:], d.labels[1000:])
    flat = capi.BinIndex(nbytes, metric)
    flat.add(d.rows, d.labels)
    return d, ix, flat


IVF_CASES = [(64, HAM), (64, JAC), (136, HAM), (136, JAC)]  # the row in the group's registers, and not


@pytest.mark.parametrize("nbytes,metric", IVF_CASES)
def test_ivf_rounds_match_the_composed_reference(nbytes, metric):
    d, ix, flat = ivf_case(nbytes, metric)
    # nprobe = 1, k = 1000: the base query's full rounds lie inside one list, each boundary inside a run of ties
    ri, rd = d.ref(1, 1000, metric)
    assert_boundaries_inside_ties(rd[0], (256, 512, 768))
    same(*ix.search_rounds(d.q, 1000, params="nprobe=1"), ri, rd)
    same(*ix.search_rounds(d.q, 1000), ri, rd)  # (params None: the default nprobe = 1)
    same(*ix.search_rounds(d.q, 1000, params=""), ri, rd)
    # nprobe = 1, k = 300: the query near the 40-row list gets a short first round, its tail stays padded through the second
    ri, rd = d.ref(1, 300, metric)
    assert (ri[1, :40] >= 0).all() and (ri[1, 40:] == -1).all()
    same(*ix.search_rounds(d.q, 300, params="nprobe=1"), ri, rd)
    for k in (257, 1000, 4096):
        same(*ix.search_rounds(d.q, k, params="nprobe=2"), *d.ref(2, k, metric))
    # every list probed: the flat index's result
    for k in (600, 4096):
        got = ix.search_rounds(d.q, k, params="nprobe=6")
        same(*got, *d.ref(NLIST, k, metric))
        same(*got, *flat.search_rounds(d.q, k))
        same(*got, *ref_topk(d.q, d.rows, d.labels, k, metric))
    for k in (1, 100, 256):  # up to 256: the existing entry's bits
        same(*ix.search_rounds(d.q, k, params="nprobe=2"), *ix.search(d.q, k, params="nprobe=2"))


@pytest.mark.parametrize("nbytes,metric", [(64, HAM), (136, JAC)])
def test_ivf_rounds_over_several_row_segments(nbytes, metric):
    """Lists cut into 64-row work items (the bin_ivf_rpb knob): every (pair, segment) slot is rewritten or cleared round by round."""
    d, ix, _ = ivf_case(nbytes, metric)
    capi.set_option("bin_ivf_rpb", 64)
    try:
        for nprobe, k in ((1, 1000), (2, 300), (6, 4096)):
            same(*ix.search_rounds(d.q, k, params="nprobe=%d" % nprobe), *d.ref(nprobe, k, metric))
    finally:
        capi.set_option("bin_ivf_rpb")


@pytest.mark.parametrize("nbytes,metric", IVF_CASES)
def test_ivf_rounds_with_a_label_filter(nbytes, metric):
    d, ix, _ = ivf_case(nbytes, metric)
    alive = np.random.default_rng(5).random(NLABEL - 500) < 0.6  # (labels at or beyond nbits are dead)
    for nprobe, k in ((1, 700), (2, 1000), (6, 2000)):
        same(*ix.search_rounds(d.q, k, params="nprobe=%d" % nprobe, alive=alive), *d.ref(nprobe, k, metric, alive))


# ---------------------------------------------------------------------------------------- 3. device entries

def device_search(ix, entry, q, k, nprobe, alive, stream):
    """q (host uint8 [nx, nbytes]) through a device entry on `stream`, outputs prefilled with garbage -> host (ids, dis)"""
    import torch
    nx = len(q)
    with torch.cuda.stream(stream):
        d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        d_ids = torch.full((nx, k), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
        d_dis = torch.full((nx, k), -123.0, dtype=torch.float32, device="cuda")
        d_alive, nbits = None, 0
        if alive is not None:
            d_alive = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).cuda()
            nbits = len(alive)
        getattr(ix, entry)(d_q.data_ptr(), nx, k, nprobe, d_ids.data_ptr(), d_dis.data_ptr(), stream=stream.cuda_stream,
                           d_alive=d_alive.data_ptr() if d_alive is not None else 0, nbits=nbits)
        stream.synchronize()
        return d_ids.cpu().numpy(), d_dis.cpu().numpy()


@pytest.mark.parametrize("nx", [1, 3, 70])
@pytest.mark.parametrize("part", [False, True])
def test_device_entries_equal_the_host_entries(nx, part):
    import torch
    d, ivf, flat = ivf_case(64, HAM)
    ix, nprobe = (ivf, 2) if part else (flat, 0)  # (a flat index ignores nprobe)
    rng = np.random.default_rng(nx)
    q = np.concatenate([d.q, d.rows[rng.integers(0, len(d.rows), 66)] ^ rng.integers(0, 2, (66, 64), dtype=np.uint8)])[:nx]
    alive = np.random.default_rng(9).random(NLABEL) < 0.7
    stream = torch.cuda.Stream()
    for al in (None, alive):
        for entry, k in (("search_device", 10), ("search_device", 256), ("search_rounds_device", 1000)):
            host = ix.search_rounds(q, k, params="nprobe=2" if part else None, alive=al)
            if k <= 256:
                same(*host, *ix.search(q, k, params="nprobe=2" if part else None, alive=al))
            if not part:
                same(*host, *ref_topk(q, d.rows, d.labels, k, HAM, al))
            same(*device_search(ix, entry, q, k, nprobe, al, stream), *host)


# ---------------------------------------------------------------------------------------- 4. errors

def code_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except capi.MsvsError as e:
        return e.code
    return capi.OK


def test_errors_and_no_ops():
    import torch
    d, ivf, flat = ivf_case(64, HAM)
    q = d.q
    d_q = torch.from_numpy(q).cuda()
    d_ids = torch.full((len(q), 8), 77, dtype=torch.int64, device="cuda")
    d_dis = torch.full((len(q), 8), 5.0, dtype=torch.float32, device="cuda")
    dev = (d_q.data_ptr(), len(q))
    out = (d_ids.data_ptr(), d_dis.data_ptr())
    for ix in (flat, ivf):
        # k beyond a limit
        assert code_of(ix.search_rounds, q, 4097) == capi.ERR_UNSUPPORTED_K
        assert code_of(ix.search_rounds_device, *dev, 4097, 1, *out) == capi.ERR_UNSUPPORTED_K
        assert code_of(ix.search_device, *dev, 257, 1, *out) == capi.ERR_UNSUPPORTED_K
        assert code_of(ix.search, q, 257) == capi.ERR_UNSUPPORTED_K
        assert code_of(ix.search, q, 257, params="nprobe=2") == capi.ERR_UNSUPPORTED_K
        # a null d_x with nx > 0
        assert code_of(ix.search_device, 0, len(q), 8, 1, *out) == capi.ERR_INVALID_ARGUMENT
        assert code_of(ix.search_rounds_device, 0, len(q), 300, 1, *out) == capi.ERR_INVALID_ARGUMENT
        # k = 0 or nx = 0: a no-op that leaves the outputs untouched
        for entry in (ix.search_device, ix.search_rounds_device):
            assert code_of(entry, *dev, 0, 1, *out) == capi.OK
            assert code_of(entry, d_q.data_ptr(), 0, 8, 1, *out) == capi.OK
            assert code_of(entry, 0, 0, 8, 1, 0, 0) == capi.OK
        ids, dis = ix.search_rounds(q[:0], 300)
        assert ids.shape == (0, 300) and dis.shape == (0, 300)
        ids, dis = ix.search_rounds(q, 0)
        assert ids.shape == (len(q), 0)
    assert code_of(capi.knn_bin_rounds, q, d.rows, 4097, HAM) == capi.ERR_UNSUPPORTED_K
    assert code_of(capi.knn_bin, q, d.rows, 257, HAM) == capi.ERR_UNSUPPORTED_K
    assert capi.knn_bin_rounds(q, d.rows, 0, HAM)[0].shape == (len(q), 0)
    # nprobe = 0: refused by a partitioned index, ignored by a flat one
    assert code_of(ivf.search_device, *dev, 8, 0, *out) == capi.ERR_INVALID_ARGUMENT
    assert code_of(ivf.search_rounds_device, *dev, 300, 0, *out) == capi.ERR_INVALID_ARGUMENT
    assert code_of(ivf.search_rounds, q, 300, params="nprobe=0") == capi.ERR_INVALID_ARGUMENT
    capi.synchronize()
    torch.cuda.synchronize()
    assert (d_ids.cpu().numpy() == 77).all() and (d_dis.cpu().numpy() == 5.0).all()  # nothing above wrote a result
    assert code_of(flat.search_device, *dev, 8, 0, *out) == capi.OK
    torch.cuda.synchronize()
    same(d_ids.cpu().numpy(), d_dis.cpu().numpy(), *flat.search(q, 8))
    # a partitioned index without centroids
    cold = capi.BinIndex(64, HAM, "ncentroids=4")
    assert code_of(cold.search_rounds, q, 300) == capi.ERR_NOT_READY
    assert code_of(cold.search_device, *dev, 8, 1, *out) == capi.ERR_NOT_READY
    assert code_of(cold.search_rounds_device, *dev, 300, 1, *out) == capi.ERR_NOT_READY
    cold.close()
