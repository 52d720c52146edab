"""The graph index (msvs_graph_index_*, capi.GraphIndex): the seeded beam search over a fixed-degree neighbour graph and its build.

ref_search restates steps 1-6 of include/msvs.h's definition in numpy, with oracle.knn for every score; ref_build restates steps
2-5 of the build.  Every comparison is == on ids (or graph words) and on the uint32 view of the distances."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o
from test_pq_ivf import blobs, code_of, same

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP, COS = capi.METRIC_L2, capi.METRIC_IP, capi.METRIC_COSINE
FLT_MAX = np.finfo(np.float32).max
NONE = capi.GRAPH_NO_EDGE
N, NLIST = 2000, 16


def stored(x, metric):
    return o.normalize_rows(x) if metric == COS else np.ascontiguousarray(x, F)


def ref_search(xs, cent, seeds, nbr, q, k, metric, ef=None, nprobe=8, width=1, max_iters=None, alive=None, ends=None):
    """xs: the rows as stored (unit rows for cosine); ends (a list): why every query's search ended"""
    ip = metric != L2
    om = o.METRIC_IP if ip else o.METRIC_L2
    n, R = nbr.shape
    ef = ef or min(max(k, 64), capi.MAX_K)
    max_iters = max_iters or -(-2 * ef // width) + 8
    qs = o.normalize_rows(q) if metric == COS else np.ascontiguousarray(q, F)
    ids = np.full((len(qs), k), -1, np.int64)
    dis = np.full((len(qs), k), -FLT_MAX if ip else FLT_MAX, F)
    for qi, v in enumerate(qs):
        seen, beam = set(), []  # beam entries: [(order value, label), expanded, distance]

        def score(labels):
            new = [l for l in dict.fromkeys(labels) if l not in seen]
            seen.update(new)
            if new:
                lab = np.array(new, np.int64)
                gi, gd = o.knn(v, xs[lab], len(lab), om, labels=lab)
                beam.extend([(-float(d) if ip else float(d), int(i)), False, d] for i, d in zip(gi[0], gd[0]) if i >= 0)
                beam.sort(key=lambda e: e[0])
                del beam[ef:]

        lists = o.knn(v, cent, min(nprobe, len(cent)), om)[0][0]
        score([int(seeds[l]) for l in lists if l >= 0 and seeds[l] >= 0])
        it, why = 0, "iters"
        while it < max_iters:
            if len(seen) + width * R > capi.GRAPH_VISITED_MAX:
                why = "visited"
                break
            parents = [e for e in beam if not e[1]][:width]
            if not parents:
                why = "closed"
                break
            for e in parents:
                e[1] = True
            score([int(t) for e in parents for t in nbr[e[0][1]] if t != NONE and t < n])
            it += 1
        if ends is not None:
            ends.append(why)
        out = [e for e in beam if alive is None or alive[e[0][1]]][:k]
        ids[qi, :len(out)] = [e[0][1] for e in out]
        dis[qi, :len(out)] = [e[2] for e in out]
    if metric == COS:
        dis = (F(1) - dis).astype(F)
    return ids, dis


def ref_build(xs, cent, metric, R):
    """steps 2-5 given the centroids -> (seeds, nbr)"""
    om = o.METRIC_L2 if metric == L2 else o.METRIC_IP
    as_query = (lambda a: o.normalize_rows(a)) if metric == COS else (lambda a: a)
    n, K0, H = len(xs), 2 * R, R // 2
    seeds = o.knn(as_query(cent), xs, 1, om)[0][:, 0].astype(np.int32)
    top = o.knn(as_query(xs), xs, K0 + 1, om)[0]
    L = np.full((n, K0), -1, np.int64)
    for i in range(n):
        row = [t for t in top[i] if t != i][:K0] if i in top[i] else top[i, :K0]
        L[i, :len(row)] = row
    Fl = []
    for i in range(n):
        det = [sum(1 for a in range(b) if L[i, a] >= 0 and L[i, b] in L[L[i, a], :b]) for b in range(K0)]
        Fl.append([int(L[i, b]) for b in sorted(range(K0), key=lambda b: (det[b], b)) if L[i, b] >= 0][:R])
    incoming = [[] for _ in range(n)]
    for i in range(n):
        for r, j in enumerate(Fl[i]):
            incoming[j].append((r, i))
    nbr = np.full((n, R), NONE, np.uint32)
    for j in range(n):
        G = [i for _, i in sorted(incoming[j])[:H]]
        row = list(dict.fromkeys(Fl[j][:H] + G + Fl[j][H:]))[:R]
        nbr[j, :len(row)] = row
    return seeds, nbr


def store_of(x, metric, placement=capi.ROWS_DEVICE):
    rows = capi.Rows(x.shape[1], len(x), normalize=metric == COS, placement=placement)
    rows.append(x)
    return rows


def device_search(ix, q, k, alive=None, **kw):
    import torch
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.ascontiguousarray(q, F)).to(dev)
    di = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    dd = torch.empty((len(q), k), device=dev, dtype=torch.float32)
    bits, nbits = 0, 0
    if alive is not None:
        db = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).to(dev)
        bits, nbits = db.data_ptr(), len(alive)
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), len(q), k, di.data_ptr(), dd.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, d_alive=bits,
                     nbits=nbits, **kw)
    torch.cuda.synchronize()
    return di.cpu().numpy(), dd.cpu().numpy()


# ---------------------------------------------------------------------------------------- 1. search parity with handed graphs

DIMS = [3, 67, 768, 772]  # pad, tail group, one batch of twelve pieces, batch plus tail
DEGREES = [16, 32, 64]
EFK = [(1, 1), (10, 10), (64, 10), (256, 256)]
NPROBES = [1, 8, 40]      # 40 > nlist
PARITY = [((L2, IP, COS)[c % 3], DIMS[c % 4], DEGREES[(c // 2) % 3], EFK[(c // 3) % 4], (1, 4)[(c // 4) % 2], NPROBES[(c // 5) % 3],
           (None, 3)[(c // 7) % 2], (1, 33)[c % 2], bool((c // 6) % 2), ("host", "device")[(c // 8) % 2], ("knn", "rnd")[(c // 9) % 2])
          for c in range(24)]


def test_parity_table_reaches_every_axis():
    want = [{L2, IP, COS}, set(DIMS), set(DEGREES), set(EFK), {1, 4}, set(NPROBES), {None, 3}, {1, 33}, {False, True}, {"host", "device"},
            {"knn", "rnd"}]
    assert [{r[i] for r in PARITY} for i in range(11)] == want


@functools.lru_cache(maxsize=None)
def data(dim):
    rng = np.random.default_rng(2000 + dim)
    _, x = blobs(rng, N, dim, NLIST, sigma=0.6)
    q = (x[rng.integers(0, N, 33)] + F(0.3) * rng.standard_normal((33, dim), dtype=F)).astype(F)
    cent = x[rng.permutation(N)[:NLIST]].copy()
    head = np.ascontiguousarray(x[:, :8])
    order = o.knn(head, head, 65, o.METRIC_L2)[0]  # neighbours by the first columns: any graph will do
    return x, q, cent, order, rng.random(N) < 0.5


@functools.lru_cache(maxsize=None)
def graph(dim, R, kind):
    x, _, cent, order, _ = data(dim)
    rng = np.random.default_rng(dim * 100 + R)
    seeds = rng.integers(0, N, NLIST).astype(np.int32)
    if kind == "knn":
        return seeds, order[:, 1:R + 1].astype(np.uint32)
    nbr = rng.integers(0, N, (N, R)).astype(np.uint32)
    nbr[:, 0] = np.arange(N)                      # self loops
    nbr[:, 5] = nbr[:, 3]                         # a label twice in a row
    nbr[rng.random((N, R)) < 0.2] = NONE          # holes anywhere
    nbr[::7, 2] = NONE
    seeds[[2, 9]] = -1
    return seeds, nbr


@functools.lru_cache(maxsize=None)
def handed(metric, dim, R, kind):
    x, _, cent, _, _ = data(dim)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d" % R)
    seeds, nbr = graph(dim, R, kind)
    ix.set_graph(cent, seeds, nbr)
    assert ix.ready and ix.num_data == N and ix.num_lists == NLIST and ix.degree == R
    assert ix.memory_usage == N * R * 4 + NLIST * ((dim + 3) // 4) * 16 + NLIST * 4
    return ix


@pytest.mark.parametrize("metric,dim,R,efk,width,nprobe,max_iters,nq,filtered,entry,kind", PARITY)
def test_search_parity(metric, dim, R, efk, width, nprobe, max_iters, nq, filtered, entry, kind):
    (ef, k), (x, q, cent, _, half) = efk, data(dim)
    ix, (seeds, nbr), alive = handed(metric, dim, R, kind), graph(dim, R, kind), half if filtered else None
    ends = []
    exp = ref_search(stored(x, metric), cent, seeds, nbr, q[:nq], k, metric, ef, nprobe, width, max_iters, alive, ends)
    if max_iters and ef > 1:
        assert "iters" in ends  # the cap binds
    if entry == "host":
        params = "ef=%d,nprobe=%d,width=%d" % (ef, nprobe, width) + (",max_iters=%d" % max_iters if max_iters else "")
        got = ix.search(q[:nq], k, params, alive=alive)
    else:
        got = device_search(ix, q[:nq], k, alive, ef=ef, nprobe=nprobe, width=width, max_iters=max_iters or 0)
    same(got, exp)
    if filtered:
        assert half[got[0][got[0] >= 0]].all()


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_nan_row_and_equal_row(metric):
    x, q, cent, order, _ = (a.copy() for a in data(67))
    x[order[40, 1], 5] = np.nan  # a neighbour of row 40: scored, never returned
    q[0] = x[40]
    seeds, nbr = graph(67, 16, "knn")
    seeds = seeds.copy()
    seeds[:] = 40
    rows = store_of(x, metric, capi.ROWS_HOST_PINNED)
    ix = capi.GraphIndex(metric, rows, "degree=16")
    ix.set_graph(cent, seeds, nbr)
    with np.errstate(all="ignore"):
        exp = ref_search(stored(x, metric), cent, seeds, nbr, q[:2], 64, metric, 64)
    got = ix.search(q[:2], 64, "ef=64")
    same(got, exp)
    assert order[40, 1] not in got[0] and (metric == IP or got[0][0, 0] == 40)
    ix.close()
    rows.close()


def test_visited_limit_ends_the_search():
    # rows on a line that approach the query as the label grows, every row pointing at the 64 after it: the beam never closes.
    # (12500 rows of 12 bytes: the limit can only bind on a store of more than MSVS_GRAPH_VISITED_MAX - width * R rows)
    n, R = 12500, 64
    x = np.zeros((n, 3), F)
    x[:, 0] = (n - np.arange(n)) * F(0.001)
    x[:3] = 0  # (the queries themselves)
    nbr = ((np.arange(n)[:, None] + 1 + np.arange(R)[None]) % n).astype(np.uint32)
    cent, seeds = x[3:7].copy(), np.arange(3, 7, dtype=np.int32)
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=64")
    ix.set_graph(cent, seeds, nbr)
    ends = []
    exp = ref_search(x, cent, seeds, nbr, x[:3], 10, L2, 256, 4, 4, 5000, None, ends)
    assert ends == ["visited"] * 3
    same(ix.search(x[:3], 10, "ef=256,nprobe=4,width=4,max_iters=5000"), exp)
    ix.close()
    rows.close()


# ---------------------------------------------------------------------------------------- 2. build parity

@pytest.mark.parametrize("metric,dim,n", [(L2, 8, 600), (COS, 8, 600), (L2, 67, 600), (COS, 67, 600), (L2, 8, 20)])
def test_build_parity(metric, dim, n):
    rng = np.random.default_rng(300 + dim + n)
    _, x = blobs(rng, n, dim, 6, sigma=0.5)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=16,ncentroids=%d,kmeans_iters=3" % (8 if n > 20 else 2))
    assert not ix.ready and code_of(lambda: ix.search(x[:1], 1)) == capi.ERR_NOT_READY
    ix.build()
    cent, seeds, nbr = ix.export()
    exp_seeds, exp_nbr = ref_build(stored(x, metric), cent, metric, 16)
    assert (seeds == exp_seeds).all()
    assert (nbr == exp_nbr).all(), np.argwhere(nbr != exp_nbr)[:5]
    ix.close()
    rows.close()


# ---------------------------------------------------------------------------------------- 3. a built index, end to end

def test_built_index_recall():
    """4000 x 64 blobs (test_pq_ivf.blobs), R = 32, 64 queries.  recall@10 of the reference over the exported structure, measured on
    the CPU for ef = 32, 64, 128: 1.000, 1.000, 1.000.  The threshold is the smallest ef reaching 0.95 (32), its value minus 0.02
    (one query's worth of results at 64 x 10): 0.98.  The GPU equals the reference bit for bit, so the CPU value is the GPU value."""
    rng = np.random.default_rng(11)
    centres, x = blobs(rng, 4000, 64, 8)
    q = (centres[rng.integers(0, 8, 64)] + F(0.3) * rng.standard_normal((64, 64), dtype=F)).astype(F)
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=32,ncentroids=16,kmeans_iters=4")
    ix.build()
    cent, seeds, nbr = ix.export()
    truth = o.knn(q, x, 10, o.METRIC_L2)[0]
    recall = lambda ids: np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, ids)])
    ref = {ef: ref_search(x, cent, seeds, nbr, q, 10, L2, ef) for ef in (32, 64, 128)}
    measured = {ef: float(recall(r[0])) for ef, r in ref.items()}
    print("reference recall@10 by ef:", measured)
    for ef, r in ref.items():
        same(ix.search(q, 10, "ef=%d" % ef), r)
    ef_min, floor = RECALL
    assert measured[ef_min] >= 0.95 and measured[ef_min] >= floor - 0.02
    ix.close()
    rows.close()


RECALL = (32, 1.0)  # (the smallest ef whose reference recall reaches 0.95, that recall as measured)


# ---------------------------------------------------------------------------------------- 4. round trip and refusals

def test_round_trip_and_refusals():
    x, q, cent, _, _ = data(67)
    ix, (seeds, nbr) = handed(L2, 67, 16, "rnd"), graph(67, 16, "rnd")
    files = {}
    ix.serialize_io(files)
    back = capi.GraphIndex.load_io(files, ix.rows)
    assert back.metric == L2 and back.degree == 16 and all((a == b).all() for a, b in zip(back.export(), ix.export()))
    same(back.search(q, 10, "ef=40,width=2"), ix.search(q, 10, "ef=40,width=2"))
    back.close()
    for at in (20, 70, len(files["graph_data"]) - 3):  # the header, a centroid, an edge
        bad = {"graph_data": bytearray(files["graph_data"])}
        bad["graph_data"][at] ^= 0x10
        assert code_of(lambda: capi.GraphIndex.load_io(bad, ix.rows)) == capi.ERR_IO
    other = store_of(x[:100], L2)
    assert code_of(lambda: capi.GraphIndex.load_io(files, other)) == capi.ERR_IO
    inv, unit, empty = capi.ERR_INVALID_ARGUMENT, store_of(x[:100], COS), capi.Rows(67, 4)
    assert code_of(lambda: capi.GraphIndex(L2, unit)) == inv and code_of(lambda: capi.GraphIndex(COS, other)) == inv
    assert code_of(lambda: capi.GraphIndex(capi.METRIC_HAMMING, other)) == capi.ERR_NOT_IMPLEMENTED
    assert code_of(lambda: capi.GraphIndex(L2, other, "degree=24")) == inv
    assert code_of(lambda: capi.GraphIndex(L2, empty).build()) == inv
    small = capi.GraphIndex(L2, other, "degree=16")
    c, s, e = cent.copy(), seeds.copy(), nbr[:100] % 100
    for bc, bs, be in ((np.where(np.arange(67) == 3, np.inf, c).astype(F), s % 100, e), (c, np.where(np.arange(NLIST) == 1, 100, s % 100), e),
                       (c, np.where(np.arange(NLIST) == 1, -2, s % 100), e), (c, s % 100, np.where(e == e[5, 5], 100, e))):
        assert code_of(lambda: small.set_graph(bc, bs, be)) == inv and not small.ready
    small.set_graph(c, s % 100, e)
    assert code_of(lambda: small.search(q, 11, "ef=10")) == capi.ERR_UNSUPPORTED_K
    assert code_of(lambda: small.search(q, 1, "ef=257")) == inv and code_of(lambda: small.search(q, 1, "width=5")) == inv
    assert code_of(lambda: small.search(q, 1, "nprobe=0")) == inv and code_of(lambda: small.search(q, 1, "max_iters=0")) == inv
    assert small.search(q[:0], 5)[0].shape == (0, 5) and small.search(q, 0)[0].shape == (33, 0)
    for h in (small, other, unit, empty):
        h.close()
