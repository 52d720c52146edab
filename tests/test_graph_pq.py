"""The graph index over product-quantised codes (create's pq_m=M, include/msvs.h "Product-quantised rows").

encode / table / row_score restate the definition in f32 numpy; ref_search is test_graph_index.ref_search's beam loop with that
score in place of oracle.knn.  Ids are compared with ==, distances by their uint32 view."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o
from test_graph_index import COS, IP, L2, N, NLIST, NONE, data, device_search, graph, same, store_of, stored
from test_graph_sq import fnv
from test_pq_ivf import blobs, code_of

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(np.float32).max
INV = capi.ERR_INVALID_ARGUMENT
DM = [(8, 8), (34, 17), (66, 33), (96, 1), (768, 96)]  # dsub 1, lanes 8 .. 15 empty | c = 2, lane 8 half full | c = 3 | lane 0 alone | c = 6


def encode(xs, cb):
    """code[s] = argmin_j of the sequential f32 L2 sub-score, ties to the lowest j, NaN never, all NaN -> 0"""
    m, ksub, dsub = cb.shape
    codes = np.zeros((len(xs), m), np.uint8)
    with np.errstate(all="ignore"):
        for s in range(m):
            e = np.zeros((len(xs), ksub), F)
            for t in range(dsub):
                d = xs[:, s * dsub + t, None] - cb[None, s, :, t]
                e = e + d * d
            e[np.isnan(e).all(1)] = 0
            codes[:, s] = np.nanargmin(e, 1)
    return codes


def table(v, cb, ip):
    m, ksub, dsub = cb.shape
    vs, T = v.reshape(m, dsub), np.zeros((m, ksub), F)
    for t in range(dsub):
        d = vs[:, t, None] - cb[:, :, t]
        T = T + (vs[:, t, None] * cb[:, :, t] if ip else d * d)
    return T


def row_score(T, codes):
    """sixteen runs of c = ceil(m / 16) sub-spaces, each summed in order from +0, folded by the adjacent-pairwise tree"""
    m, c = len(T), -(-len(T) // 16)
    p = np.zeros((len(codes), 16), F)
    for s in range(m):
        p[:, s // c] = p[:, s // c] + T[s, codes[:, s]]
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def ref_search(cb, codes, cent, seeds, nbr, q, k, metric, ef, nprobe=8, width=1, max_iters=None, alive=None, cap=capi.GRAPH_VISITED_MAX):
    ip = metric != L2
    om = o.METRIC_IP if ip else o.METRIC_L2
    n, R = nbr.shape
    max_iters = max_iters or -(-2 * ef // width) + 8
    qs = o.normalize_rows(q) if metric == COS else np.ascontiguousarray(q, F)
    ids = np.full((len(qs), k), -1, np.int64)
    dis = np.full((len(qs), k), -FLT_MAX if ip else FLT_MAX, F)
    for qi, v in enumerate(qs):
        T, seen, beam = table(v, cb, ip), set(), []  # beam entries: [(order value, label), expanded, score]

        def score(labels):
            new = [l for l in dict.fromkeys(labels) if l not in seen]
            seen.update(new)
            if new:
                for l, d in zip(new, row_score(T, codes[new])):
                    if (d > -FLT_MAX) if ip else (d < FLT_MAX):  # strictly better than the neutral value; NaN never
                        beam.append([(-float(d) if ip else float(d), l), False, d])
                beam.sort(key=lambda e: e[0])
                del beam[ef:]

        lists = o.knn(v, cent, min(nprobe, len(cent)), om)[0][0]
        score([int(seeds[l]) for l in lists if l >= 0 and seeds[l] >= 0])
        for _ in range(max_iters):
            parents = [e for e in beam if not e[1]][:width]
            if len(seen) + width * R > cap or not parents:
                break
            for e in parents:
                e[1] = True
            score([int(t) for e in parents for t in nbr[e[0][1]] if t != NONE and t < n])
        out = [e for e in beam if alive is None or alive[e[0][1]]][:k]
        ids[qi, :len(out)] = [e[0][1] for e in out]
        dis[qi, :len(out)] = [e[2] for e in out]
    return ids, (F(1) - dis).astype(F) if metric == COS else dis


@functools.lru_cache(maxsize=None)
def codebooks(dim, m, bits):
    return (F(0.7) * np.random.default_rng(dim + 7 * m + bits).standard_normal((m, 1 << bits, dim // m), dtype=F)).astype(F)


def create(metric, rows, m, bits, R=16, more=""):
    return capi.GraphIndex(metric, rows, "degree=%d,pq_m=%d,bit_size=%d%s" % (R, m, bits, more))


def stored_row_bytes(m, bits):
    return 64 if -(-m // 16) * bits <= 32 else 128


# ---------------------------------------------------------------------------------------- 1. codes

@pytest.mark.parametrize("dim,m", DM)
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("metric", [L2, COS])
def test_codes(metric, bits, dim, m):
    cb = codebooks(dim, m, bits)
    x = blobs(np.random.default_rng(dim + m), 600, dim, 6, sigma=0.5)[1]
    x[7] = cb[:, 3].reshape(-1)  # a row that is an entry of every sub-codebook
    x[5] = np.nan
    rows = store_of(x, metric)
    ix = create(metric, rows, m, bits)
    assert ix.pq_m == m and ix.bit_size == bits and not ix.ready and code_of(ix.export_pq) == capi.ERR_NOT_READY
    ix.set_pq_codebooks(cb)
    ix.set_graph(x[:4], np.zeros(4, np.int32), np.full((600, 16), NONE, np.uint32))
    rows.close()
    got_cb, got = ix.export_pq()
    with np.errstate(all="ignore"):
        exp = encode(stored(x, metric), cb)
    assert (got_cb == cb).all() and (got == exp).all(), np.argwhere(got != exp)[:5]
    assert (got[5] == 0).all() and (metric != L2 or (got[7] == 3).all()) and got.max() < 1 << bits
    assert ix.memory_usage == 600 * 16 * 4 + 4 * ((dim + 3) // 4) * 16 + 4 * 4 + 600 * stored_row_bytes(m, bits) + (4 * dim << bits)
    ix.close()


# ---------------------------------------------------------------------------------------- 2. search parity

# metric, bits, (dim, m), R, (ef, k), width, nq, filtered, entry
PARITY = [(L2, 8, DM[4], 32, (64, 10), 1, 33, False, "device"), (IP, 4, DM[4], 16, (64, 10), 4, 33, True, "host"),
          (COS, 8, DM[1], 64, (256, 256), 1, 1, False, "host"), (L2, 4, DM[1], 16, (1, 1), 1, 33, False, "device"),
          (IP, 8, DM[2], 64, (64, 10), 4, 1, True, "device"), (COS, 4, DM[2], 16, (256, 256), 4, 33, False, "host"),
          (L2, 8, DM[0], 16, (256, 256), 4, 33, True, "wide"), (COS, 4, DM[0], 64, (64, 10), 1, 1, False, "wide"),
          (IP, 8, DM[3], 16, (1, 1), 1, 33, False, "host"), (L2, 4, DM[3], 64, (64, 10), 1, 33, True, "device"),
          (L2, 8, DM[2], 16, (1024, 300), 1, 1, False, "wide"), (COS, 8, DM[4], 64, (64, 10), 4, 1, True, "wide")]


@functools.lru_cache(maxsize=None)
def handed(metric, bits, dim, m, R):
    """-> (the index over a CLOSED row store, the codebooks, the definition's codes)"""
    x, cb = data(dim)[0], codebooks(dim, m, bits)
    rows = store_of(x, metric)
    ix = create(metric, rows, m, bits, R)
    ix.set_pq_codebooks(cb)
    ix.set_graph(data(dim)[2], *graph(dim, R, "rnd" if R == 16 else "knn"))
    rows.close()
    return ix, cb, encode(stored(x, metric), cb)


@pytest.mark.parametrize("metric,bits,dm,R,efk,width,nq,filtered,entry", PARITY)
def test_search_parity(metric, bits, dm, R, efk, width, nq, filtered, entry):
    (dim, m), (ef, k), (_, q, cent, _, half) = dm, efk, data(dm[0])
    (ix, cb, codes), (seeds, nbr), alive = handed(metric, bits, dim, m, R), graph(dim, R, "rnd" if R == 16 else "knn"), half if filtered else None
    cap = capi.GRAPH_WIDE_VISITED_MAX if entry == "wide" else capi.GRAPH_VISITED_MAX
    exp = ref_search(cb, codes, cent, seeds, nbr, q[:nq], k, metric, ef, 8, width, None, alive, cap)
    params = "ef=%d,width=%d" % (ef, width)
    if entry == "device":
        got = device_search(ix, q[:nq], k, alive, ef=ef, width=width)
    else:
        got = (ix.search_wide if entry == "wide" else ix.search)(q[:nq], k, params, alive=alive)
    same(got, exp)
    assert (exp[0][:, 0] >= 0).any()


# ---------------------------------------------------------------------------------------- 3. refusals and round trip

def test_refusals():
    x, _, cent, _, _ = data(34)
    seeds, nbr = graph(34, 16, "rnd")
    rows = store_of(x, L2)
    for params in ("pq_m=4", "pq_m=129", "pq_m=17,bit_size=32", "pq_m=17,bit_size=16", "bit_size=4"):
        assert code_of(lambda: capi.GraphIndex(L2, rows, "degree=16," + params)) == INV
    ix = create(L2, rows, 17, 8)
    bad = codebooks(34, 17, 8).copy()
    bad[3, 5, 1] = np.nan
    assert code_of(lambda: ix.set_pq_codebooks(bad)) == INV and code_of(ix.export_codes) == INV
    few = store_of(x[:255], L2)  # n < ksub: nothing to train 256 entries on
    short = create(L2, few, 17, 8, more=",kmeans_iters=2")
    assert code_of(lambda: short.set_graph(cent, seeds % 255, nbr[:255] % 255)) == INV and not short.ready
    plain = capi.GraphIndex(L2, rows, "degree=16")
    assert plain.pq_m == 0 and plain.bit_size == 32 and code_of(plain.export_pq) == INV
    assert code_of(lambda: plain.set_pq_codebooks(bad)) == INV
    for h in (ix, short, plain, few, rows):
        h.close()


def test_round_trip():
    """A nibble or a byte cannot hold a code >= ksub, so the file has no such state to refuse: the pad nibble of an odd m is the one
    place where a 4-bit row can carry a bit the codes do not own."""
    dim, m, R = 34, 17, 16
    (ix, cb, codes), q = handed(L2, 4, dim, m, R), data(dim)[1]
    first, files = ix.search(q, 10, "ef=40,width=2"), {}
    ix.serialize_io(files)
    raw = bytes(files["graph_data"])
    sizes = [NLIST * dim * 4, NLIST * 4, N * R * 4, 16, 16 * dim * 4, N * 9]
    assert struct.unpack_from("<I", raw, 8)[0] == 3 and len(raw) == 64 + sum(sizes)
    assert struct.unpack_from("<2Q", raw, 64 + sum(sizes[:3])) == (m, 4)
    back = capi.GraphIndex.load_io(files)
    assert back.pq_m == m and back.bit_size == 4 and back.memory_usage == ix.memory_usage
    assert all((a == b).all() for a, b in zip(back.export() + back.export_pq(), ix.export() + (cb, codes)))
    same(back.search(q, 10, "ef=40,width=2"), first)
    back.close()

    def signed(b):
        parts = np.cumsum([64] + sizes)
        b[48:56] = struct.pack("<Q", fnv(struct.pack("<6Q", *[fnv(b[a:c]) for a, c in zip(parts, parts[1:])])))
        b[56:64] = struct.pack("<Q", fnv(b[:56]))
        return {"graph_data": b}

    flipped, pad, geometry, short = bytearray(raw), bytearray(raw), bytearray(raw), bytearray(raw[:-1])
    flipped[-3] ^= 0x10   # a code, the checksums as they were
    pad[-1] |= 0x10       # the last row's pad nibble under valid checksums
    geometry[64 + sum(sizes[:3])] = 16  # m = 16 does not divide 34
    assert capi.GraphIndex.load_io(signed(bytearray(raw))).pq_m == m  # (signed() signs as the library does)
    for b in ({"graph_data": flipped}, signed(pad), signed(geometry), {"graph_data": short}):
        assert code_of(lambda: capi.GraphIndex.load_io(b)) == capi.ERR_IO
    # versions 1 and 2 are written and read as before
    rows = store_of(data(dim)[0], L2)
    for params, version in (("degree=16", 1), ("degree=16,bit_size=8", 2)):
        old, out = capi.GraphIndex(L2, rows, params), {}
        old.set_graph(data(dim)[2], *graph(dim, R, "rnd"))
        old.serialize_io(out)
        again = capi.GraphIndex.load_io(out, rows)
        assert struct.unpack_from("<I", out["graph_data"], 8)[0] == version and again.pq_m == 0
        same(again.search(q, 10, "ef=40"), old.search(q, 10, "ef=40"))
        old.close()
        again.close()
    rows.close()


# ---------------------------------------------------------------------------------------- 4. a built index, end to end

# recall@10 of the numpy reference's search(k = 100) followed by refine, over the structure the first GPU run exported: 0.985 at
# pq_m=16 / 8 bits and 0.858 at pq_m=32 / 4 bits (IVFPQ at kc = 100 on this data: 0.992 - 1.000, tests/test_refine.py).  The floors
# are those values rounded down to a multiple of 0.05.
PQ_RECALL = {(8, 16): 0.95, (4, 32): 0.85}


@pytest.mark.parametrize("bits,m", list(PQ_RECALL))
def test_built_index(bits, m):
    """test_refine's data (seed 11, 4000 x 64, 8 blobs, 100 queries): training is deterministic, the search equals the reference over
    the exported structure, and search(k = 100) + refine against the row store reaches its floor in PQ_RECALL."""
    rng = np.random.default_rng(11)
    centres, x = blobs(rng, 4000, 64, 8)
    q = (centres[rng.integers(0, 8, 100)] + F(0.3) * rng.standard_normal((100, 64), dtype=F)).astype(F)
    truth = np.argsort(((q[:, None, :].astype(np.float64) - x[None]) ** 2).sum(-1), axis=1, kind="stable")[:, :10]
    rows, out = store_of(x, L2), []
    for _ in range(2):
        ix = create(L2, rows, m, bits, 32, ",ncentroids=16,kmeans_iters=4")
        ix.build()
        out.append(ix.export() + ix.export_pq())
        if len(out) == 1:
            ix.close()
    assert all((a == b).all() for a, b in zip(*out))
    cent, seeds, nbr, cb, codes = out[0]
    assert (codes == encode(x, cb)).all()
    ref = ref_search(cb, codes, cent, seeds, nbr, q, 100, L2, 100)
    got = ix.search(q, 100)
    same(got, ref)
    recall = lambda ids: float(np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, ids)]))
    measured = recall(capi.refine(rows, L2, q, ref[0], 10)[0])
    print("pq%d:%d recall@10 of search(k = 100) + refine: %.3f (the first stage's own top 10: %.3f)" % (bits, m, measured, recall(ref[0][:, :10])))
    assert measured >= PQ_RECALL[bits, m]
    ix.close()
    rows.close()
