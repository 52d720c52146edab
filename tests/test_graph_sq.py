"""The graph index over 8-bit codes (bit_size=8; graph_kernels.hpp's coded score step, graph_index.hip): quantiser and codes against a
numpy encode in f32, the search against test_graph_index.ref_search over the DECODED rows.  ids ==, distances by their uint32 view."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_graph_index as tg
from test_graph_index import COS, F, IP, L2, NONE, blobs, device_search, ref_search, same, store_of, stored
from test_pq_ivf import code_of

pytestmark = pytest.mark.gpu
N, NLIST = tg.N, tg.NLIST
INV = capi.ERR_INVALID_ARGUMENT


def encode(xs):
    """include/msvs.h's quantiser and codes of the stored rows, every operation rounded to f32 -> (vmin, vmax, codes)"""
    with np.errstate(all="ignore"):
        vmin, vmax = np.nanmin(xs, 0).astype(F), np.nanmax(xs, 0).astype(F)
        step = ((vmax - vmin) / F(255)).astype(F)
        t = ((xs - vmin) / step).astype(F)
        codes = np.clip(np.rint(t), 0, 255)
    codes[np.isnan(t) | (step == 0)] = 0
    return vmin, vmax, codes.astype(np.uint8)


def decode(vmin, vmax, codes):
    step = ((vmax - vmin) / F(255)).astype(F)
    return (vmin + (codes.astype(F) * step).astype(F)).astype(F)


def pad16(dim):
    return (dim + 15) // 16 * 16


# ---------------------------------------------------------------------------------------- 1. quantiser and codes

@pytest.mark.parametrize("dim", [3, 67, 256, 772])  # a pad inside one word, a tail only, one permuted block, three blocks and a tail
@pytest.mark.parametrize("metric", [L2, COS])
def test_quantiser_and_codes(metric, dim):
    rng = np.random.default_rng(40 + dim)
    _, x = blobs(rng, 600, dim, 6, sigma=0.5)
    x[:, 1] = 0       # a constant column: step 0 (cosine keeps a zero column zero)
    x[7, 0] = np.nan  # (cosine: the whole row is NaN once normalised)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=16,bit_size=8")
    ix.set_graph(x[20:24], np.arange(4, dtype=np.int32), np.full((600, 16), NONE, np.uint32))
    got, exp = ix.export_codes(), encode(stored(x, metric))
    assert ix.bit_size == 8 and all((g == e).all() for g, e in zip(got, exp)), [np.argwhere(g != e)[:5] for g, e in zip(got, exp)]
    assert got[2].min() == 0 and got[2].max() == 255 and (got[2][:, 1] == 0).all() and got[2][7, 0] == 0
    ix.close()
    rows.close()


# ---------------------------------------------------------------------------------------- 2. search parity with handed graphs

DIMS = [3, 67, 256, 772]
EFK = [(1, 1), (64, 10), (256, 256)]
PARITY = [((L2, IP, COS)[c % 3], DIMS[c % 4], (16, 64)[(c // 2) % 2], EFK[(c // 3) % 3], (1, 4)[(c // 4) % 2], (1, 33)[c % 2], bool((c // 6) % 2),
           ("host", "device")[(c // 8) % 2], ("knn", "rnd")[(c // 3) % 2]) for c in range(16)]
PARITY.append((L2, 2049, 64, (64, 10), 4, 5, True, "device", "rnd"))  # nine units a row: the long-row form of the score step
assert [len({r[i] for r in PARITY[:16]}) for i in range(9)] == [3, 4, 2, 3, 2, 2, 2, 2, 2]


@functools.lru_cache(maxsize=None)
def handed(metric, dim, R, kind):
    """a coded index over tg's handed graph -> (index, its decoded rows); the store is closed: no search may read it"""
    x, _, cent, _, _ = tg.data(dim)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d,bit_size=8" % R)
    ix.set_graph(cent, *tg.graph(dim, R, kind))
    rows.close()
    assert ix.ready and ix.num_data == N and ix.bit_size == 8
    assert ix.memory_usage == N * R * 4 + NLIST * ((dim + 3) // 4) * 16 + NLIST * 4 + N * pad16(dim) + 2 * pad16(dim) * 4
    return ix, decode(*ix.export_codes())


@pytest.mark.parametrize("metric,dim,R,efk,width,nq,filtered,entry,kind", PARITY)
def test_search_parity(metric, dim, R, efk, width, nq, filtered, entry, kind):
    (ef, k), (_, q, cent, _, half) = efk, tg.data(dim)
    (ix, xhat), (seeds, nbr), alive = handed(metric, dim, R, kind), tg.graph(dim, R, kind), half if filtered else None
    exp = ref_search(xhat, cent, seeds, nbr, q[:nq], k, metric, ef, 8, width, None, alive)
    if entry == "host":
        got = ix.search(q[:nq], k, "ef=%d,width=%d" % (ef, width), alive=alive)
    else:
        got = device_search(ix, q[:nq], k, alive, ef=ef, width=width)
    same(got, exp)
    assert filtered or (exp[0][:, 0] >= 0).all()


# ---------------------------------------------------------------------------------------- 3. independence and round trip

def fnv(b):
    h = 0xcbf29ce484222325
    for c in bytes(b):
        h = ((h ^ c) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def test_store_independence_round_trip_and_refusals():
    dim, R = 67, 16
    x, q, cent, _, _ = tg.data(dim)
    seeds, nbr = tg.graph(dim, R, "rnd")
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=16,bit_size=8")
    ix.set_graph(cent, seeds, nbr)
    first = ix.search(q, 10, "ef=40,width=2")
    rows.close()
    same(ix.search(q, 10, "ef=40,width=2"), first)
    files = {}
    ix.serialize_io(files)
    data = bytes(files["graph_data"])
    sizes = [NLIST * dim * 4, NLIST * 4, N * R * 4, dim * 4, dim * 4, N * dim]
    assert struct.unpack_from("<I", data, 8)[0] == 2 and len(data) == 64 + sum(sizes)
    back = capi.GraphIndex.load_io(files)
    assert back.bit_size == 8 and back.metric == L2 and back.dim == dim and back.memory_usage == ix.memory_usage
    assert all((a == b).all() for a, b in zip(back.export() + back.export_codes(), ix.export() + ix.export_codes()))
    same(back.search(q, 10, "ef=40,width=2"), first)
    back.close()
    flipped = bytearray(data)
    flipped[-3] ^= 0x10  # a code
    assert code_of(lambda: capi.GraphIndex.load_io({"graph_data": flipped})) == capi.ERR_IO
    nan_bound = bytearray(data)  # vmin[2] = NaN under valid checksums: the bounds' own check
    at = 64 + sum(sizes[:3]) + 8
    nan_bound[at:at + 4] = struct.pack("<f", np.nan)
    parts = np.cumsum([64] + sizes)
    nan_bound[48:56] = struct.pack("<Q", fnv(struct.pack("<6Q", *[fnv(nan_bound[a:b]) for a, b in zip(parts, parts[1:])])))
    nan_bound[56:64] = struct.pack("<Q", fnv(nan_bound[:56]))
    assert code_of(lambda: capi.GraphIndex.load_io({"graph_data": nan_bound})) == capi.ERR_IO
    other = store_of(x[:100], L2)
    assert code_of(lambda: capi.GraphIndex.load_io(files, other)) == capi.ERR_IO  # a store is checked for n
    y = x.copy()
    y[5, 3] = np.inf
    infs = store_of(y, L2)
    bad = capi.GraphIndex(L2, infs, "degree=16,bit_size=8")
    assert code_of(lambda: bad.set_graph(cent, seeds, nbr)) == INV and not bad.ready
    assert code_of(lambda: capi.GraphIndex(L2, infs, "bit_size=7")) == INV
    # bit_size=32 is the index as it was
    plain, named = capi.GraphIndex(L2, infs, "degree=16"), capi.GraphIndex(L2, infs, "degree=16,bit_size=32")
    out = []
    for h in (plain, named):
        h.set_graph(cent, seeds, nbr)
        out.append({})
        h.serialize_io(out[-1])
        assert h.bit_size == 32 and code_of(h.export_codes) == INV
    assert bytes(out[0]["graph_data"]) == bytes(out[1]["graph_data"]) and struct.unpack_from("<I", out[0]["graph_data"], 8)[0] == 1
    assert plain.memory_usage == named.memory_usage == N * R * 4 + NLIST * ((dim + 3) // 4) * 16 + NLIST * 4
    for h in (ix, bad, plain, named, infs, other):
        h.close()


# ---------------------------------------------------------------------------------------- 4. a built index

RECALL = 0.9734375  # the numpy reference's recall@10 at ef = 64, computed on the CPU ("Coded rows")


def test_built_index():
    """tg.test_built_index_recall's data (4000 x 64 blobs, R = 32, 64 queries).  The coded search equals the reference over the
    exported structure and codes bit for bit; the reference's recall@10 against the exact f32 top-10 at ef = 64 is asserted at the
    CPU figure minus 0.02, a margin that covers nothing on the GPU side."""
    rng = np.random.default_rng(11)
    centres, x = blobs(rng, 4000, 64, 8)
    q = (centres[rng.integers(0, 8, 64)] + F(0.3) * rng.standard_normal((64, 64), dtype=F)).astype(F)
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=32,ncentroids=16,kmeans_iters=4,bit_size=8")
    ix.build()
    rows.close()
    cent, seeds, nbr = ix.export()
    vmin, vmax, codes = ix.export_codes()
    assert all((g == e).all() for g, e in zip((vmin, vmax, codes), encode(x)))
    ref = ref_search(decode(vmin, vmax, codes), cent, seeds, nbr, q, 10, L2, 64)
    same(ix.search(q, 10, "ef=64"), ref)
    truth = tg.o.knn(q, x, 10, tg.o.METRIC_L2)[0]
    recall = float(np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, ref[0])]))
    print("reference recall@10 at ef = 64 over the decoded rows:", recall)
    assert recall >= RECALL - 0.02
    ix.close()
