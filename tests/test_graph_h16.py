"""The graph index over binary16 rows (bit_size=16, graph_score_h16): every search against test_graph_index.ref_search over the
rows decoded by numpy's float16, the IEEE conversion of include/msvs.h.  ids ==, distances by their uint32 view."""
import functools
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_graph_index as tg
from test_graph_index import COS, F, IP, L2, blobs, data, device_search, graph, ref_search, same, store_of, stored
from test_graph_sq import fnv
from test_pq_ivf import code_of

pytestmark = pytest.mark.gpu
N, NLIST = tg.N, tg.NLIST


def decode(xs):
    with np.errstate(over="ignore"):
        return np.float16(xs).astype(F)


def usage(dim, R):
    return N * R * 4 + NLIST * ((dim + 3) // 4) * 16 + NLIST * 4 + N * 2 * ((dim + 15) // 16 * 16)


# dims: pad inside one word, tail only, exactly one permuted block, six blocks and a tail; 2049: the long-row form; three wide cases
DIMS = [3, 67, 128, 772]
EFK = [(1, 1), (64, 10), (256, 256)]
PARITY = [((L2, IP, COS)[c % 3], DIMS[c % 4], (16, 64)[(c // 2) % 2], EFK[(c // 3) % 3], (1, 4)[(c // 4) % 2], (1, 33)[c % 2], bool((c // 6) % 2),
           ("host", "device")[(c // 8) % 2], ("knn", "rnd")[(c // 3) % 2]) for c in range(16)]
PARITY.append((L2, 2049, 64, (64, 10), 4, 5, True, "device", "rnd"))
PARITY += [(L2, 772, 64, (300, 300), 4, 3, False, "wide", "knn"), (COS, 67, 16, (300, 300), 1, 3, False, "wide", "knn"),
           (IP, 128, 64, (4096, 10), 4, 3, True, "wide", "knn")]
assert [len({r[i] for r in PARITY[:16]}) for i in range(9)] == [3, 4, 2, 3, 2, 2, 2, 2, 2]


@functools.lru_cache(maxsize=None)
def handed(metric, dim, R, kind):
    """a binary16 index over tg's handed graph -> (index, its decoded rows); the store is closed: no search may read it"""
    x, _, cent, _, _ = data(dim)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=%d,bit_size=16" % R)
    ix.set_graph(cent, *graph(dim, R, kind))
    rows.close()
    assert ix.ready and ix.num_data == N and ix.bit_size == 16 and ix.memory_usage == usage(dim, R)
    return ix, decode(stored(x, metric))


@pytest.mark.parametrize("metric,dim,R,efk,width,nq,filtered,entry,kind", PARITY)
def test_search_parity(metric, dim, R, efk, width, nq, filtered, entry, kind):
    (ef, k), (_, q, cent, _, half) = efk, data(dim)
    (ix, xhat), (seeds, nbr), alive = handed(metric, dim, R, kind), graph(dim, R, kind), half if filtered else None
    exp = ref_search(xhat, cent, seeds, nbr, q[:nq], k, metric, ef, 8, width, None, alive)
    if entry == "device":
        got = device_search(ix, q[:nq], k, alive, ef=ef, width=width)
    else:
        got = (ix.search if entry == "host" else ix.search_wide)(q[:nq], k, "ef=%d,width=%d" % (ef, width), alive=alive)
    same(got, exp)
    assert filtered or (exp[0][:, 0] >= 0).all()


@pytest.mark.parametrize("metric", [L2, IP])
def test_values_at_the_edges_of_binary16(metric):
    # rows around label 40, the only seed: +-inf by overflow, the ties 1 + 2^-11 -> 1 and 65520 -> inf, subnormals, +-0, a NaN
    x, q, cent, order, _ = (a.copy() for a in data(67))
    near = order[40, 1:8]
    x[near[0], 3], x[near[1], 3], x[near[2], :2] = 70000.0, -1e6, (1 + 2.0 ** -11, 65520.0)
    x[near[3], :4] = (2.0 ** -24, 3 * 2.0 ** -25, -5 * 2.0 ** -26, 2.0 ** -15 + 2.0 ** -25)  # the smallest; a tie; below 2^-14
    x[near[4], :3], x[near[5], 7] = (2.0 ** -26, -1e-10, 2.0 ** -25), np.nan                 # below the smallest one; its tie -> 0
    q[0] = x[40]
    seeds, nbr = graph(67, 16, "knn")
    seeds = np.full_like(seeds, 40)
    rows = store_of(x, metric)
    ix = capi.GraphIndex(metric, rows, "degree=16,bit_size=16")
    ix.set_graph(cent, seeds, nbr)
    rows.close()
    xhat = decode(x)
    assert np.isinf(xhat[near[:3]]).sum() == 3 and xhat[near[2], 0] == 1 and (xhat[near[4], :3] == 0).all() and xhat[near[3], 0] == 2.0 ** -24
    with np.errstate(all="ignore"):
        exp = ref_search(xhat, cent, seeds, nbr, q[:2], 64, metric, 64)
    same(ix.search(q[:2], 64, "ef=64"), exp)
    ix.close()


def test_store_independence_file_and_refusals():
    dim, R, how = 67, 16, "ef=40,width=2"
    x, q, cent, _, _ = data(dim)
    seeds, nbr = graph(dim, R, "rnd")
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=16,bit_size=16")
    ix.set_graph(cent, seeds, nbr)
    first = ix.search(q, 10, how)
    rows.close()
    same(ix.search(q, 10, how), first)
    same(first, ref_search(decode(x), cent, seeds, nbr, q, 10, L2, 40, 8, 2))
    assert ix.bit_size == 16 and ix.memory_usage == usage(dim, R) and code_of(ix.export_codes) == capi.ERR_INVALID_ARGUMENT
    assert code_of(lambda: capi.GraphIndex(L2, rows, "pq_m=1,bit_size=16")) == capi.ERR_INVALID_ARGUMENT
    files = {}
    ix.serialize_io(files)
    blob = bytes(files["graph_data"])
    assert struct.unpack_from("<I", blob, 8)[0] == 4 and len(blob) == 64 + NLIST * dim * 4 + NLIST * 4 + N * R * 4 + N * dim * 2
    assert (np.frombuffer(blob[-N * dim * 2:], np.uint16) == np.float16(x).view(np.uint16).ravel()).all()  # natural order
    back = capi.GraphIndex.load_io(files)
    assert back.bit_size == 16 and back.dim == dim and back.memory_usage == ix.memory_usage
    same(back.search(q, 10, how), first)
    assert code_of(lambda: capi.GraphIndex.load_io({"graph_data": bytearray(blob[:-2])})) == capi.ERR_IO
    # versions 1 and 2 write the bytes they wrote before this form existed (FNV-1a of the file, computed on the parent commit)
    for params, size, want in (("degree=16", 132416, 0x7e09568946c6bb16), ("degree=16,bit_size=8", 266952, 0xa24a251a3574246c)):
        rows, old = store_of(x, L2), {}
        was = capi.GraphIndex(L2, rows, params)
        was.set_graph(cent, seeds, nbr)
        was.serialize_io(old)
        assert len(old["graph_data"]) == size and fnv(old["graph_data"]) == want
        was.close()
        rows.close()
    ix.close()
    back.close()


RECALL = 0.996875  # the numpy reference's recall@10 at ef = 64 over the decoded rows, computed on the CPU ("binary16 rows")


def test_built_index():
    """tg.test_built_index_recall's data.  The reference's recall@10 against the exact f32 top-10 at ef = 64 (measured: 0.996875; the
    f32 rows give 1.0) is asserted at that figure minus 0.02: the trainer's centroids only choose seeds."""
    rng = np.random.default_rng(11)
    centres, x = blobs(rng, 4000, 64, 8)
    q = (centres[rng.integers(0, 8, 64)] + F(0.3) * rng.standard_normal((64, 64), dtype=F)).astype(F)
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=32,ncentroids=16,kmeans_iters=4,bit_size=16")
    ix.build()
    rows.close()
    ref = ref_search(decode(x), *ix.export(), q, 10, L2, 64)
    same(ix.search(q, 10, "ef=64"), ref)
    truth = tg.o.knn(q, x, 10, tg.o.METRIC_L2)[0]
    recall = float(np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, ref[0])]))
    assert recall >= RECALL - 0.02
    ix.close()
