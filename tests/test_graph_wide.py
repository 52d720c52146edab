"""The graph index's wide search (msvs_graph_index_search_wide[_device], capi.GraphIndex.search_wide): ef and k up to 4096, the visited
set in device memory.  The reference is test_graph_index.ref_search (bit_size=8: over the decoded rows); ids ==, distances by their
uint32 view."""
import functools

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import test_graph_index as tg
from test_graph_index import COS, F, IP, L2, data, ref_search, store_of, stored
from test_graph_sq import decode
from test_pq_ivf import blobs, code_of, same

pytestmark = pytest.mark.gpu
INV, BIG_K = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED_K


def device_search_wide(ix, q, k, alive=None, **kw):
    class Wide:  # tg.device_search stages the buffers and calls .search_device
        search_device = staticmethod(ix.search_wide_device)
    return tg.device_search(Wide, q, k, alive, **kw)


@functools.lru_cache(maxsize=None)
def handed(metric, dim, R, bits):
    """tg's handed knn graph over data(dim) -> (index, the rows its search scores)"""
    x, _, cent, _, _ = data(dim)
    ix = capi.GraphIndex(metric, store_of(x, metric), "degree=%d,bit_size=%d" % (R, bits))
    ix.set_graph(cent, *tg.graph(dim, R, "knn"))
    return ix, decode(*ix.export_codes()) if bits == 8 else stored(x, metric)


# ef: the first entry of a thread's second slot, an exact and an off-by-one multiple of 256, and the cap (a beam that never fills:
# n = 2000, so k = 4096 is padded with -1)
EFK = [(257, 257), (512, 10), (513, 300), (1024, 1024), (4096, 4096)]
PARITY = [((L2, IP, COS)[c % 3], (3, 67, 772)[(c // 3) % 3], (16, 64)[c % 2], EFK[c % 5], (1, 4)[(c // 2) % 2], bool((c // 3) % 2),
           (32, 8)[(c // 4) % 2], ("host", "device")[(c // 6) % 2]) for c in range(12)]
assert [len({r[i] for r in PARITY}) for i in range(8)] == [3, 3, 2, 5, 2, 2, 2, 2] and (L2, 67, 64, EFK[3], 4, True, 32, "host") in PARITY
PARITY.append((IP, 67, 64, (2048, 2000), 4, False, 8, "device"))  # eight beam entries a thread, which none of the five ef above takes


@pytest.mark.parametrize("metric,dim,R,efk,width,filtered,bits,entry", PARITY)
def test_wide_parity(metric, dim, R, efk, width, filtered, bits, entry):
    (ef, k), (_, q, cent, _, half) = efk, data(dim)
    (ix, xs), (seeds, nbr), alive = handed(metric, dim, R, bits), tg.graph(dim, R, "knn"), half if filtered else None
    exp = ref_search(xs, cent, seeds, nbr, q[:3], k, metric, ef, 8, width, None, alive)
    if entry == "host":
        got = ix.search_wide(q[:3], k, "ef=%d,width=%d" % (ef, width), alive=alive)
    else:
        got = device_search_wide(ix, q[:3], k, alive, ef=ef, width=width)
    same(got, exp)
    assert (got[0][:, 0] >= 0).all() and (k <= tg.N or (got[0][:, -1] == -1).all())


def test_more_queries_than_blocks():
    """2500 queries: more than the four blocks a CU holds on any device, so a block clears and reuses its table across queries"""
    ix, xs = handed(L2, 3, 16, 32)
    rng = np.random.default_rng(5)
    x, _, cent, _, _ = data(3)
    q = (x[rng.integers(0, tg.N, 2500)] + F(0.2) * rng.standard_normal((2500, 3), dtype=F)).astype(F)
    exp = ref_search(xs, cent, *tg.graph(3, 16, "knn"), q, 300, L2, 300, 8, 1, 6)
    same(ix.search_wide(q, 300, "ef=300,max_iters=6"), exp)


@pytest.mark.parametrize("k,params,filtered", [(10, "ef=64", False), (256, "ef=256,width=4", True)])
def test_wide_equals_narrow(k, params, filtered):
    (ix, _), (_, q, _, _, half) = handed(COS, 67, 64, 32), data(67)
    alive = half if filtered else None
    same(ix.search_wide(q, k, params, alive=alive), ix.search(q, k, params, alive=alive))


def test_wide_visited_limit_ends_the_search(monkeypatch):
    """300000 rows of 12 bytes on a line that approach the query as the label grows, R = 64, width 4, ef = 4096, one query.  Row i
    points at rows i + 4, i + 8, ..., i + 256, so the four parents of an iteration, adjacent labels, bring 256 new labels and every
    round is full: the beam never closes and the search ends by |V| + width * R > MSVS_GRAPH_WIDE_VISITED_MAX after 1023 iterations.
    (With random edges over random rows the reference ends "closed": 1024 iterations are all a beam of 4096 has at width 4 unless
    better rows keep coming.)"""
    monkeypatch.setattr(capi, "GRAPH_VISITED_MAX", capi.GRAPH_WIDE_VISITED_MAX)
    n, R = 300000, 64
    x = np.zeros((n, 3), F)
    x[:, 0] = (n - np.arange(n)) * F(0.001)
    x[0] = 0  # (the query itself)
    nbr = ((np.arange(n)[:, None] + 4 * (1 + np.arange(R))[None]) % n).astype(np.uint32)
    cent, seeds = x[1:5].copy(), np.arange(1, 5, dtype=np.int32)
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=64")
    ix.set_graph(cent, seeds, nbr)
    ends = []
    exp = ref_search(x, cent, seeds, nbr, x[:1], 4096, L2, 4096, 4, 4, 100000, None, ends)
    assert ends == ["visited"]
    same(ix.search_wide(x[:1], 4096, "ef=4096,nprobe=4,width=4,max_iters=100000"), exp)
    ix.close()
    rows.close()


def test_wide_limits_and_errors():
    """(No parameter set reaches the 160 KiB refusal: the largest image, dim = 8192 with bit_size=8 at ef = 4096, is 138368 bytes.)"""
    x, q, cent, _, _ = data(67)
    ix, _ = handed(L2, 67, 16, 32)
    assert code_of(lambda: ix.search_wide(q, 1, "ef=4097")) == INV and code_of(lambda: ix.search_wide(q, 4097)) == BIG_K
    assert code_of(lambda: ix.search_wide(q, 300, "ef=299")) == BIG_K and code_of(lambda: ix.search_wide(q, 1, "width=5")) == INV
    assert code_of(lambda: device_search_wide(ix, q, 1, ef=4097)) == INV and code_of(lambda: device_search_wide(ix, q, 4097)) == BIG_K
    assert code_of(lambda: ix.search(q, 1, "ef=257")) == INV and code_of(lambda: ix.search(q, 257)) == BIG_K  # the narrow entry keeps its limits
    fresh = capi.GraphIndex(L2, ix.rows, "degree=16")
    assert code_of(lambda: fresh.search_wide(q, 1)) == capi.ERR_NOT_READY
    assert ix.search_wide(q[:0], 5)[0].shape == (0, 5) and ix.search_wide(q, 0)[0].shape == (33, 0)
    same(ix.search_wide(q, 300), ix.search_wide(q, 300, "ef=300"))  # the default ef is max(k, 64)
    fresh.close()


# The numpy reference's recall@10 at ef = 2048 under the 5 % filter (223 rows alive), computed on the CPU over ref_build's graph of
# numpy Lloyd centroids: 1.0 (at ef = 256: 0.992 with 5 of 640 slots unfilled; at ef = 1024: 1.0).  DESIGN.md 4.14, "Wide search".
FILTERED_RECALL = 1.0


def test_selective_filter_fills_its_slots():
    """tg.test_built_index_recall's data (4000 x 64 blobs, R = 32, 64 queries), a fixed 5 % of the rows alive, k = 10: the narrow search
    at its largest beam leaves slots unfilled, the wide search at ef = 2048 fills every one."""
    rng = np.random.default_rng(11)
    centres, x = blobs(rng, 4000, 64, 8)
    q = (centres[rng.integers(0, 8, 64)] + F(0.3) * rng.standard_normal((64, 64), dtype=F)).astype(F)
    alive = np.random.default_rng(12).random(4000) < 0.05
    rows = store_of(x, L2)
    ix = capi.GraphIndex(L2, rows, "degree=32,ncentroids=16,kmeans_iters=4")
    ix.build()
    narrow, wide = ix.search(q, 10, "ef=256", alive=alive)[0], ix.search_wide(q, 10, "ef=2048", alive=alive)[0]
    assert (narrow == -1).any() and (wide >= 0).all() and alive[wide].all()
    truth = np.flatnonzero(alive)[tg.o.knn(q, x[alive], 10, tg.o.METRIC_L2)[0]]
    recall = float(np.mean([len(set(t.tolist()) & set(g.tolist())) / 10 for t, g in zip(truth, wide)]))
    print("recall@10 of search_wide at ef = 2048, 5 % alive:", recall, "unfilled narrow slots:", int((narrow == -1).sum()))
    assert recall >= FILTERED_RECALL - 0.02
    ix.close()
    rows.close()
