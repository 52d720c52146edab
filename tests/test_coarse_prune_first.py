"""coarse_tail_kernel's prune-first path (option coarse_prune_first, round 12): the pre-pruning of a batched L2 IVFFLAT search decided on
all the coarse words before the top-nprobe selection, for the queries whose pruned probe list follows from the words alone.

Every case compares (1) ids and distances with the oracle, (2) with coarse_prune_first = 0 (the select + band, then the pre-pruning
launch for every query), (3) the pruned probe lists and the bound upre with option 0 bit for bit, for every served query whose band
formed under option 0, and (4) the served counter with what the case must give -- a case cannot pass by never taking the path.

The path needs the centroid-shadow coarse pass (nlist >= 256, nprobe <= 40, >= 192 queries): the shapes with 64 lists or 64 probes
must not take it and must give the same results."""
import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

pytestmark = pytest.mark.gpu

D, NQ = 96, 260  # 260 queries: past the 256 of the workgroup-tiled coarse product, not a multiple of 4
SHAPES = [(2, 10), (32, 1), (32, 10), (64, 10)]  # (nprobe, k)
_DATA = {}


def eligible(nlist, nprobe):
    return nlist >= 256 and 2 <= nprobe <= 40


def blob_rows(rng, centers, n, sigma, counts=None):
    """n rows around the centres; counts: {centre: exact number of rows} (the others share the rest evenly at random)."""
    counts = counts or {}
    free = np.array([c for c in range(len(centers)) if c not in counts])
    lab = [np.full(m, c) for c, m in counts.items()]
    lab.append(free[rng.integers(0, len(free), n - sum(counts.values()))])
    lab = np.concatenate(lab)
    return (centers[lab] + sigma * rng.standard_normal((n, D), dtype=np.float32)).astype(np.float32)


def data(kind, nlist):
    """-> (centroids, rows, queries, info) of a case, made once per (kind, nlist) and left unchanged."""
    key = (kind, nlist)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(1200 + 17 * nlist + sum(map(ord, kind)))
    n = 30000
    info = {}
    if kind == "iid":
        x = rng.standard_normal((n, D), dtype=np.float32)
        cent = x[rng.choice(n, nlist, replace=False)].copy()
        q = rng.standard_normal((NQ, D), dtype=np.float32)
    elif kind == "straddle":
        # twice as many blobs as centroids: centroid j sits between blobs 2j and 2j + 1, which are |delta_j| = 0.5 .. 12 away from it --
        # lists of every width; a query next to a wide pair cannot prune anybody (more than 64 members), one next to a narrow pair
        # keeps the widest lists as members that classify OUT
        base = 2 * rng.standard_normal((nlist, D), dtype=np.float32)
        delta = rng.standard_normal((nlist, D), dtype=np.float32)
        delta *= (np.linspace(0.5, 12.0, nlist, dtype=np.float32) / np.linalg.norm(delta, axis=1))[:, None]
        blobs = np.concatenate([base + delta, base - delta]).astype(np.float32)
        cent = base
        x = blob_rows(rng, blobs, n, 0.3)
        q = (blobs[rng.integers(0, 2 * nlist, NQ)] + 0.3 * rng.standard_normal((NQ, D), dtype=np.float32)).astype(np.float32)
        q[:8] *= 0.02  # next to the origin, about as far from every centroid: nothing is prunable
    else:
        cent = 2 * rng.standard_normal((nlist, D), dtype=np.float32)
        counts = None
        near = rng.integers(0, nlist, NQ)
        if kind == "awkward":
            # list 9 has 3 rows (shorter than k = 10), list 7 exactly 10; centroid 5 is moved next to centroid 6, 6 units away: every
            # row of blob 6 is nearer to its own centroid -- list 5 is empty and among the near ones of the queries around blob 6
            cent[5] = cent[6] + 6.0 * np.eye(D, dtype=np.float32)[0]
            counts = {9: 3, 7: 10, 5: 0}
            near[:90] = np.repeat([9, 7, 6], 30)
            info["short"] = np.arange(30)  # the queries whose nearest list is shorter than k = 10
        if kind == "dup":
            cent[nlist // 2:] = cent[: nlist - nlist // 2]  # every centroid twice: equal words at every rank
        x = blob_rows(rng, cent, n, 0.3, counts)
        q = (cent[near] + 0.3 * rng.standard_normal((NQ, D), dtype=np.float32)).astype(np.float32)
        if kind == "degenerate":
            q[3] = 0.0
            q[100, 5] = np.inf
            q[200, 95] = np.nan
            info["bad"] = np.array([100, 200])
    _DATA[key] = (cent, x, q, info)
    return _DATA[key]


def build(cent, x):
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, D, "ncentroids=%d" % len(cent))
    ix.set_centroids(cent)
    ix.add(x)
    ix.build()
    return ix


def same(a_ids, a_dis, b_ids, b_dis):
    assert (a_ids == b_ids).all(), np.argwhere(a_ids != b_ids)[:5]
    assert (a_dis.view(np.uint32) == b_dis.view(np.uint32)).all()


def search_both(opt, ix, q, nprobe, k):
    """One search with the default (prune first), one with coarse_prune_first = 0; the four comparisons but the oracle's.
    -> (ids, distances, served mask)."""
    nq = len(q)
    opt("coarse_prune_debug", "1")
    s0 = capi.debug_prune_first_served()
    ids1, dis1 = ix.search(q, k, "nprobe=%d" % nprobe)
    have1, p1, u1, f1 = capi.debug_prune_first(nq, nprobe)
    s1 = capi.debug_prune_first_served()
    opt("coarse_prune_first", "0")
    ids0, dis0 = ix.search(q, k, "nprobe=%d" % nprobe)
    have0, p0, u0, f0 = capi.debug_prune_first(nq, nprobe)
    assert capi.debug_prune_first_served() == s1  # option 0 never takes the path
    opt("coarse_prune_first", None)
    same(ids1, dis1, ids0, dis0)
    served = (f1 & 1) != 0
    assert not (f0 & 1).any()
    assert s1 - s0 == served.sum()
    if served.any():
        assert have1 and have0
        both = served & ((f0 & 2) != 0)  # served, and the band formed under option 0: the same lists and bounds bit for bit
        print("served %d of %d, of them with a band under option 0: %d; pairs kept per served query %.2f"
              % (served.sum(), nq, both.sum(), (p1[served] >= 0).sum() / served.sum()))
        assert (p1[both] == p0[both]).all(), np.argwhere(p1 != p0)[:5]
        assert (u1.view(np.uint32)[both] == u0.view(np.uint32)[both]).all()
    return ids1, dis1, served


def oracle(ix, q, nprobe, k):
    cent, off, vecs, lids = ix.export()
    oi, od, _ = o.ivf_search(cent, off, vecs, lids, q, nprobe, k, o.METRIC_L2)
    return oi, od


@pytest.mark.parametrize("nprobe,k", SHAPES)
@pytest.mark.parametrize("nlist", [64, 256])
@pytest.mark.parametrize("kind", ["blobs", "iid", "straddle", "awkward", "dup", "degenerate"])
def test_prune_first_matches_the_oracle_and_the_two_launch_form(kind, nlist, nprobe, k, opt):
    cent, x, q, info = data(kind, nlist)
    ix = build(cent, x)
    ids, dis, served = search_both(opt, ix, q, nprobe, k)
    oi, od = oracle(ix, q, nprobe, k)
    same(ids, dis, oi, od)
    ns = int(served.sum())
    if not eligible(nlist, nprobe) or kind == "iid":
        assert ns == 0  # (iid: nothing is prunable -- more than 64 members)
    elif kind == "blobs":
        assert ns == NQ  # one centroid per blob: the nearest list is the only member
    elif kind == "straddle":
        assert 0 < ns < NQ and not served[:8].any()
    elif kind == "awkward":
        assert ns > 0
        if k == 10:
            assert not served[info["short"]].any()  # no bound from a nearest list with fewer than k rows
    elif kind == "dup":
        assert ns > 0
    elif kind == "degenerate":
        assert ns > 0 and not served[info["bad"]].any()  # (Inf / NaN norms: not served; the zero query: whatever its words say)
    ix.close()


def test_feedback_gate_iid_batch_then_blobs_batch(opt):
    """The attempt is skipped while the plan's feedback word says the last search of the shape kept many pairs per query: an iid batch
    (far from every blob: nothing prunable), then batches around the blobs, on one index -- right whichever path each took, and the
    path is back once a search of the shape has come out with few pairs."""
    cent, x, qb, _ = data("blobs", 256)
    rng = np.random.default_rng(77)
    qi = rng.standard_normal((NQ, D), dtype=np.float32)
    ix = build(cent, x)
    nprobe, k = 32, 10
    total = 0
    for q in (qi, qb, qb, qb):
        ids, dis, served = search_both(opt, ix, q, nprobe, k)
        oi, od = oracle(ix, q, nprobe, k)
        same(ids, dis, oi, od)
        total += int(served.sum())
    assert served.sum() == NQ  # the last blobs batch
    assert total >= NQ
    ix.close()
