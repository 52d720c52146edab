"""The two load placements of the canonical re-rank (option rerank_chain; mfma_scan_kernels.hpp: ivf_rerank_kernel and
rerank_all_query): 1 = one prologue round trip, eps formed once, a lane's whole row in flight; 0 = the loads where each step needs
them, row pieces four at a time.  Only loads move: ids and distances are the oracle's bit for bit under both, the same queries
reach the canonical fallback, and the same number of rows is evaluated."""
import numpy as np
import pytest

import myscaledb_amd.capi as capi
from oracle import oracle as o

OM = {capi.METRIC_L2: o.METRIC_L2, capi.METRIC_IP: o.METRIC_IP, capi.METRIC_COSINE: o.METRIC_COSINE}
FORMS = ("1", "0")
NQ, NPROBE = 300, 8  # >= 256 queries: the batched coarse pass


def same(a_ids, a_dis, b_ids, b_dis):
    assert np.array_equal(a_ids, b_ids), "ids differ"
    assert np.array_equal(a_dis.view(np.uint32), b_dis.view(np.uint32)), "distances differ"


def build_ivf(x, metric, nlist, params="", centroids=None):
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, x.shape[1], "ncentroids=%d,kmeans_iters=5%s" % (nlist, params))
    if centroids is not None:
        ix.set_centroids(centroids)
    else:
        ix.train(x)
    half = x.shape[0] // 2
    ix.add(x[:half])
    ix.add(x[half:])
    ix.build()
    return ix


def oracle_on_exported(ix, q, nprobe, k, metric):
    cent, off, vecs, lids = ix.export()
    if metric == capi.METRIC_COSINE:
        oi, od, pr = o.ivf_search(cent, off, vecs, lids, o.normalize_rows(q), nprobe, k, o.METRIC_IP)
        return oi, (np.float32(1) - od).astype(np.float32), pr
    return o.ivf_search(cent, off, vecs, lids, q, nprobe, k, OM[metric])


def clustered(seed, n, d, nlist, nq):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((nlist, d), dtype=np.float32) * 2
    x = (centers[rng.integers(0, nlist, n)] + rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    q = (centers[rng.integers(0, nlist, nq)] + rng.standard_normal((nq, d), dtype=np.float32)).astype(np.float32)
    return x, q


def search_both_forms(ix, q, k, nprobe, opt, oi, od, what="", cap=None):
    """One search per form, each against the oracle; -> {form: (fallbacks, first-stage rows, second-chance rows)} of the search.
    The candidate pass has to be the path that served every query, or the re-rank is not under test.  cap (searches under
    default settings: a tenth of the queries): the most queries that may reach the canonical fallback, in either form."""
    out = {}
    for form in FORMS:
        opt("rerank_chain", form)
        p0, r0 = capi.prefilter_stats(), capi.debug_rerank_rows()
        ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
        p1, r1 = capi.prefilter_stats(), capi.debug_rerank_rows()
        assert p1[0] - p0[0] == len(q), "%s rerank_chain=%s: the candidate pass did not run for all queries" % (what, form)
        same(ids, dis, oi, od)
        out[form] = (p1[1] - p0[1], r1[0] - r0[0], r1[1] - r0[1])
    opt("rerank_chain", None)
    print("%s k=%d (fallbacks, rows first, rows second) chain 1: %s chain 0: %s" % (what, k, out["1"], out["0"]))
    assert out["1"][0] == out["0"][0], "%s: the two forms send different numbers of queries to the canonical fallback" % what
    for form in FORMS:
        assert cap is None or out[form][0] <= cap, "%s rerank_chain=%s k=%d: %d of %d queries fell back" % (what, form, k, out[form][0], len(q))
    return out


# d -> (rows, lists): jfull = d / 64 whole pieces per lane, jtail = (d / 4) % 16 lanes with one more
SHAPES = {20: (20000, 32), 64: (20000, 32), 100: (20000, 32), 760: (6000, 16), 768: (6000, 16), 772: (6000, 16), 1100: (5000, 16),
          1536: (4000, 16), 2432: (3000, 16)}  # 2432: the largest d the shadow list scan serves -- 38 pieces, three batches and two more
KS = (1, 10, 12, 13, 40, 41, 100)  # kc = 32 / 64 / 256 (R = 4); 12 | 13: the edge of the first early-exit round
ROW_CASES = [(d, capi.METRIC_L2, None) for d in SHAPES] + [(d, capi.METRIC_IP, None) for d in SHAPES] \
    + [(d, capi.METRIC_COSINE, None) for d in (64, 768)] + [(d, capi.METRIC_L2, f) for d in (64, 768) for f in ("2", "3")]


@pytest.mark.gpu
@pytest.mark.parametrize("d,metric,h16_form", ROW_CASES)
def test_row_shapes_match_the_oracle_under_both_forms(d, metric, h16_form, opt):
    """Every split of a row into whole pieces and a tail (one batch of twelve at d = 768, two at 1536, a batch and a remainder
    four at a time at 772 and 1100, the four-at-a-time loop alone below 768), every candidate count, L2 / IP / cosine, and the fp16 (2) and int8 residual (3) shadows forced at build time.
    Under default settings at most a tenth of the queries may reach the canonical fallback, in either form.  d = 2432, the largest
    dimension the shadow list scan serves (three batches of twelve pieces and two more): measured on an MI355X, none of the 300
    queries fell back at any k, L2 or IP, in either form -- the cap holds there as it stands."""
    n, nlist = SHAPES[d]
    x, q = clustered(8000 + d, n, d, nlist, NQ)
    if h16_form is not None:
        opt("h16_form", h16_form)
    ix = build_ivf(x, metric, nlist)
    for k in KS:
        oi, od, _ = oracle_on_exported(ix, q, NPROBE, k, metric)
        search_both_forms(ix, q, k, NPROBE, opt, oi, od, "d=%d metric=%d form=%s" % (d, metric, h16_form), cap=NQ // 10)
    ix.close()


@pytest.mark.gpu
def test_short_lists_pad_with_absent_candidates(opt):
    """200 rows in 16 lists, 2 probes: fewer candidates than kc and fewer probed rows than k -- KEY_NONE padding in the
    candidates' LDS copy, -1 ids in the result.  Eight lists of 23 rows and, far away from them, eight of 2: a query near one of
    the small lists probes two of those, 4 rows for a top-10."""
    rng = np.random.default_rng(31)
    centers = rng.standard_normal((16, 64), dtype=np.float32) * 2
    centers[8:, 0] += 100
    lists = np.concatenate([np.repeat(np.arange(8), 23), np.repeat(np.arange(8, 16), 2)])
    x = (centers[lists] + rng.standard_normal((200, 64), dtype=np.float32)).astype(np.float32)
    q = (centers[rng.integers(0, 16, NQ)] + rng.standard_normal((NQ, 64), dtype=np.float32)).astype(np.float32)
    ix = build_ivf(x, capi.METRIC_L2, 16, centroids=centers)
    oi, od, _ = oracle_on_exported(ix, q, 2, 10, capi.METRIC_L2)
    assert (oi < 0).any(), "the data was meant to leave some results empty"
    search_both_forms(ix, q, 10, 2, opt, oi, od, "short lists", cap=NQ // 10)
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 768])
def test_ties_are_broken_by_id(d, opt):
    """Every row stored twice: equal distances at every rank, the ids decide."""
    n, nlist = (8000, 32) if d == 64 else (3000, 16)
    x, q = clustered(77 + d, n, d, nlist, NQ)
    x = np.concatenate([x, x])
    ix = build_ivf(x, capi.METRIC_L2, nlist)
    for k in (10, 13):
        oi, od, _ = oracle_on_exported(ix, q, NPROBE, k, capi.METRIC_L2)
        assert (od[:, 0] == od[:, 1]).all()
        search_both_forms(ix, q, k, NPROBE, opt, oi, od, "ties d=%d" % d, cap=NQ // 10)
    ix.close()


# ivf_eps_scale at which the first certificate fails for many queries and the second chance serves them.  Measured on the data
# of `forced` below with rerank_chain = 0, as (fallbacks without a second chance, fallbacks with it, rows of the first stage, rows
# of the second chance) of the 300 queries: scale 4: (1, 0, 5913, 33); 8: (200, 0, 9165, 7817); 16: (300, 15, 9600, 27056);
# 32 and beyond: (300, 300, 9600, 44403).
EPS_SECOND_CHANCE = "8"


@pytest.fixture(scope="module")
def forced():
    x, q = clustered(4242, 6000, 768, 16, NQ)
    ix = build_ivf(x, capi.METRIC_L2, 16)
    oi, od, _ = oracle_on_exported(ix, q, NPROBE, 10, capi.METRIC_L2)
    yield ix, q, oi, od
    ix.close()


FORCED_SETTINGS = [{"ivf_eps_scale": EPS_SECOND_CHANCE}, {"ivf_eps_scale": "1e12"}, {"rerank_fused": "0"}, {"rerank_fused": "1"},
                   {"rerank_hint": "0"}, {"rerank_early": "0"},
                   {"ivf_eps_scale": EPS_SECOND_CHANCE, "rerank_fused": "0"}, {"ivf_eps_scale": EPS_SECOND_CHANCE, "rerank_hint": "0"},
                   {"ivf_eps_scale": EPS_SECOND_CHANCE, "rerank_early": "0"},
                   {"ivf_eps_scale": EPS_SECOND_CHANCE, "rerank_fused": "0", "rerank_hint": "0"}]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", FORCED_SETTINGS, ids=lambda kn: ",".join("%s=%s" % it for it in kn.items()))
def test_forced_failures_take_the_same_route_in_both_forms(knobs, forced, opt):
    """Certificates made to fail: the bounds are the same in both forms, so the same number of queries reaches the canonical
    fallback (search_both_forms) and, under rerank_stats, both stages evaluate the same number of rows -- nothing is prefetched
    that the early exit or the hint would skip."""
    ix, q, oi, od = forced
    for kn, v in knobs.items():
        opt(kn, v)
    opt("rerank_stats", "1")
    out = search_both_forms(ix, q, 10, NPROBE, opt, oi, od, str(knobs), cap=None if "ivf_eps_scale" in knobs else NQ // 10)
    assert out["1"] == out["0"], "rows evaluated differ between the forms: %s" % (out,)
    assert out["1"][1] > 0, "the first stage evaluated nothing"
    if knobs.get("ivf_eps_scale") == "1e12":
        assert out["1"][0] == NQ  # nobody has a certificate
    elif "ivf_eps_scale" in knobs:
        assert out["1"][2] > 0, "no query took the second chance at this ivf_eps_scale"
        assert out["1"][0] <= NQ // 10, "the second chance was meant to serve the queries whose first certificate fails"
    if knobs.get("ivf_eps_scale") == EPS_SECOND_CHANCE and len(knobs) == 1:
        # how many first certificates fail at this scale: without a second chance all of them take the canonical fallback
        opt("rerank_second", "0")
        first = search_both_forms(ix, q, 10, NPROBE, opt, oi, od, "no second chance")
        assert first["0"][0] >= NQ // 4, "the scale was meant to fail many first certificates"


SIGNAL_NQ = 200  # at most 256 queries through the host entry: the shadow list scan ends with the armed host signal
SIGNAL_SETTINGS = [{"ivf_eps_scale": EPS_SECOND_CHANCE}, {"ivf_eps_scale": EPS_SECOND_CHANCE, "rerank_fused": "0"}, {"ivf_eps_scale": "1e12"}]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", SIGNAL_SETTINGS, ids=lambda kn: ",".join("%s=%s" % it for it in kn.items()))
def test_armed_host_signal_that_comes_back_with_failures(knobs, forced, opt):
    """A host-pointer call of 200 queries arms the signal (`forced`'s 300 never do): the host hears how many queries are without
    a certificate -- after the fused second chance, or in front of the one that is a launch of its own -- and only then enqueues
    what is left of the chain.  With certificates made to fail the count it hears is not zero: the second chance serves most of
    the queries at EPS_SECOND_CHANCE, the canonical fallback all of them at 1e12.  The results are the oracle's and the same
    number of queries reaches the fallback as with every launch enqueued blindly (host_signal_batch = 0)."""
    ix, q, oi, od = forced
    q, oi, od = q[:SIGNAL_NQ], oi[:SIGNAL_NQ], od[:SIGNAL_NQ]
    for kn, v in knobs.items():
        opt(kn, v)
    opt("rerank_stats", "1")
    counts = {}
    for signal in ("1", "0"):
        opt("host_signal_batch", signal)
        p0, r0 = capi.prefilter_stats(), capi.debug_rerank_rows()
        ids, dis = ix.search(q, 10, "nprobe=%d" % NPROBE)
        p1, r1 = capi.prefilter_stats(), capi.debug_rerank_rows()
        assert p1[0] - p0[0] == SIGNAL_NQ, "host_signal_batch=%s: the candidate pass did not run for all queries" % signal
        same(ids, dis, oi, od)
        counts[signal] = (p1[1] - p0[1], r1[1] - r0[1])
    print("%s (fallbacks, rows second) signal armed: %s every launch enqueued: %s" % (knobs, counts["1"], counts["0"]))
    assert counts["1"][0] == counts["0"][0], "the armed signal changed how many queries reach the canonical fallback: %s" % (counts,)
    if knobs["ivf_eps_scale"] == "1e12":
        assert counts["1"][0] == SIGNAL_NQ  # nobody has a certificate
    else:
        assert counts["1"][1] > 0, "no query took the second chance at this ivf_eps_scale"
        assert counts["1"][0] <= SIGNAL_NQ // 10, "the second chance was meant to serve the queries whose first certificate fails"


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_second_chance_skips_the_chunks_the_hint_empties(fused, forced, opt):
    """The second chance walks a query's candidate buffer in chunks of 256 keys; under rerank_chain = 1 a chunk of which the
    first stage's hint leaves no key skips its row loop and its rank pass.  The blown-up bound fails 200 of the 300 first
    certificates; their buffers hold ~150 keys on average, some more than 256, and the hints keep ~40 rows of each, so a few
    second chunks go whole (measured: 4 chunks, fused and as a launch of its own; 7817 rows evaluated in both forms).  The
    skips are counted (debug_rerank_skipped_chunks), the parent form has none, and results, fallbacks and evaluated rows are
    the same in both forms."""
    ix, q, oi, od = forced
    opt("ivf_eps_scale", EPS_SECOND_CHANCE)
    opt("h16_nocut", "1")
    opt("cand_cap", "16384")
    opt("rerank_fused", fused)
    opt("rerank_stats", "1")
    res = {}
    for form in FORMS:
        opt("rerank_chain", form)
        p0, r0, s0 = capi.prefilter_stats(), capi.debug_rerank_rows(), capi.debug_rerank_skipped_chunks()
        ids, dis = ix.search(q, 10, "nprobe=%d" % NPROBE)
        p1, r1, s1 = capi.prefilter_stats(), capi.debug_rerank_rows(), capi.debug_rerank_skipped_chunks()
        assert p1[0] - p0[0] == NQ, "the candidate pass did not run for all queries"
        same(ids, dis, oi, od)
        res[form] = (p1[1] - p0[1], r1[0] - r0[0], r1[1] - r0[1], s1 - s0)
    print("fused=%s (fallbacks, rows first, rows second, chunks skipped) chain 1: %s chain 0: %s" % (fused, res["1"], res["0"]))
    assert res["1"][:3] == res["0"][:3], res
    assert res["1"][2] > 0, "no query took the second chance"
    assert res["0"][3] == 0 and res["1"][3] > 0, "chunks skipped: %s" % (res,)


@pytest.mark.gpu
def test_default_settings_evaluate_the_same_rows(forced, opt):
    """No extra reads under default settings either: the first stage's row count is equal between the forms and not zero."""
    ix, q, oi, od = forced
    opt("rerank_stats", "1")
    out = search_both_forms(ix, q, 10, NPROBE, opt, oi, od, "defaults", cap=NQ // 10)
    assert out["1"][1:] == out["0"][1:] and out["1"][1] > 0, out
    assert out["1"][1] < NQ * 32, "the early exit skipped nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [capi.METRIC_L2, capi.METRIC_IP])
@pytest.mark.parametrize("n,d", [(16000, 96), (8000, 768)])
def test_probe_passes_through_the_block_kernel(n, d, metric, opt):
    """coarse_tail = 0: the coarse quantiser's probe lists come from ivf_rerank_kernel (out_probes, the band, and with the error
    bound blown up the queue behind coarse_tail_kernel through qmap) -- the band reads the candidates' LDS copy under
    rerank_chain = 1.  Duplicate centroids: ties at every rank of the probe selection."""
    nlist, nprobe, k = 256, 16, 10
    rng = np.random.default_rng(900 + d)
    centers = rng.standard_normal((nlist // 2, d), dtype=np.float32) * 2
    centers = np.concatenate([centers, centers])
    x = (centers[rng.integers(0, nlist, n)] + rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    q = (centers[rng.integers(0, nlist, NQ)] + rng.standard_normal((NQ, d), dtype=np.float32)).astype(np.float32)
    ix = build_ivf(x, metric, nlist, centroids=centers)
    oi, od, _ = oracle_on_exported(ix, q, nprobe, k, metric)
    for knobs in ({"coarse_tail": "0"}, {"coarse_tail": "0", "ivf_eps_scale": "1e12"}, {"ivf_eps_scale": "1e12"},
                  {"ivf_eps_scale": "1e12", "coarse_slow_inline": "0"}):
        for kn, v in knobs.items():
            opt(kn, v)
        counts = {}
        for form in FORMS:
            opt("rerank_chain", form)
            c0, p0 = capi.coarse_stats(), capi.prefilter_stats()
            ids, dis = ix.search(q, k, "nprobe=%d" % nprobe)
            c1, p1 = capi.coarse_stats(), capi.prefilter_stats()
            same(ids, dis, oi, od)
            assert p1[0] - p0[0] == NQ, "rerank_chain=%s %s: the candidate pass did not run for all queries" % (form, knobs)
            counts[form] = (c1[0] - c0[0], c1[1] - c0[1], p1[1] - p0[1])
        opt("rerank_chain", None)
        print("d=%d metric=%d %s (coarse queries, coarse fallbacks, result fallbacks) %s" % (d, metric, knobs, counts))
        assert counts["1"] == counts["0"], (knobs, counts)
        assert counts["1"][0] == NQ, "the shadow coarse pass did not run"
        if "ivf_eps_scale" in knobs:
            assert counts["1"][1] == NQ, "every band was meant to fail"
        else:  # default error bound: at most a tenth of the queries may reach the canonical fallback, in either form
            assert counts["1"][2] <= NQ // 10 and counts["0"][2] <= NQ // 10, (knobs, counts)
        for kn in knobs:
            opt(kn, None)
    ix.close()
