"""Searches with more than MSVS_MAX_K = 256 results (k <= MSVS_MAX_K_ROUNDS = 4096): the BM25 entries (exact rank-window rounds
over the whole batch), the device fusion of long lists, and the vector device entries.  Everything is held against the CPU
oracle / the host fusion: ids exactly, scores by their bits."""
import os
import re

import numpy as np
import pytest

import myscaledb_amd.capi as capi
import myscaledb_amd.host as mhost
from oracle import oracle as o

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------- not GPU

def test_max_k_rounds_constant_agrees_with_the_header():
    assert capi.MAX_K_ROUNDS == 4096
    text = open(os.path.join(ROOT, "include", "msvs.h")).read()
    assert int(re.search(r"#define\s+MSVS_MAX_K_ROUNDS\s+(\d+)", text).group(1)) == capi.MAX_K_ROUNDS
    assert int(re.search(r"#define\s+MSVS_MAX_K\s+(\d+)", text).group(1)) == capi.MAX_K


# ---------------------------------------------------------------------------------------- BM25

N_DOCS, VOCAB, N_TIED = 8000, 40, 700
# terms by what they match: 0 more than 4096 documents, 1 ~1500, 2 ~400, 3 ~100, 4 exactly 256, 5 exactly 512, 6 none,
# 7 the N_TIED first documents with tf 1 (they share one field length: one score), 8 .. 39 a few hundred to 3000 each
T_BIG, T_MID, T_400, T_100, T_256, T_512, T_NONE, T_TIED = range(8)


def make_corpus(seed, num_fields=1):
    """(post_off, doc, tf, fn [num_fields, N_DOCS], term_field, tokens [num_fields]); term id = field * VOCAB + token."""
    rng = np.random.default_rng(seed)
    docs, tfs, counts, fns, tokens = [], [], [], [], []
    for f in range(num_fields):
        lens = rng.integers(1, 40, N_DOCS)
        lens[:N_TIED] = 10
        fns.append(np.array([o.fieldnorm_id(int(v)) for v in range(41)], np.uint8)[lens])
        tokens.append(int(lens.sum()))
        sizes = {T_BIG: 5000, T_MID: 1500, T_400: 400, T_100: 100, T_256: 256, T_512: 512, T_NONE: 0}
        for t in range(VOCAB):
            if t == T_TIED:
                d = np.arange(N_TIED)
                tf = np.ones(N_TIED, np.uint32)
            else:
                n = sizes.get(t, int(rng.integers(300, 3000)))
                d = np.sort(rng.choice(N_DOCS, n, replace=False))
                tf = rng.integers(1, 6, n).astype(np.uint32)
            docs.append(d.astype(np.uint32))
            tfs.append(tf)
            counts.append(len(d))
    post_off = np.zeros(VOCAB * num_fields + 1, np.int64)
    np.cumsum(counts, out=post_off[1:])
    term_field = np.repeat(np.arange(num_fields, dtype=np.uint8), VOCAB)
    return post_off, np.concatenate(docs), np.concatenate(tfs), np.stack(fns), term_field, np.asarray(tokens, np.uint64)


class Corpus:
    def __init__(self, seed, num_fields=1):
        self.post_off, self.doc, self.tf, self.fn, self.term_field, self.tokens = make_corpus(seed, num_fields)
        self.num_fields = num_fields
        self.df = np.diff(self.post_off)
        self.ps = capi.Postings(self.post_off, self.doc, self.tf, self.fn if num_fields > 1 else self.fn[0],
                                term_field=self.term_field if num_fields > 1 else None)
        self.total = self.tokens if num_fields > 1 else int(self.tokens[0])
        self._ref = {}

    def dfs(self, queries):
        return [[int(self.df[t]) for t in q] for q in queries]

    def oracle(self, q, k, alive=None, groups=None, operator_or=True, tag=None):
        """Computed once per (query, k, variant) and shared."""
        key = (tuple(q), k, tag, None if groups is None else tuple(groups), operator_or)
        if key not in self._ref:
            self._ref[key] = o.bm25_search_ex(self.post_off, self.doc, self.tf, self.fn, q, [int(self.df[t]) for t in q], N_DOCS, self.tokens,
                                              k, alive=alive, term_field=self.term_field if self.num_fields > 1 else None, qgroups=groups,
                                              operator_or=operator_or)
        return self._ref[key]


@pytest.fixture(scope="module")
def corpus():
    return Corpus(2024)


# more than k / between 256 and k / fewer than 256 / no match, all in one batch: the queries finish in different rounds
MIXED = [[T_BIG], [T_MID], [T_400], [T_100], [T_256], [T_512], [T_NONE], [T_TIED], [T_BIG, T_MID], [8, 9, 10, 11, 12, 13], []]  # -> bm25r_kernel
LEAN = [[T_BIG], [T_MID], [T_100], [T_256], [T_512], [T_NONE], [T_TIED], [T_400, 8, 9], [14, 15, 16, 17]]                    # -> bm25l_kernel


def same_hits(got, exp, what):
    (gr, gs), (er, es) = got, exp
    assert gr.tolist() == er.tolist(), what
    assert (gs.view(np.uint32) == es.view(np.uint32)).all(), what


def device_batch(c, queries, k, alive=None, groups=None, operator_or=True):
    """The device entry: int64 ids (-1 = no hit) and scores [nq, k]; `alive` goes up as a device bitmap of len(alive) bits."""
    import torch

    oi = torch.empty((len(queries), k), device="cuda", dtype=torch.int64)
    od = torch.empty((len(queries), k), device="cuda", dtype=torch.float32)
    kw = {}
    if alive is not None:
        bits = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).cuda()
        kw = {"d_alive": bits.data_ptr(), "nbits": len(alive)}
    c.ps.bm25_search_batch_device(queries, c.dfs(queries), N_DOCS, c.total, k, oi.data_ptr(), od.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream, groups=groups, operator_or=operator_or, **kw)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy()


def check_all_entries(c, queries, k, alive=None, oracle_alive=None, tag=None, groups=None, operator_or=True):
    """batch entry == device entry == single-query entry == oracle for every query: ids exactly, scores by their bits, -1 tails on
    the device side.  `alive`: the per-call bitmap as passed; `oracle_alive`: what the oracle filters by (the per-call bitmap padded to
    the corpus, ANDed with a resident one).  The single-query entry is msvs_bm25_search: one text column, operator_or, every term its
    own token -- it runs wherever the case can be put to it.  Returns the batch results."""
    if oracle_alive is None and alive is not None:
        oracle_alive = np.zeros(N_DOCS, bool)
        oracle_alive[:len(alive)] = alive
    got = c.ps.bm25_search_batch(queries, c.dfs(queries), N_DOCS, c.total, k, alive=alive, groups=groups, operator_or=operator_or)
    di, dd = device_batch(c, queries, k, alive=alive, groups=groups, operator_or=operator_or)
    for qi, (q, hit) in enumerate(zip(queries, got)):
        what = (k, tag, operator_or, q)
        er, es = c.oracle(q, k, alive=oracle_alive, groups=None if groups is None else groups[qi], operator_or=operator_or, tag=tag)
        same_hits(hit, (er, es), what)
        n = len(er)
        assert di[qi, :n].tolist() == er.astype(np.int64).tolist() and (di[qi, n:] == -1).all(), what
        assert (dd[qi, :n].view(np.uint32) == es.view(np.uint32)).all(), what
        if operator_or and groups is None and c.num_fields == 1 and len(q):
            same_hits(c.ps.bm25_search(q, c.dfs([q])[0], N_DOCS, c.total, k, alive=alive), (er, es), what)
    return got


@gpu
@pytest.mark.parametrize("k", [257, 300, 512, 1000, 4096])
def test_bm25_batch_single_device_and_oracle_agree(k, corpus):
    c = corpus
    for queries in (MIXED, LEAN):
        got = check_all_entries(c, queries, k)
        lens = [len(g[0]) for g in got]
        assert max(lens) == k and 0 in lens and any(0 < n < 256 for n in lens)
        if queries is MIXED and k >= 512:
            assert any(256 < n < k for n in lens)


@gpu
def test_bm25_window_edges_exactly_256_and_512_matches(corpus):
    """The round after the last full round returns nothing, repeats nothing and drops nothing."""
    c = corpus
    for k in (300, 512, 513, 1000):
        got = check_all_entries(c, [[T_256], [T_512]], k)
        for (gr, _), n in zip(got, (256, 512)):
            assert len(gr) == min(n, k) and len(set(gr.tolist())) == len(gr)


@gpu
def test_bm25_ties_across_the_window_edge(corpus):
    c = corpus
    er, es = c.oracle([T_TIED], 300)
    assert len(er) == 300 and len(set(es[250:263].view(np.uint32).tolist())) == 1  # or the case tests nothing
    for queries in ([[T_TIED]], [[T_TIED], [8, 9, 10, 11, 12]]):  # bm25l_kernel, bm25r_kernel
        gr, gs = check_all_entries(c, queries, 300)[0]
        assert (np.diff(gr[250:263].astype(np.int64)) > 0).all() and int(gr[256]) == int(er[256])
    check_all_entries(c, [[T_TIED]], 1000)


@gpu
def test_bm25_alive_bitmaps(corpus):
    """A per-call bitmap of about half the documents, shorter than the corpus; the resident one ANDed with it."""
    c = corpus
    rng = np.random.default_rng(5)
    alive = rng.random(N_DOCS - 1237) < 0.5
    full = np.zeros(N_DOCS, bool)
    full[:len(alive)] = alive
    k = 600
    for queries in (MIXED, LEAN):
        got = check_all_entries(c, queries, k, alive=alive, tag="half")
        assert max(len(g[0]) for g in got) == k
    part = rng.random(N_DOCS) < 0.8
    c.ps.set_alive(part)
    try:
        for al, eff, tag in ((None, part, "part"), (alive, full & part, "both")):
            for queries in (MIXED, LEAN):
                check_all_entries(c, queries, k, alive=al, oracle_alive=eff, tag=tag)
    finally:
        c.ps.set_alive(None)


@gpu
def test_bm25_operator_and(corpus):
    """(The single-query entry has no AND form: batch and device entries.)"""
    c = corpus
    queries = [[T_BIG, T_MID], [T_BIG, 8], [T_BIG, 9, 10], [T_TIED, T_BIG], [T_BIG], [8, 9, 10, 11, 12]]
    alive = np.random.default_rng(6).random(N_DOCS - 300) < 0.7
    for k in (300, 1000):
        got = check_all_entries(c, queries, k, operator_or=False)
        assert max(len(g[0]) for g in got) > 256
        check_all_entries(c, queries, k, operator_or=False, alive=alive, tag="and-alive")


@gpu
def test_bm25_three_text_columns_with_groups():
    """(The single-query entry takes one text column: batch and device entries.)"""
    c = Corpus(2025, num_fields=3)
    queries, groups = [], []
    for toks in ([T_BIG], [T_MID, T_400], [T_100], [T_NONE], [T_TIED, 9], [8, 9, 10]):
        queries.append([int(f * VOCAB + t) for t in toks for f in range(3)])
        groups.append([g for g in range(len(toks)) for _ in range(3)])
    alive = np.random.default_rng(7).random(N_DOCS - 77) < 0.5
    for op_or in (True, False):
        for k in (300, 4096):
            got = check_all_entries(c, queries, k, groups=groups, operator_or=op_or)
            assert max(len(g[0]) for g in got) > 256
        check_all_entries(c, queries, 300, groups=groups, operator_or=op_or, alive=alive, tag="cols-alive")


@gpu
def test_bm25_k_beyond_the_rounds_limit_is_refused(corpus):
    c = corpus
    for call in (lambda: c.ps.bm25_search_batch([[T_BIG]], c.dfs([[T_BIG]]), N_DOCS, c.total, 4097),
                 lambda: c.ps.bm25_search([T_BIG], c.dfs([[T_BIG]])[0], N_DOCS, c.total, 4097),
                 lambda: device_batch(c, [[T_BIG]], 4097)):
        with pytest.raises(capi.MsvsError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED_K


@gpu
def test_bm25_first_256_of_300_are_the_256_result(corpus):
    c = corpus
    for queries in (MIXED, LEAN):
        a = c.ps.bm25_search_batch(queries, c.dfs(queries), N_DOCS, c.total, 256)
        b = c.ps.bm25_search_batch(queries, c.dfs(queries), N_DOCS, c.total, 300)
        di_a, dd_a = device_batch(c, queries, 256)
        di_b, dd_b = device_batch(c, queries, 300)
        assert (di_a == di_b[:, :256]).all() and (dd_a.view(np.uint32) == dd_b[:, :256].view(np.uint32)).all()
        for q, (ar, as_), (br, bs) in zip(queries, a, b):
            assert ar.tolist() == br[:256].tolist() and (as_.view(np.uint32) == bs[:256].view(np.uint32)).all()
            if len(q):
                sa, sb = (c.ps.bm25_search(q, c.dfs([q])[0], N_DOCS, c.total, kk) for kk in (256, 300))
                assert sa[0].tolist() == sb[0][:256].tolist() and (sa[1].view(np.uint32) == sb[1][:256].view(np.uint32)).all()


@gpu
@pytest.mark.parametrize("knob", ["bm25_posting"])
def test_bm25_other_scorers_keep_the_old_limit(knob, corpus, opt):
    """The rounds run on the record scorers only: the knob that selects the dense accumulator answers k > 256 as before, and says
    which."""
    c = corpus
    opt(knob, "0")
    with pytest.raises(capi.MsvsError) as e:
        c.ps.bm25_search_batch([[T_BIG]], c.dfs([[T_BIG]]), N_DOCS, c.total, 300)
    assert e.value.code == capi.ERR_UNSUPPORTED_K and knob in str(e.value)
    same_hits(c.ps.bm25_search_batch([[T_BIG]], c.dfs([[T_BIG]]), N_DOCS, c.total, 256)[0], c.oracle([T_BIG], 256), knob)


@pytest.mark.parametrize("name", ["bm25_wave", "bm25_rec", "bm25_select2", "bm25_bounds8", "bm25_tables_ride", "bm25_fine_sample"])
def test_bm25_retired_options_are_unknown(name):
    """The knobs of the scorers, selection and bounds kernels that are gone: setting one is an error, not a silent no-op."""
    with pytest.raises(capi.MsvsError) as e:
        capi.set_option(name, "0")
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and name in str(e.value)


# ---------------------------------------------------------------------------------------- fusion

def fusion_lists(rng, nq, kv, kt, constant=False):
    vi, ti = np.full((nq, kv), -1, np.int64), np.full((nq, kt), -1, np.int64)
    vd, td = np.zeros((nq, kv), np.float32), np.zeros((nq, kt), np.float32)
    for q in range(nq):
        nv = kv if q == 0 else int(rng.integers(kv // 2, kv + 1))  # -1-padded tails from the second query on
        nt = kt if q == 0 else int(rng.integers(kt // 2, kt + 1))
        pool = rng.permutation(3 * (kv + kt))
        v = pool[:nv]
        shared = rng.random(nt) < 0.5                                # about half of the text labels are vector labels too
        pick = rng.permutation(nv)
        t = np.array([v[pick[j]] if (shared[j] and j < nv) else pool[kv + kt + j] for j in range(nt)], np.int64)
        vi[q, :nv], ti[q, :nt] = v, t
        vd[q, :nv] = np.float32(0.75) if constant else np.sort(rng.random(nv).astype(np.float32))
        td[q, :nt] = np.float32(3.25) if constant else -np.sort(-rng.random(nt).astype(np.float32) * 20)
    return vd, vi, td, ti


def check_fusion(fusion, vd, vi, td, ti, topk, direction, weight, fk):
    import torch

    nq, kv, kt = vi.shape[0], vi.shape[1], ti.shape[1]
    es, el, ec = mhost.hybrid_search_batch(fusion, vd, vi, td, ti, topk, fusion_k=fk, fusion_weight=weight, vector_scan_direction=direction)
    g = lambda a: torch.from_numpy(a).cuda()
    dvd, dvi, dtd, dti = g(vd), g(vi), g(td), g(ti)
    os_ = torch.empty((nq, topk), device="cuda", dtype=torch.float32)
    ol = torch.empty((nq, topk), device="cuda", dtype=torch.int64)
    on = torch.empty((nq,), device="cuda", dtype=torch.int32)
    capi.hybrid_fuse_device(fusion, dvd.data_ptr(), dvi.data_ptr(), kv, dtd.data_ptr(), dti.data_ptr(), kt, nq, topk, os_.data_ptr(),
                            ol.data_ptr(), on.data_ptr(), torch.cuda.current_stream().cuda_stream, fusion_k=fk, fusion_weight=weight,
                            vector_scan_direction=direction)
    torch.cuda.synchronize()
    hs, hl, hn = os_.cpu().numpy(), ol.cpu().numpy(), on.cpu().numpy()
    for q in range(nq):
        n = int(ec[q])
        what = (fusion, kv, kt, topk, direction, q)
        assert int(hn[q]) == n, what
        assert hl[q, :n].tolist() == [int(x) for x in el[q, :n]], what
        assert (hs[q, :n].view(np.uint32) == es[q, :n].view(np.uint32)).all(), what
        assert (hl[q, n:] == -1).all(), what


@gpu
@pytest.mark.parametrize("kv,kt", [(257, 100), (300, 300), (4096, 4096), (1000, 17)])
@pytest.mark.parametrize("fusion", ["rrf", "rsf"])
def test_device_fusion_of_long_lists_equals_the_host_fusion(fusion, kv, kt):
    rng = np.random.default_rng(kv * 7 + kt + (fusion == "rsf"))
    vd, vi, td, ti = fusion_lists(rng, 3, kv, kt)
    for direction, weight, fk in ((1, 0.5, 60), (-1, 0.3, 7)):
        for topk in (10, 300, 4096):
            check_fusion(fusion, vd, vi, td, ti, topk, direction, weight, fk)


@gpu
@pytest.mark.parametrize("fusion", ["rrf", "rsf"])
def test_device_fusion_of_long_constant_score_lists(fusion):
    """Both lists constant: RSF normalises every entry to 1 (the mn == mx branch)."""
    vd, vi, td, ti = fusion_lists(np.random.default_rng(3), 3, 700, 300, constant=True)
    for direction in (1, -1):
        check_fusion(fusion, vd, vi, td, ti, 300, direction, 0.4, 60)


@gpu
def test_device_fusion_beyond_the_limit_is_refused():
    import torch

    z = torch.zeros(8, device="cuda", dtype=torch.int64)
    with pytest.raises(capi.MsvsError) as e:
        capi.hybrid_fuse_device("rrf", z.data_ptr(), z.data_ptr(), 4097, z.data_ptr(), z.data_ptr(), 1, 1, 1, z.data_ptr(), z.data_ptr(),
                                z.data_ptr())
    assert e.value.code == capi.ERR_UNSUPPORTED_K


# ---------------------------------------------------------------------------------------- vector device entries

OM = {capi.METRIC_L2: o.METRIC_L2, capi.METRIC_IP: o.METRIC_IP}


def device_search(ix, q, k, nprobe, alive=None, flt=None):
    import torch

    dq = torch.from_numpy(q).cuda()
    oi = torch.empty((len(q), k), device="cuda", dtype=torch.int64)
    od = torch.empty((len(q), k), device="cuda", dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    if flt is not None:
        ix.search_filter_device(dq.data_ptr(), len(q), k, nprobe, flt, oi.data_ptr(), od.data_ptr(), stream)
    elif alive is not None:
        bits = torch.from_numpy(capi.pack_bits(alive).view(np.int64)).cuda()
        ix.search_device(dq.data_ptr(), len(q), k, nprobe, oi.data_ptr(), od.data_ptr(), stream, d_alive=bits.data_ptr(), nbits=len(alive))
    else:
        ix.search_device(dq.data_ptr(), len(q), k, nprobe, oi.data_ptr(), od.data_ptr(), stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy()


def same(a, b):
    assert (a[0] == b[0]).all(), np.argwhere(a[0] != b[0])[:5]
    assert (a[1].view(np.uint32) == b[1].view(np.uint32)).all()


@gpu
@pytest.mark.parametrize("metric", [capi.METRIC_L2, capi.METRIC_IP])
def test_ivf_device_entries_with_large_k(metric):
    rng = np.random.default_rng(11 + metric)
    n, d, nq = 4000, 32, 3
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    ix = capi.Index(capi.INDEX_IVFFLAT, metric, d, "ncentroids=8,kmeans_iters=4")
    ix.train(x)
    ix.add(x)
    ix.build()
    cent, off, vecs, lids = ix.export()
    alive = rng.random(n) < 0.5
    deleted = rng.random(n) < 0.9
    for k in (300, 1000):
        ref = o.ivf_search(cent, off, vecs, lids, q, 8, k, OM[metric])[:2]
        same(device_search(ix, q, k, 8), ref)
        same(ix.search(q, k, "nprobe=8"), ref)
        ref_f = o.ivf_search(cent, off, vecs, lids, q, 8, k, OM[metric], alive=alive)[:2]
        same(device_search(ix, q, k, 8, alive=alive), ref_f)
        same(device_search(ix, q, k, 8, flt=capi.Filter.from_bool(alive)), ref_f)
        same(ix.search(q, k, "nprobe=8", alive=alive), ref_f)
        same(ix.search_filter(q, k, "nprobe=8", capi.Filter.from_bool(alive)), ref_f)
    ix.set_delete_bitmap(deleted)
    ref_d = o.ivf_search(cent, off, vecs, lids, q, 8, 300, OM[metric], alive=deleted)[:2]
    same(device_search(ix, q, 300, 8), ref_d)
    same(ix.search(q, 300, "nprobe=8"), ref_d)
    same(device_search(ix, q, 300, 8, flt=capi.Filter.from_bool(alive)),
         o.ivf_search(cent, off, vecs, lids, q, 8, 300, OM[metric], alive=alive & deleted)[:2])
    for call in (lambda: device_search(ix, q, 4097, 8), lambda: device_search(ix, q, 4097, 8, flt=capi.Filter.from_bool(alive)),
                 lambda: ix.search_filter(q, 4097, "nprobe=8", capi.Filter.from_bool(alive))):
        with pytest.raises(capi.MsvsError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED_K


@gpu
def test_flat_device_entry_with_large_k():
    rng = np.random.default_rng(13)
    n, d = 3000, 24
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((2, d), dtype=np.float32)
    ix = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, d, "")
    ix.add(x)
    ix.build()
    alive = rng.random(n) < 0.3  # 900 rows: k = 1000 comes back short
    for k in (300, 1000):
        same(device_search(ix, q, k, 1), o.knn(q, x, k, o.METRIC_L2))
        same(device_search(ix, q, k, 1, flt=capi.Filter.from_bool(alive)), o.knn(q, x, k, o.METRIC_L2, alive=alive))
        same(ix.search_filter(q, k, "", capi.Filter.from_bool(alive)), o.knn(q, x, k, o.METRIC_L2, alive=alive))
