#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X vector-search hot path (BASELINE.json).

Metric   : QPS (+ p50 latency) at recall@10 >= 0.95, 1M x 768-d f32, L2, top-10.
Workload : BASELINE.json configs[1] -- IVFFLAT nlist=1024, nprobe=32, on synthetic data of that shape; the coarse quantiser is
           trained as SURVEY 8d says (k-means, 20 iterations on a 256 k sample, seed 7).
A "step" : one batch of `--batch` queries through the search entry point (coarse quantiser + list scan + exact re-rank /
           top-k merge), queries / index / outputs resident in HBM, enqueued on torch's current stream.
N = 1    : msvs_index_search_device.
N > 1    : one process per GPU, libmsvs owns the RCCL communicator, lists sharded list_id % N over the SAME 1M-row index.  `value`
           switches to the ROUTED form (msvs_shard_search_routed_device_async, two steps in flight): every rank brings its OWN batch
           of `--batch` queries per step, so `value` = N x batch queries per step / max-over-ranks time and "scaling" = "weak" -- weak
           in QUERIES over a FIXED index (a reader of SCALE: the ratio value(N) / value(1) is the gain in served queries per second
           when N servers share one index, not a larger table).  The replicated form (msvs_shard_search_device: every rank works
           through the same batch; strong scaling of one batch) is timed beside it under legs.multi_gpu.replicated.
           `python bench.py --gpus N` without a launcher spawns its N ranks itself (torch.distributed.run on 127.0.0.1).
           The collective C4 leg that follows the headline at N > 1 (12.5M x 1536 rows per rank) is guarded: the ranks agree on their
           builds before the first collective search, and if the leg has not returned after --leg-timeout seconds (a rank lost) the
           measured headline line is printed without it.

Data: there is no network, so vectors are synthetic.  The headline (`value`) runs on SURVEY 8d's clustered model -- 1024 gaussian
blobs, sigma 0.3, in R^768 (`blobs03`) -- at the configuration's nprobe = 32 (recall@10 measured against the exact scan of the
same rows; the smallest nprobe that reaches recall 0.95 on it is timed beside it: `operating_points`).  SURVEY 8d's other model,
rows and queries iid N(0,1)^768 (`iid`: no IVF index reaches recall 0.95 on it, the operating point is an exhaustive scan), and
the low-intrinsic-dimension mixture the first three rounds quoted (`latent32`: 1024 blobs in a 32-d latent space embedded in
R^768) are separate legs.  `--data` picks the headline's model.

A plain run (`--gpus 1 --steps K --warmup W`) sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`,
`config`; `recall_at_10`, `roofline` and `cpu_baseline` are null): its time outside the steps is the set-up alone.  Everything
else below -- the recall check, the roofline pass, the 3-stream side measurement, the CPU baseline, every leg and, at N > 1, the
replicated form beside the routed one and the sharded C4 family -- runs under --full.  --dump-outputs DIR writes what the last
timed step returned (DIR/ids.npy as float64, DIR/distances.npy as float32; rank 0's batch at N > 1) before anything else runs
on the device; every input is seeded, so two builds of the project can be compared output for output.

Prints ONE JSON line on rank 0 (driver contract): a compact digest (< 6 KB, `compact_line`: the contract's keys, `roofline` and
`cpu_baseline` without prose, one or two numbers per leg under `legs`).  The FULL object described below goes to bench_detail.json
(beside bench.py and under gpurun_out/) and to stderr:
  roofline      -- the dominant kernel (the list scan: h16_sample_kernel + h16_scan_kernel, two launches per step).  `frac` prices
                   the bytes the launches HAVE TO READ (the fp16 shadow + norms of the union of the probed rows); the f32-equivalent
                   rate of SURVEY 8d's formula is a side field (it credits bytes that never move); `whole_step_frac` = the same
                   bytes over the whole step.
  cpu_baseline  -- the SIMD CPU restatement (oracle/simd_baseline.c, built -march=native on this machine) on a bounded sample,
                   plus a bit-for-bit check of >= 256 bench queries against the parity oracle.
  other_batches -- the same index at 1 / 16 / 64 / 256 / 1024 queries per step.
  latency       -- SURVEY 8d's protocol through the host-pointer C-ABI (query in, ids + distances out): p50 / p99 of
                   single-query calls, QPS at 1 / 8 / 64 / 128 concurrent host threads (native threads, one query per call: the
                   reference's calling pattern), small batches of 4 .. 256 host queries per call, the 4096-query host-pointer call.
  iid, blobs03  -- SURVEY 8d's data models at their recall >= 0.95 operating points.
  target_100m   -- one GPU's share of the configuration north_star states its targets on (100M x 768 L2 top-10 over 8 GPUs):
                   12.5M x 768 rows, 2048 local lists, 8 local probes; QPS at 64 / 1024 / 4096 queries per batch, recall@10 against
                   the exact scan, moved-bytes roofline fraction from HIP events, a 64-query oracle check on rows re-gathered from
                   the SOURCE table, and the SIMD CPU baseline on the same lists.
  other_configs -- BASELINE configs C1 (FLAT 10k x 128), C3 (10M x 768 cosine, batches of 64), C4 (one GPU's share of
                   100M x 1536 inner product: 12.5M rows, 2048 of the 16384 lists, 8 of the 64 probes), C5 (hybrid: vector top-100
                   + BM25 top-100 over 10M documents + RRF), each with its own bytes/s figure and an oracle check; C1 and C3 carry
                   their own cpu_baseline.
Every hbm fraction in the line prices the bytes the launches MOVE (fp16 shadow row + norm + id for the shadow pass, f32 rows for
the canonical paths); MFMA-bound passes (exhaustive batches) are priced against the dense fp16 matrix peak.
Under --full, every leg but the headline is skipped by --headline-only (profiler runs); --only LEG[,LEG] runs the named legs only;
N > 1 runs the headline and the sharded C4 family (12.5M rows, 2048 lists, 8 probes PER RANK: at N = 8 that is BASELINE configs[3]).
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import myscaledb_amd.capi as capi  # noqa: E402  (raises if libmsvs.so is missing: no fallback)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_F16_PEAK_TF = 2500.0  # dense fp16 matrix peak (MI355X_MICROARCH.md; the 5 PF headline figure is 2:1 sparse)

LATENT_DIM = 32
N_BLOBS = 1024
MID_BLOBS = 64  # the `mid` model: fewer blobs than lists


def _latent_model(d, seed, device, blobs=N_BLOBS):
    """Synthetic embedding model: a 1024-component gaussian mixture in a 32-d latent space (blob centres ~ 3 N(0,I),
    unit within-blob spread), embedded into R^d by a fixed random linear map, plus small isotropic noise.  Low
    intrinsic dimension + cluster structure is what real embedding sets look like to an IVF index; iid N(0,I) in 768-d
    has no neighbourhood structure at all (all points equidistant) and no index can reach recall 0.95 on it."""
    g = torch.Generator(device=device).manual_seed(seed)
    centres = 3.0 * torch.randn((blobs, LATENT_DIM), generator=g, device=device, dtype=torch.float32)
    proj = torch.randn((LATENT_DIM, d), generator=g, device=device, dtype=torch.float32) / (LATENT_DIM ** 0.5)
    return centres, proj


def _sample(model, n, g, device, chunk=65536, out=None):
    centres, proj = model
    d = proj.shape[1]
    x = out if out is not None else torch.empty((n, d), device=device, dtype=torch.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        z = torch.randint(0, centres.shape[0], (hi - lo,), generator=g, device=device)
        lat = centres[z] + torch.randn((hi - lo, LATENT_DIM), generator=g, device=device, dtype=torch.float32)
        x[lo:hi] = lat @ proj + 0.05 * torch.randn((hi - lo, d), generator=g, device=device, dtype=torch.float32)
    return x


def _sample_of_blobs(model, n, g, device, first, stride, out, chunk=65536):
    """Rows of the blobs first, first + stride, first + 2 stride, ... only (one rank's share of a list_id % world sharding
    when the coarse centroids are the blob centres)."""
    centres, proj = model
    d = proj.shape[1]
    mine = (centres.shape[0] - first + stride - 1) // stride
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        z = first + stride * torch.randint(0, mine, (hi - lo,), generator=g, device=device)
        lat = centres[z] + torch.randn((hi - lo, LATENT_DIM), generator=g, device=device, dtype=torch.float32)
        out[lo:hi] = lat @ proj + 0.05 * torch.randn((hi - lo, d), generator=g, device=device, dtype=torch.float32)
    return out


def make_data(n, d, seed, device, blobs=N_BLOBS):
    model = _latent_model(d, 99, device, blobs)
    g = torch.Generator(device=device).manual_seed(seed)
    return model, _sample(model, n, g, device)


def make_queries(model, nq, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    return _sample(model, nq, g, device).contiguous()


def blob_centres(d, device, blobs=N_BLOBS, seed=99):
    """SURVEY 8d's clustered model: blob centres ~ N(0,1)^d (seed 99)."""
    return torch.randn((blobs, d), generator=torch.Generator(device=device).manual_seed(seed), device=device, dtype=torch.float32)


def blob_sample(centres, n, g, device, sigma=0.3, out=None, chunk=131072):
    """n rows: a uniformly drawn centre + sigma N(0,1)^d."""
    x = out if out is not None else torch.empty((n, centres.shape[1]), device=device, dtype=torch.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        z = torch.randint(0, centres.shape[0], (hi - lo,), generator=g, device=device)
        x[lo:hi] = centres[z] + sigma * torch.randn((hi - lo, centres.shape[1]), generator=g, device=device, dtype=torch.float32)
    return x


def data_model(kind, n, nq, d, device):
    """(rows [n, d], queries [nq, d], description) of one of the three synthetic models; rows seed 1234, queries seed 4321."""
    g = torch.Generator(device=device).manual_seed(1234)
    gq = torch.Generator(device=device).manual_seed(4321)
    if kind == "iid":
        return (torch.randn((n, d), generator=g, device=device, dtype=torch.float32),
                torch.randn((nq, d), generator=gq, device=device, dtype=torch.float32),
                "rows and queries iid N(0,1)^%d, seeds 1234 / 4321 (torch generators on the GPU) -- SURVEY 8d" % d)
    if kind == "blobs03":
        c = blob_centres(d, device)
        return (blob_sample(c, n, g, device), blob_sample(c, nq, gq, device),
                "1024 gaussian blobs (centres N(0,1)^%d, seed 99), sigma 0.3, rows seed 1234, queries seed 4321 -- SURVEY 8d's clustered variant" % d)
    if kind == "latent32":
        model = _latent_model(d, 99, device)
        return (_sample(model, n, g, device), _sample(model, nq, gq, device).contiguous(),
                "1024-blob gaussian mixture in a 32-d latent space embedded in R^%d + 0.05 noise, seeds 99 / 1234 / 4321 (the model "
                "rounds 1-3 quoted; not one of SURVEY 8d's)" % d)
    if kind == "mid":
        model = _latent_model(d, 99, device, blobs=MID_BLOBS)
        return (_sample(model, n, g, device), _sample(model, nq, gq, device).contiguous(),
                "%d-blob gaussian mixture in a 32-d latent space (centres 3 N(0,I), unit spread) embedded in R^%d + 0.05 noise, seeds 99 / 1234 / "
                "4321: 16 lists per blob -- a query's neighbours lie in several lists of its blob (recall@10 0.29 / 0.69 / 0.90 / 0.999 at nprobe "
                "1 / 4 / 8 / 16), the other blobs' lists can be pruned: the regime between SURVEY 8d's two models" % (MID_BLOBS, d))
    raise SystemExit("unknown data model %r" % kind)


def build_postings(n_docs, vocab):
    """SURVEY 8d C5 corpus on the GPU (torch is plumbing here): Zipf(1.1) vocabulary, document length ~ Poisson(30),
    seed 5 -> (capi.Postings, df per term, total tokens, number of postings)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(5)
    p = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** 1.1
    lens_t = torch.clamp(torch.poisson(torch.full((n_docs,), 30.0, device=dev), generator=g), min=1).to(torch.int64)
    total = int(lens_t.sum().item())
    toks = torch.multinomial((p / p.sum()).to(torch.float32), total, replacement=True, generator=g)
    doc_of = torch.repeat_interleave(torch.arange(n_docs, device=dev, dtype=torch.int64), lens_t)
    key, _ = torch.sort(toks * n_docs + doc_of)
    uk_t, tf_t = torch.unique_consecutive(key, return_counts=True)
    uk, tf = uk_t.cpu().numpy(), tf_t.cpu().numpy()
    lens = lens_t.cpu().numpy()
    del toks, doc_of, key, uk_t, tf_t
    term, doc = uk // n_docs, (uk % n_docs).astype(np.uint32)
    post_off = np.zeros(vocab + 1, np.int64)
    np.cumsum(np.bincount(term, minlength=vocab), out=post_off[1:])
    table = [b if b < 24 else 24 + (((b - 24) & 7) if ((b - 24) >> 3) == 0 else (((b - 24) & 7) | 8) << (((b - 24) >> 3) - 1))
             for b in range(256)]
    fn_ids = (np.searchsorted(np.array(table, np.int64), lens, side="right") - 1).astype(np.uint8)
    ps = capi.Postings(post_off, doc, tf.astype(np.uint32), fn_ids)
    return ps, np.diff(post_off), total, len(doc)


def ivf_params(nlist, n_train, extra=""):
    """k-means 20 iterations on a 256 k sample, seed 7 (the sample never exceeds the rows it is drawn from)."""
    return "ncentroids=%d,kmeans_iters=20,train_sample=%d,seed=7%s" % (nlist, min(n_train, 262144), extra)


def oracle_on_index_lists(ix, q, nprobe, k, metric, threads=8):
    """The parity oracle on what the queries touch, for an index too large to export whole: probes from the oracle's exact scan
    of the exported centroids, then the oracle's exact scan of the rows of the probed lists, exported list by list from the
    index's own storage (msvs_index_export_list); bulk: rows_by_id is called ONCE with every id (a source that is regenerated
    rather than resident).  Test infrastructure: only the check legs of this script and tests/ call it."""
    from oracle import oracle as o
    om = {capi.METRIC_L2: o.METRIC_L2, capi.METRIC_IP: o.METRIC_IP, capi.METRIC_COSINE: o.METRIC_IP}[metric]
    cent, off, _, _ = ix.export(with_vecs=False)
    qn = o.normalize_rows(q) if metric == capi.METRIC_COSINE else q
    probes, _ = o.knn(qn, cent, nprobe, om)
    cache = {}
    out_i, out_d = [], []
    for qi in range(q.shape[0]):
        vs, ls = [], []
        for l in probes[qi]:
            if l < 0 or off[l + 1] == off[l]:
                continue
            if int(l) not in cache:
                if len(cache) > 256:
                    cache.clear()
                cache[int(l)] = ix.export_list(int(l), int(off[l + 1] - off[l]))
            vs.append(cache[int(l)][0])
            ls.append(cache[int(l)][1])
        sub, rows = np.concatenate(vs), np.concatenate(ls)
        i1, d1 = o.knn(qn[qi:qi + 1], sub, k, om, labels=rows)
        out_i.append(i1[0])
        out_d.append((np.float32(1) - d1[0]).astype(np.float32) if metric == capi.METRIC_COSINE else d1[0])
    return np.stack(out_i), np.stack(out_d)


def probed_sub_index(ix, q, nprobe, metric, rows_by_id=None, bulk=False):
    """What a query sample touches of an index too large to export whole, as the arrays the parity oracle and the SIMD baseline
    take: the centroid table complete, the probed lists' rows, every other list empty -- so a search of the sub-index with
    the same nprobe IS the search of the whole index for these queries.  The probes come from the oracle's exact scan of the
    exported centroids.  rows_by_id(ids) -> f32 rows re-gathers the rows from the SOURCE table by their ids (a row damaged at
    add time then shows up as a mismatch); None: exported list by list from the index's own storage.
    Test infrastructure: only the check / cpu_baseline legs of this script and tests/ call it."""
    from oracle import oracle as o
    om = {capi.METRIC_L2: o.METRIC_L2, capi.METRIC_IP: o.METRIC_IP, capi.METRIC_COSINE: o.METRIC_IP}[metric]
    cent, off, _, lids = ix.export(with_vecs=False)
    qn = o.normalize_rows(q) if metric == capi.METRIC_COSINE else q
    probes, _ = o.knn(qn, cent, nprobe, om)
    used = sorted(set(int(l) for l in probes.ravel() if l >= 0 and off[l + 1] > off[l]))
    lens = np.zeros(len(off) - 1, np.int64)
    lens[used] = [off[l + 1] - off[l] for l in used]
    sub_off = np.zeros(len(off), np.int64)
    np.cumsum(lens, out=sub_off[1:])
    vecs = np.empty((int(sub_off[-1]), ix.dim), np.float32)
    ids = np.empty(int(sub_off[-1]), np.int64)
    for l in used:
        lo, hi = int(sub_off[l]), int(sub_off[l + 1])
        ids[lo:hi] = lids[off[l]:off[l + 1]]
        if rows_by_id is None:
            vecs[lo:hi] = ix.export_list(l, hi - lo)[0]
        elif not bulk:
            r = rows_by_id(ids[lo:hi])
            vecs[lo:hi] = o.normalize_rows(r) if metric == capi.METRIC_COSINE else r
    if rows_by_id is not None and bulk:
        r = rows_by_id(ids)  # one call: a source that is regenerated rather than resident
        vecs[:] = o.normalize_rows(r) if metric == capi.METRIC_COSINE else r
    return cent, sub_off, vecs, ids, qn, om


def oracle_on_sub_index(sub, nprobe, k, metric, threads=8):
    """The parity oracle's IVF search over probed_sub_index's arrays -> (ids, distances as the index reports them)."""
    from oracle import oracle as o
    cent, off, vecs, ids, qn, om = sub
    oi, od, _ = o.ivf_search(cent, off, vecs, ids, qn, nprobe, k, om, threads=threads)
    return oi, ((np.float32(1) - od).astype(np.float32) if metric == capi.METRIC_COSINE else od)


def simd_baseline_on_sub_index(sub, nprobe, k, seconds, cores):
    """oracle/simd_baseline.c over the same arrays, the query sample repeated until ~`seconds` of CPU work -> (queries/s, the
    sample description)."""
    from oracle import oracle as o
    cent, off, vecs, ids, qn, om = sub
    o.simd_ivf_search(cent, off, vecs, ids, qn[:cores], nprobe, k, om, cores)  # builds -march=native, warms up
    t1 = time.perf_counter()
    o.simd_ivf_search(cent, off, vecs, ids, qn, nprobe, k, om, cores)
    per_round = max(time.perf_counter() - t1, 1e-4)
    rounds = int(max(1, min(2000, seconds / per_round)))
    t1 = time.perf_counter()
    for _ in range(rounds):
        o.simd_ivf_search(cent, off, vecs, ids, qn, nprobe, k, om, cores)
    el = time.perf_counter() - t1
    return rounds * qn.shape[0] / el, "%d queries x %d rounds, %.1f s" % (qn.shape[0], rounds, el)


def cpu_cores():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:  # a cgroup CPU quota smaller than the visible core count is what the threads really get
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return cores


def timed(fn, steps, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def profiled(fn, steps, families, drain=None):
    """HIP-event time per step of the named kernel families (msvs_profile_*), on the launch stream.  drain: completes steps a
    pipelined entry point still holds (collective)."""
    capi.profile_reset()
    capi.profile_enable(True)
    for i in range(steps):
        fn(i)
    if drain:
        drain()
    torch.cuda.synchronize()
    capi.profile_enable(False)
    out = {}
    for f in families:
        c, ms = capi.profile_get(f)
        out[f] = ms / steps if c else 0.0
    capi.profile_reset()
    return out


def rows_read_per_step(fn, steps):
    """Rows the shadow list scan's two launches READ per step (main launch: the lists with surviving pairs beyond block 0; sample
    launch: block 0 of the lists probed after the pre-pruning), counted on the device by the plan kernels (msvs_debug_scan_rows
    under rerank_stats): with the probe pruning the launches read less than the union of the probed lists, and the roofline
    prices what moves."""
    capi.set_option("rerank_stats", "1")
    try:
        r0 = capi.debug_scan_rows()
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        r1 = capi.debug_scan_rows()
    finally:
        capi.set_option("rerank_stats", None)
    return ((r1[0] - r0[0]) + (r1[1] - r0[1])) / float(steps)


SCAN_FAMILIES = ("ivf_scan", "ivf_sample_scan")
STEP_FAMILIES = ("coarse_pass", "flat_scan", "merge", "ivf_plan", "ivf_prep", "ivf_sample_scan", "ivf_scan", "rerank",
                 "fallback_scan", "fallback_merge", "lat_search")


def recall_at_k(got, gt, k):
    return float(np.mean([len(set(a) & set(b)) / k for a, b in zip(got.tolist(), gt.tolist())]))


DUMP_BYTES = 64 << 20


def dump_outputs(path, ids, dis):
    """--dump-outputs: one step's results (ids as float64, exact for every row id; distances as float32) as path/ids.npy and
    path/distances.npy.  A step larger than DUMP_BYTES is sampled: the same seeded rows every run."""
    ids, dis = ids.cpu().numpy(), dis.cpu().numpy()
    rows = DUMP_BYTES // (ids.shape[1] * (8 + 4))
    if ids.shape[0] > rows:
        keep = np.sort(np.random.default_rng(0).choice(ids.shape[0], rows, replace=False))
        ids, dis = ids[keep], dis[keep]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "ids.npy"), ids.astype(np.float64))
    np.save(os.path.join(path, "distances.npy"), dis.astype(np.float32))


def leg(name, fn, out):
    """Optional legs never cost the bench line: a failure is recorded instead."""
    t = time.time()
    try:
        out[name] = fn()
    except Exception as e:  # noqa: BLE001
        out[name] = {"error": repr(e)[:300]}
    if isinstance(out[name], dict):
        out[name]["leg_s"] = round(time.time() - t, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    # 4096 queries per step: about 1 ms of arrivals at the measured rate -- what a batching front end in front of
    # `ScanThreadLimiter`-many client threads accumulates; smaller steps and single calls are reported next to it
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--streams", type=int, default=1,
                    help="independent batches in flight on one GPU: step i runs on HIP stream i %% streams (N = 1 only)")
    ap.add_argument("--data", default="blobs03", choices=("blobs03", "iid", "latent32", "mid"),
                    help="data model of the headline: SURVEY 8d's clustered variant (default), its iid one, or the 32-d latent mixture")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else this script measures and checks: recall@10, the roofline pass, the "
                         "3-stream side measurement, the CPU baseline, the legs (N > 1: the replicated form, the sharded C4 family)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's results to DIR/ids.npy (float64) and DIR/distances.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-concurrent", action="store_true", help="skip the 3-stream side measurement (kernel traces of the single-stream steps)")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: only the timed steps + the roofline pass (profiler runs)")
    ap.add_argument("--skip", default="", help="comma list of legs to skip: other_batches,latency,iid,blobs03,latent32,mid,target,c1,c3,c4,c5,cpu")
    ap.add_argument("--shard-mode", default="routed", choices=("routed", "replicated"),
                    help="N > 1: every rank brings its own batch and queries are routed to the ranks that own their lists (default), or "
                         "every rank works through the same batch (msvs_shard_search_device)")
    ap.add_argument("--only", default="", help="with --full: comma list of legs to run (the others are skipped; the headline always runs)")
    ap.add_argument("--c4-rows", type=int, default=12_500_000, help="rows per GPU of the C4 leg (100M / 8)")
    ap.add_argument("--big-rows", type=int, default=10_000_000, help="rows of the C3 / C5 legs")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--leg-timeout", type=int, default=480, help="N > 1: seconds the collective c4_sharded leg may take before the headline "
                                                                   "line is printed without it")
    ap.add_argument("--test-single-device", action="store_true",
                    help="N > 1 ranks all on cuda:0 with a gloo transport under msvs_shard_search_device: exercises the N > 1 "
                         "code path of this script on a one-GPU box (not a measurement)")
    args = ap.parse_args()
    if args.only and not args.full:
        ap.error("--only picks legs of --full")
    skip = set(x for x in args.skip.split(",") if x)
    ALL_LEGS = ("other_batches", "latency", "iid", "blobs03", "latent32", "mid", "target", "c1", "c3", "c4", "c5", "cpu")
    if args.only:
        skip |= set(ALL_LEGS) - set(x for x in args.only.split(",") if x)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched without torch.distributed.run: spawn the N ranks ourselves (one process per GPU) and pass the JSON line through
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.test_single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    capi.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    comm = None
    if world > 1:
        import torch.distributed as dist
        from myscaledb_amd import sharded
        if args.test_single_device:
            dist.init_process_group("gloo")
            comm = sharded.gloo_comm()
            comm_kind = "gloo transport on host copies (test)"
        else:
            dist.init_process_group("nccl", device_id=dev)
            try:
                comm = sharded.rccl_comm()  # RCCL communicator owned by libmsvs; torch only carried the unique id
                comm_kind = "RCCL communicator owned by libmsvs (msvs_comm_init)"
            except Exception as e:  # noqa: BLE001 -- keep the N > 1 run alive; every rank takes the same branch or the all-reduce below fails
                sys.stderr.write("rank %d: msvs_comm_init failed (%r): all-gathers through torch.distributed\n" % (rank, e))
                comm = None
            ok = torch.tensor([1 if comm is not None else 0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0:
                comm = sharded.torch_comm()
                comm_kind = "torch.distributed all_gather_into_tensor callback (msvs_comm_init_custom)"

    n, d, nlist, nprobe, k, B = args.rows, args.dim, args.nlist, args.nprobe, args.k, args.batch
    t_setup = time.time()
    n_pool = 8
    x, q_all, data_desc = data_model(args.data, n, n_pool * B, d, dev)

    # ---- build: rank 0 trains the coarse quantiser, everyone adopts the same centroids, keeps its own lists
    params = ivf_params(nlist, n, ",shard_rank=%d,shard_world=%d" % (rank, world))
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, params)
    if world == 1:
        ix.train(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    else:
        cent = torch.empty((nlist, d), device=dev, dtype=torch.float32)
        if rank == 0:
            t = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, params)
            t.train(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
            t.add(x[:nlist].contiguous().data_ptr(), n=nlist, mem=capi.MEM_DEVICE)
            t.build()
            cent.copy_(torch.from_numpy(t.export()[0]))
            t.close()
        if args.test_single_device:
            c_ = cent.cpu()
            dist.broadcast(c_, 0)
            cent.copy_(c_)
        else:
            dist.broadcast(cent, 0)
        ix.set_centroids(cent.cpu().numpy())
    ix.add(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    ix.build()
    torch.cuda.synchronize()
    setup_s = time.time() - t_setup

    stream = torch.cuda.current_stream().cuda_stream
    out_ids = torch.empty((B, k), device=dev, dtype=torch.int64)
    out_dis = torch.empty((B, k), device=dev, dtype=torch.float32)
    # --streams S: S independent batches in flight, each search on its own stream with its own result buffers (a server with S
    # worker streams): the small launches around one batch's list scan run beside the other batch's scan
    n_streams = max(1, args.streams) if world == 1 else 1
    side_streams = 3 if args.full and world == 1 and n_streams == 1 and not args.no_concurrent else 0  # reported beside the headline (`concurrent_batches`), never as `value`
    xs = [torch.cuda.Stream() for _ in range(max(n_streams, side_streams))] if max(n_streams, side_streams) > 1 else []
    xs_out = [(torch.empty((B, k), device=dev, dtype=torch.int64), torch.empty((B, k), device=dev, dtype=torch.float32)) for _ in xs]
    multi = {"on": False, "n": n_streams}

    routed = world > 1 and args.shard_mode == "routed"
    routed_served = []
    routed_live = []
    routed_slots = [(torch.empty((B, k), device=dev, dtype=torch.int64), torch.empty((B, k), device=dev, dtype=torch.float32), ctypes.c_uint64(0))
                    for _ in range(3)] if routed else []

    def step(i):
        if routed:
            # every rank brings its OWN batch (the queries that arrived at its server); a query visits the ranks that own lists it still
            # needs after the pre-pruning at its home rank (msvs_shard_search_routed_device)
            # two steps in flight (msvs_shard_search_routed_device_async): call i enqueues the front phase of batch i and the back phase
            # of batch i - 1, whose count matrix was gathered one call ago; fence() drains (collective) and synchronises
            j = (i * world + rank) % n_pool
            slot = routed_slots[i % 3]  # (batch i - 1 is still in flight and batch i - 2's event has just been handed out)
            ix.shard_search_routed_device_async(comm, q_all[j * B:(j + 1) * B].data_ptr(), B, k, nprobe, slot[0].data_ptr(), slot[1].data_ptr(),
                                                stream, served=slot[2], want_event=False)
            routed_live.append(slot[2])
            return
        q = q_all[(i % n_pool) * B:(i % n_pool + 1) * B]
        if world > 1:
            # the whole sharded search as ONE stream-ordered call (no host synchronisation).  (The two-batches-in-flight form,
            # msvs_shard_search_device_async, hands over between two streams five times per batch: 0.70 against 0.51 ms per step on one
            # rank -- more than the top-k exchange it could hide costs.)
            ix.shard_search_device(comm, q.data_ptr(), B, k, nprobe, out_ids.data_ptr(), out_dis.data_ptr(), stream)
        elif multi["on"]:
            s_ = i % multi["n"]
            ix.search_device(q.data_ptr(), B, k, nprobe, xs_out[s_][0].data_ptr(), xs_out[s_][1].data_ptr(), xs[s_].cuda_stream)
        else:
            ix.search_device(q.data_ptr(), B, k, nprobe, out_ids.data_ptr(), out_dis.data_ptr(), stream)

    def fence():
        if world > 1:
            comm.drain(stream)  # (a pending routed step's back phase runs here: collective)
        torch.cuda.synchronize()
        if routed_live:
            routed_served.extend(c.value for c in routed_live[-3:])  # (the pairs counters of the last steps, complete after the drain)
            routed_live.clear()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    multi["on"] = n_streams > 1
    if routed:
        # the routed entry has only ever run on a 1-GPU box (two ranks sharing it): if its first step fails on any rank, every rank
        # falls back to the replicated form instead of losing the N > 1 line
        ok_r = 1
        try:
            step(0)
            fence()  # (the back phase of the step runs in the drain: a failure on ANY rank's front phase is raised there on EVERY rank)
        except Exception as e:  # noqa: BLE001
            sys.stderr.write("rank %d: routed search failed (%r): replicated form\n" % (rank, e))
            ok_r = 0
        t_ok = torch.tensor([ok_r], device="cpu" if args.test_single_device else dev)
        dist.all_reduce(t_ok, op=dist.ReduceOp.MIN)
        if int(t_ok.item()) == 0:
            routed = False
            routed_served.clear()
    for i in range(args.warmup):
        step(i)
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        last = args.steps - 1  # (the buffers step(last) wrote, complete after the fence)
        res = routed_slots[last % 3][:2] if routed else xs_out[last % n_streams] if n_streams > 1 else (out_ids, out_dis)
        dump_outputs(args.dump_outputs, *res)
    if world > 1:
        t = torch.tensor([elapsed], device="cpu" if args.test_single_device else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    qps = args.steps * B * (world if routed else 1) / elapsed

    def head():
        """The line's headline keys: the rate of the timed steps and what was timed."""
        return {
            "metric": "QPS at recall@10>=0.95, 1Mx768-d L2 top-10 (IVFFLAT nlist=1024 nprobe=%d)" % nprobe,
            "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak" if routed else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "IVFFLAT nlist=%d, %dx%d f32, L2, nprobe=%d, top-%d, batch %d queries/step "
                                   "(BASELINE.json configs[1])" % (nlist, n, d, nprobe, k, B),
                       "rows": n, "dim": d, "nlist": nlist, "nprobe": nprobe, "k": k, "batch": B,
                       "parallelism": (("lists %% %d, ROUTED: a batch of %d queries per rank and step, coarse quantiser + pre-pruning at the home rank, "
                                        "point-to-point exchange of the surviving (query, rank) pairs, local search, results back, merge at home "
                                        "(msvs_shard_search_routed_device_async: two steps in flight); transport: %s" % (world, B, comm_kind)) if routed else
                                       ("lists %% %d, coarse quantiser by query, probe (+ coarse distance word) and packed top-k all-gathers, "
                                        "one stream-ordered call per batch (msvs_shard_search_device); transport: %s"
                                        % (world, comm_kind))) if world > 1 else
                                      ("single GPU" if n_streams == 1 else "single GPU, %d independent batches in flight on %d HIP streams" % (n_streams, n_streams)),
                       "streams": n_streams, "data_model": data_desc},
        }

    if not args.full:
        if rank == 0:
            emit(dict(head(), setup_s=round(setup_s, 1)))
        if world > 1:
            comm.close()
            dist.barrier()
            dist.destroy_process_group()
        return
    multi["on"] = False  # (the profiled passes below run one batch at a time on the current stream)
    concurrent = None
    if side_streams:
        # the same steps with 3 independent batches in flight (a server with 3 worker streams): the small launches around one
        # batch's list scan run beside another batch's scan
        multi.update(on=True, n=side_streams)
        for i in range(2 * side_streams):
            step(i)
        fence()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        fence()
        e1 = time.perf_counter() - t1
        multi.update(on=False, n=n_streams)
        concurrent = {"streams": side_streams, "qps": round(args.steps * B / e1, 1), "ms_per_step": round(e1 / args.steps * 1e3, 4),
                      "note": "%d independent batches in flight on %d HIP streams, same steps; `value` is the single-stream rate" % (side_streams, side_streams)}
    multi_gpu = None
    if world > 1:
        # both forms side by side: the routed one (own batch per rank) and the replicated one (every rank works through the same batch)
        served = torch.tensor([float(np.mean(routed_served[-args.steps:])) if routed_served else 0.0], dtype=torch.float64)
        allv = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        if args.test_single_device:
            dist.all_gather(allv, served)
        else:
            sv = served.to(dev)
            av = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
            dist.all_gather(av, sv)
            allv = [a.cpu() for a in av]
        fam_r = None
        if routed:
            fam_r = profiled(step, min(args.steps, 4), ("shard_exchange", "coarse_pass", "ivf_plan", "ivf_scan", "ivf_sample_scan", "rerank", "merge"),
                             drain=fence)
        routed_now = routed
        routed = False
        for i in range(2):
            step(i)
        fence()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        fence()
        e2 = time.perf_counter() - t1
        routed = routed_now
        t = torch.tensor([e2], device="cpu" if args.test_single_device else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        multi_gpu = {"mode": "routed" if routed_now else "replicated",
                     "routed": {"queries_per_step_per_rank": B, "routed_pairs_per_step_by_rank": [round(float(a.item()), 1) for a in allv],
                                "qps": round(qps, 1) if routed_now else None, "stage_ms_rank0": fam_r,
                                "note": "routed_pairs = (query, rank) pairs a rank served: its share of the list-scan work; W x batch when nothing can be pruned"},
                     "replicated": {"qps": round(args.steps * B / float(t.item()), 1), "ms_per_step": round(float(t.item()) / args.steps * 1e3, 4),
                                    "note": "msvs_shard_search_device: every rank works through the SAME batch (strong scaling of one batch's latency)"}}

    # ---- roofline of the dominant kernel: the list scan = h16_sample_kernel + h16_scan_kernel (HIP events on the launch
    # stream, separate pass over the same steps)
    pf0 = capi.prefilter_stats()
    n_prof = min(args.steps, n_pool)
    fam = profiled(step, n_prof, STEP_FAMILIES)
    pf1 = capi.prefilter_stats()
    cand_pass = pf1[0] > pf0[0]
    scan_ms = fam["ivf_scan"] + fam["ivf_sample_scan"]
    # share of the step's (query, list) pairs the probe pruning proved useless and kept out of the main launch (two counted steps)
    capi.set_option("rerank_stats", "1")
    ps0 = capi.debug_prune_stats()
    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    ps1 = capi.debug_prune_stats()
    capi.set_option("rerank_stats", None)
    pruned_frac = (ps1[0] - ps0[0]) / float(ps1[1] - ps0[1]) if ps1[1] > ps0[1] else 0.0
    sr = [ix.scanned_rows(q_all[(i % n_pool) * B:(i % n_pool + 1) * B].cpu().numpy(), nprobe) for i in range(n_prof)]
    rows_model = sum(r[0] for r in sr) / n_prof   # sum over (query, probed list) of list length (SURVEY 8d per-query model)
    rows_unique = sum(r[2] for r in sr) / n_prof  # rows probed by >= 1 query of the batch: must leave HBM once
    # ALGORITHMIC bytes of one step's list scan (batch form): the union of the probed rows x (4d + 4) B -- the
    # f32 row + its id, whatever the kernel actually reads.  This round's kernel reads an fp16 shadow of the rows
    # (2d B + 4 B norm) and re-ranks a few dozen f32 rows per query, so it moves about HALF the algorithmic bytes:
    # `achieved` can exceed what HBM delivered; moved_gbs / moved_frac price the bytes the launch really has to move.
    rows_read = rows_read_per_step(step, n_prof) if cand_pass and world == 1 else rows_unique  # (N > 1: every rank reads its own share)
    bytes_alg = rows_unique * (4 * d + 4)
    bytes_moved = rows_read * (2 * d + 8) if cand_pass else bytes_alg
    achieved = bytes_alg / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
    moved_gbs = bytes_moved / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
    # (HBM traffic from the PMC counters is NOT measured inside this run: the FETCH_SIZE / WRITE_SIZE passes of the same step are
    # kept under profiles/ -- traffic.json, rNN_pmc_*.txt -- and the line says null rather than quoting another run's number)
    traffic = None
    traffic_src = None
    try:
        # the FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes of THIS step (same data model, batch, nprobe), run under rocprofv3 in their own
        # processes (tools/r6_pmc_traffic.sh) and committed with the tree: quoted only when the run's shape is the one they measured
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            tj = json.load(f)
        leg_ = {"blobs03": "headline", "mid": "mid", "iid": "iid"}.get(args.data)
        if world == 1 and cand_pass and leg_ in tj.get("legs", {}) and (n, d, B, nprobe, nlist) == (1_000_000, 768, 4096, 32, 1024):
            traffic = int(tj["legs"][leg_]["hbm_bytes_per_step"])
            traffic_src = "profiles/traffic.json (%s: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same step)" % tj.get("round")
    except (OSError, ValueError, KeyError):
        pass
    # matrix-core work of the same launches: fp16 MFMA, 2 flop per (query, probed row, element padded to 64)
    mfma_tf = rows_model * 2 * ((d + 63) // 64 * 64) / (scan_ms * 1e-3) / 1e12 if scan_ms > 0 and cand_pass else 0.0
    if world > 1:
        t = torch.tensor([achieved, moved_gbs], device="cpu" if args.test_single_device else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        achieved, moved_gbs = float(t[0].item()), float(t[1].item())
    step_ms = elapsed / args.steps * 1e3
    roof = {
        "bound": "hbm", "achieved": round(moved_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(moved_gbs / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
        "kernel": "h16_scan_kernel + h16_sample_kernel (fp16-shadow MFMA candidate pass of the list scan; exact f32 re-rank + "
                  "certificate follow)" if cand_pass else "ivf_batched_scan_kernel / ivf_scan_kernel (canonical f32 scan)",
        "launch_ms": round(scan_ms, 4), "launches_per_step": 2 if fam["ivf_sample_scan"] else 1,
        "bytes_per_launch": int(bytes_moved), "rows_read_per_step": int(rows_read), "rows_probed_union_per_step": int(rows_unique),
        "whole_step_gbs": round(bytes_moved / (step_ms * 1e-3) / 1e9, 1),
        "whole_step_frac": round(bytes_moved / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "non_scan_ms_per_step": round(step_ms - scan_ms, 4),
        "mfma_tflops": round(mfma_tf, 1), "mfma_frac_of_2500": round(mfma_tf / 2500.0, 4),
        "per_query_model_gbs": round(rows_model * (4 * d + 4) / (scan_ms * 1e-3) / 1e9, 1) if scan_ms > 0 else None,
        "prefilter": [pf1[0] - pf0[0], pf1[1] - pf0[1]],
        "pruned_pair_fraction": round(pruned_frac, 4),
        "step_kernels_ms": {f: round(v, 4) for f, v in fam.items() if v},
        "note": "achieved / frac = the bytes the two launches READ -- the rows of the lists their plans hold (counted on the device: the probe pruning keeps lists out of them; rows_probed_union_per_step is what the reference's scan would visit) x (2d + 8) B: the fp16 "
                "shadow row, its f32 norm and its id -- / (sample + main launch time, HIP events on the launch stream); "
                "whole_step_* = the same bytes over the whole step; traffic: HBM bytes of the two launches per step from the FETCH_SIZE (x2, gfx950) + "
                "WRITE_SIZE passes of this step kept in profiles/traffic.json (null when the run's shape is not the measured one); prefilter = (queries through the candidate pass, queries that needed "
                "the canonical fallback) during the profiled steps; per_query_model_gbs exceeds HBM speed because one pass over "
                "a list serves every query of the step that probes it",
    }

    extra = {}
    solo = world == 1 and not args.headline_only

    # ---- N > 1: BASELINE configs[3] as a weak-scaling family -- 12.5M rows, 2048 lists and 8 probes PER RANK of one logical
    # IVFFLAT index (N = 8: 100M x 1536, nlist 16384, nprobe 64, lists list_id % 8).  Every rank is shown every row of the
    # index (generated on its device, chunk by chunk) and keeps the rows of its lists; the coarse centroids are the blob centres
    # of the data model (identical on every rank: nothing to train or broadcast).
    def c4_sharded_build():
        d4, nl_g = 1536, 2048 * world
        mdl = _latent_model(d4, 99, dev, nl_g)
        cent = (mdl[0] @ mdl[1]).contiguous()
        six = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_IP, d4, "ncentroids=%d,shard_rank=%d,shard_world=%d" % (nl_g, rank, world))
        six.set_centroids(cent.cpu().numpy())
        t1 = time.time()
        chunk = 500_000
        buf = torch.empty((chunk, d4), device=dev, dtype=torch.float32)
        ids = torch.empty((chunk,), device=dev, dtype=torch.int64)
        # rows generated PER RANK on the device: the coarse centroids are the blob centres, so rank r draws from the blobs
        # r, r + world, ... -- the lists it owns under list_id % world (the few rows that fall nearest to a foreign centre are
        # dropped by the shard at add time); ids = rank * rows_per_rank + i
        g = torch.Generator(device=dev).manual_seed(1234 + rank)
        for lo in range(0, args.c4_rows, chunk):
            m = min(chunk, args.c4_rows - lo)
            _sample_of_blobs(mdl, m, g, dev, rank, world, buf)
            torch.arange(rank * args.c4_rows + lo, rank * args.c4_rows + lo + m, out=ids[:m])
            six.add(buf.data_ptr(), ids=ids.data_ptr(), n=m, mem=capi.MEM_DEVICE)
        del buf, ids
        six.build()
        torch.cuda.synchronize()
        build_s = time.time() - t1
        return six, mdl, build_s

    def c4_sharded():
        # every rank builds; the ranks agree that ALL of them did before the first collective search
        built, err = None, None
        try:
            built = c4_sharded_build()
        except Exception as e:  # noqa: BLE001 -- reported below, on every rank alike
            err = e
        okt = torch.tensor([1 if built is not None else 0], device="cpu" if args.test_single_device else dev)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        if int(okt.item()) == 0:
            if built is not None:
                built[0].close()
            raise RuntimeError("c4_sharded: a rank could not build its shard (%r)" % (err,))
        six, mdl, build_s = built
        d4, nl_g, npb = 1536, 2048 * world, 8 * world
        total_rows = args.c4_rows * world
        res = {"workload": "IVFFLAT %d x %d f32 inner product, nlist %d, nprobe %d, lists list_id %% %d, top-%d; weak scaling family "
                           "(12.5M rows generated on each rank's device, 2048 lists, 8 probes per rank; every rank searches the same "
                           "batch, so qps stays ~constant while the table grows with N)" % (total_rows, d4, nl_g, npb, world, k),
               "rows_on_rank0": six.num_data, "build_s": round(build_s, 1), "scaling": "weak", "batches": {}}
        for bq in (4096, 1024):
            qs = make_queries(mdl, 4 * bq, 4321, dev)
            o_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
            o_d = torch.empty((bq, k), device=dev, dtype=torch.float32)

            def sstep(i):
                six.shard_search_device(comm, qs[(i % 4) * bq:(i % 4 + 1) * bq].data_ptr(), bq, k, npb, o_i.data_ptr(), o_d.data_ptr(), stream)
            for i in range(3):
                sstep(i)
            fence()
            t2 = time.perf_counter()
            for i in range(10):
                sstep(i)
            fence()
            el = time.perf_counter() - t2
            tt = torch.tensor([el], device="cpu" if args.test_single_device else dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
            res["batches"][str(bq)] = {"qps": round(10 * bq / el, 1), "ms_per_batch": round(el / 10 * 1e3, 4)}
        six.close()
        return res

    if world > 1 and not args.headline_only and "c4" not in skip:
        # The leg is COLLECTIVE: a rank that fails in it (out of memory while it builds 12.5M x 1536 rows, a lost peer) leaves the others
        # waiting in an all-gather, and the run would end without its line.  The headline is measured by now: a watchdog prints it
        # (with the leg marked as timed out) and ends the process if the leg has not come back in --leg-timeout seconds.
        import threading

        def bail():
            if rank == 0:
                emit({"metric": "QPS at recall@10>=0.95, 1Mx768-d L2 top-10 (IVFFLAT nlist=1024 nprobe=%d)" % nprobe,
                      "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
                      "scaling": "weak" if routed else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                      "config": {"workload": "IVFFLAT nlist=%d, %dx%d f32, L2, nprobe=%d, top-%d, batch %d queries/step "
                                             "(BASELINE.json configs[1])" % (nlist, n, d, nprobe, k, B),
                                 "rows": n, "dim": d, "nlist": nlist, "nprobe": nprobe, "k": k, "batch": B,
                                 "parallelism": "lists %% %d, %s; transport: %s" % (world, "routed" if routed else "replicated", comm_kind),
                                 "streams": 1, "data_model": data_desc},
                      "recall_at_10": None, "p50_ms_batch1": None, "roofline": roof, "multi_gpu": multi_gpu, "cpu_baseline": None,
                      "c4_sharded": {"error": "the collective leg did not return within %d s: line printed by the watchdog" % args.leg_timeout},
                      "setup_s": round(setup_s, 1)})
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        wd = threading.Timer(args.leg_timeout, bail)
        wd.daemon = True
        wd.start()
        leg("c4_sharded", c4_sharded, extra)
        wd.cancel()

    # ---- the same index at other step sizes (20 timed steps each)
    def other_batches():
        res = {}
        for b2 in (1, 16, 64, 256, 1024):
            if b2 >= B:
                continue
            o_i = torch.empty((b2, k), device=dev, dtype=torch.int64)
            o_d = torch.empty((b2, k), device=dev, dtype=torch.float32)

            def step2(i):
                lo = (i % (n_pool * B // b2)) * b2
                ix.search_device(q_all[lo:lo + b2].data_ptr(), b2, k, nprobe, o_i.data_ptr(), o_d.data_ptr(), stream)
            dt2 = timed(step2, 40 if b2 <= 64 else 20)
            f2 = profiled(step2, 8, STEP_FAMILIES)
            u2 = sum(ix.scanned_rows(q_all[i * b2:(i + 1) * b2].cpu().numpy(), nprobe)[2] for i in range(8)) / 8
            sc = f2["ivf_scan"] + f2["ivf_sample_scan"] + f2["lat_search"]
            # bytes the path MOVES: the two-launch path reads f32 (3 MB of centroids + the probed rows + their ids), the canonical
            # batched scan f32 rows, the shadow pass fp16 rows + norms + ids
            shadow = bool(f2["ivf_sample_scan"])
            # the shadow pass: rows its launches read (pruning counted); the canonical paths read f32 rows of the lists they keep --
            # not counted on the device, so no fraction is quoted for them once pruning may have thinned the probes
            by = rows_read_per_step(step2, 8) * (2 * d + 8) if shadow else None
            res[str(b2)] = {"qps": round(b2 / dt2, 1), "ms_per_step": round(dt2 * 1e3, 4), "list_scan_ms": round(sc, 4),
                            "hbm_frac": round(by / (sc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sc and by else None,
                            "whole_step_hbm_frac": round(by / dt2 / 1e9 / HBM_PEAK_GBS, 4) if by else None,
                            "bytes_moved_per_step": int(by) if by else None, "rows_probed_union_per_step": int(u2),
                            "path": "two-launch (f32 rows)" if f2["lat_search"] else ("fp16-shadow pass" if shadow else "canonical (f32 rows)")}
        return res

    # ---- SURVEY 8d latency protocol through the host-pointer entry (query in, k ids + distances out)
    def latency():
        qh = q_all[:4096].cpu().numpy()
        sp = "nprobe=%d" % nprobe
        for i in range(100):
            ix.search(qh[i:i + 1], k, sp)
        lat = np.empty(10000)
        for i in range(10000):
            t1 = time.perf_counter()
            ix.search(qh[i % 4096:i % 4096 + 1], k, sp)
            lat[i] = time.perf_counter() - t1
        res = {"calls": 10000, "p50_us": round(float(np.percentile(lat, 50)) * 1e6, 1),
               "p99_us": round(float(np.percentile(lat, 99)) * 1e6, 1), "qps_1_thread": round(1.0 / float(lat.mean()), 1),
               "api": "msvs_index_search (host pointers; includes launch + D2H of the k results; python ctypes call overhead included)"}
        # concurrency: NATIVE host threads, one query per msvs_index_search call (the reference's calling pattern; python threads
        # spend ~30 us per call under the GIL and cannot keep more than a few calls in flight: 26 k QPS whatever the library
        # does).  Callers beyond 8 in flight are served in batches by msvs_index_search's combining front end.
        import myscaledb_amd.host as mhost
        for c in (1, 8, 64, 128):
            per = 10000 // c if c > 1 else 4000
            if c > 8:
                mhost.concurrent_search(ix, qh, c, 20, k, sp)  # (the index's worker thread and its arenas exist)
            b0 = capi.combine_stats()
            sec, al, _, _ = mhost.concurrent_search(ix, qh, c, per, k, sp)
            b1 = capi.combine_stats()
            res["threads_%d" % c] = {"qps": round(c * per / sec, 1), "p50_us": round(float(np.percentile(al, 50)), 1),
                                     "p99_us": round(float(np.percentile(al, 99)), 1),
                                     "combined_batches": int(b1[1] - b0[1]), "queries_in_batches": int(b1[2] - b0[2]),
                                     "driver": "native threads (msvs_host_concurrent_search)"}
        # small batches through the same entry (what a combined batch of concurrent callers costs; a few rows of a batch_distance call)
        small = {}
        for b in (4, 8, 16, 32, 64, 128, 256):
            for i in range(10):
                ix.search(qh[i * b:(i + 1) * b], k, sp)
            t1 = time.perf_counter()
            for i in range(100):
                ix.search(qh[(i % 16) * b:(i % 16 + 1) * b], k, sp)
            dt_ = (time.perf_counter() - t1) / 100
            small[str(b)] = {"us_per_call": round(dt_ * 1e6, 1), "qps": round(b / dt_, 1)}
        res["host_pointer_small_batches"] = small
        # the seam's real call form for a batch (VIWithDataPart.cpp:900-926: a host DataSet<float> in, host result buffers out):
        # H2D of 4096 x 768 x 4 B = 12.6 MB, the search, D2H of the results -- one thread; then two host threads (each on its own
        # stream: one's copies beside the other's search -- the double-buffered form a serving loop would run)
        import threading
        for i in range(3):
            ix.search(qh, k, sp)
        t1 = time.perf_counter()
        for i in range(20):
            ix.search(qh, k, sp)
        hp = (time.perf_counter() - t1) / 20
        res["host_pointer_batch4096"] = {"qps": round(4096 / hp, 1), "ms": round(hp * 1e3, 4),
                                         "api": "msvs_index_search, 4096 queries in HOST memory per call (pageable: numpy), results to host"}

        def worker(reps):
            for _ in range(reps):
                ix.search(qh, k, sp)
        th = [threading.Thread(target=worker, args=(3,)) for _ in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        th = [threading.Thread(target=worker, args=(20,)) for _ in range(2)]
        t1 = time.perf_counter()
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        hp2 = (time.perf_counter() - t1) / 40
        res["host_pointer_batch4096_two_threads"] = {"qps": round(4096 / hp2, 1), "ms_per_batch": round(hp2 * 1e3, 4),
                                                     "note": "two host threads, each msvs_index_search of 4096 host queries on its own stream (ctypes releases the GIL)"}
        return res

    # ---- recall@10 against the exact scan of the same rows
    recall = None
    if solo:
        flat = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, d)
        flat.add(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
        flat.build()
        qh = q_all[:1000].cpu().numpy()
        gt, _ = flat.search(qh, k)
        got, _ = ix.search(qh, k, "nprobe=%d" % nprobe)
        recall = recall_at_k(got, gt, k)
        flat.close()

    # ---- CPU baseline + oracle check (before the big legs free / reuse memory)
    def cpu_baseline():
        from oracle import oracle as o
        cent, off, vecs, lids = ix.export()
        cores = cpu_cores()
        qh = q_all.cpu().numpy()  # n_pool x batch queries
        o.simd_ivf_search(cent, off, vecs, lids, qh[:cores], nprobe, k, o.METRIC_L2, cores)  # builds -march=native, warms up
        t1 = time.perf_counter()
        o.simd_ivf_search(cent, off, vecs, lids, qh[:4 * cores], nprobe, k, o.METRIC_L2, cores)
        per_round = max(time.perf_counter() - t1, 1e-3) / 4
        nqs = int(min(qh.shape[0], max(cores, cores * int(args.cpu_seconds / per_round))))
        t1 = time.perf_counter()
        si, _ = o.simd_ivf_search(cent, off, vecs, lids, qh[:nqs], nprobe, k, o.METRIC_L2, cores)
        cpu_s = time.perf_counter() - t1
        t1 = time.perf_counter()
        o.simd_ivf_search(cent, off, vecs, lids, qh[:64], nprobe, k, o.METRIC_L2, 1)
        one_thread = (time.perf_counter() - t1) / 64
        gi, gd = ix.search(qh[:nqs], k, "nprobe=%d" % nprobe)
        # the parity oracle (canonical arithmetic, no fma) on 256 of the bench queries: bit for bit
        nchk = 256
        oi, od, _ = o.ivf_search(cent, off, vecs, lids, qh[:nchk], nprobe, k, o.METRIC_L2, threads=cores)
        exact = bool((oi == gi[:nchk]).all() and (od.view(np.uint32) == gd[:nchk].view(np.uint32)).all())
        return {"value": round(nqs / cpu_s, 2), "unit": "queries/s", "cores": cores, "kind": "port",
                "simd_lanes_f32": o.simd_lanes(), "single_thread_ms_per_query": round(one_thread * 1e3, 3),
                "sample": "%d of the bench queries on the exported index structure, oracle/simd_baseline.c (fused multiply-add "
                          "SIMD loops built -O3 -march=native on this machine, OpenMP across queries, %d threads), %.1f s; "
                          "recall@%d of its ids against the GPU result %.4f (fma changes last bits: not a parity oracle)"
                          % (nqs, cores, cpu_s, k, recall_at_k(si, gi, k)),
                "oracle_check": {"queries": nchk, "ids_and_distances_bit_identical": exact,
                                 "oracle": "oracle/msvs_oracle.c oracle_ivf_search_mt (canonical f32 arithmetic)"}}

    if solo and "other_batches" not in skip:
        leg("other_batches", other_batches, extra)
    if solo and "latency" not in skip:
        leg("latency", latency, extra)
    cpu = None
    if solo and rank == 0 and not args.no_cpu_baseline and "cpu" not in skip:
        tmp = {}
        leg("cpu", cpu_baseline, tmp)
        cpu = tmp["cpu"]

    # ---- SURVEY 8d's own data models, each at ITS recall@10 >= 0.95 operating point (nprobe sweep), same index parameters
    def operating_point(kind):
        xi, qi, data = data_model(kind, n, 2 * B, d, dev)
        t1 = time.time()
        iix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, ivf_params(nlist, n))
        iix.train(xi.data_ptr(), n=n, mem=capi.MEM_DEVICE)
        iix.add(xi.data_ptr(), n=n, mem=capi.MEM_DEVICE)
        iix.build()
        torch.cuda.synchronize()
        build_s = time.time() - t1
        fl = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, d)
        fl.add(xi.data_ptr(), n=n, mem=capi.MEM_DEVICE)
        fl.build()
        qh = qi[:1000].cpu().numpy()
        gt, _ = fl.search(qh, k)
        res = {"data": data, "batch": B, "build_s": round(build_s, 1), "lists": iix.list_stats(), "recall_at_%d" % k: {}}
        op = None
        for npb in (1, 2, 4, 8, 16, 32, 64, 128, 256):  # the coarse top-k limit is 256 probes
            if npb > nlist:
                break
            got, _ = iix.search(qh, k, "nprobe=%d" % npb)
            r = recall_at_k(got, gt, k)
            res["recall_at_%d" % k]["nprobe_%d" % npb] = round(r, 4)
            if r >= 0.95:
                op = npb
                break

        def run_at(npb):
            def istep(i):
                iix.search_device(qi[(i % 2) * B:(i % 2 + 1) * B].data_ptr(), B, k, npb, out_ids.data_ptr(), out_dis.data_ptr(), stream)
            p0 = capi.prefilter_stats()
            dt = timed(istep, 20)
            p1 = capi.prefilter_stats()
            fo = profiled(istep, 4, STEP_FAMILIES)
            uni = sum(iix.scanned_rows(qi[j * B:(j + 1) * B].cpu().numpy(), npb)[2] for j in range(2)) / 2
            sc = fo["ivf_scan"] + fo["ivf_sample_scan"]
            mv = rows_read_per_step(istep, 2) * (2 * d + 8)
            capi.set_option("rerank_stats", "1")
            ps0 = capi.debug_prune_stats()
            for i in range(2):
                istep(i)
            torch.cuda.synchronize()
            ps1 = capi.debug_prune_stats()
            capi.set_option("rerank_stats", None)
            return {"nprobe": npb, "qps": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 4), "list_scan_ms": round(sc, 4),
                    "pruned_pair_fraction": round((ps1[0] - ps0[0]) / float(2 * B * npb), 4),  # (query, list) pairs dropped / pairs probed, two steps
                    "union_rows_per_step": int(uni), "rows_read_per_step": int(mv / (2 * d + 8)),
                    "roofline_frac": round(mv / (sc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sc else None,
                    "whole_step_frac": round(mv / dt / 1e9 / HBM_PEAK_GBS, 4),
                    "candidate_pass_queries": p1[0] - p0[0], "fallback_queries": p1[1] - p0[1],
                    "step_kernels_ms": {f: round(v, 4) for f, v in fo.items() if v}}
        if op is not None:
            del xi
            res["at_recall_0.95"] = run_at(op)
            if kind == "mid":
                # the metric's other half at this operating point: one query per msvs_index_search call (host pointers), and the CPU
                # port on the exported index structure beside it (bounded sample)
                for i in range(30):
                    iix.search(qh[i:i + 1], k, "nprobe=%d" % op)
                lat1 = np.empty(1500)
                for i in range(1500):
                    t2 = time.perf_counter()
                    iix.search(qh[i % 1000:i % 1000 + 1], k, "nprobe=%d" % op)
                    lat1[i] = time.perf_counter() - t2
                res["at_recall_0.95"]["single_query_p50_us"] = round(float(np.percentile(lat1, 50)) * 1e6, 1)
                res["at_recall_0.95"]["single_query_p99_us"] = round(float(np.percentile(lat1, 99)) * 1e6, 1)
                if not args.no_cpu_baseline and "cpu" not in skip:
                    from oracle import oracle as o
                    cent, off, vecs, lids = iix.export()
                    cores = cpu_cores()
                    o.simd_ivf_search(cent, off, vecs, lids, qh[:cores], op, k, o.METRIC_L2, cores)
                    nqs = min(1000, 16 * cores)
                    t2 = time.perf_counter()
                    si, _ = o.simd_ivf_search(cent, off, vecs, lids, qh[:nqs], op, k, o.METRIC_L2, cores)
                    cs = time.perf_counter() - t2
                    oi_, od_, _ = o.ivf_search(cent, off, vecs, lids, qh[:64], op, k, o.METRIC_L2, threads=cores)
                    gi_, gd_ = iix.search(qh[:64], k, "nprobe=%d" % op)
                    res["at_recall_0.95"]["cpu_port"] = {"qps": round(nqs / cs, 1), "cores": cores, "queries": nqs, "kind": "port",
                                                         "oracle_check_64_queries_bit_identical": bool((oi_ == gi_).all() and (od_.view(np.uint32) == gd_.view(np.uint32)).all())}
                    del cent, off, vecs, lids
        else:
            # ... or, twice as fast, through the list scan's fp16 shadow: an IVFFLAT index of 256 lists with ALL of them probed
            # is an exhaustive scan too (every row is in some list; results exact as always), and its candidate pass reads
            # 2 bytes per element where the FLAT table pass reads 4
            eix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, ivf_params(256, n))
            eix.train(xi.data_ptr(), n=n, mem=capi.MEM_DEVICE)
            eix.add(xi.data_ptr(), n=n, mem=capi.MEM_DEVICE)
            eix.build()
            del xi
            got, _ = eix.search(qh, k, "nprobe=256")
            r_e = recall_at_k(got, gt, k)

            def estep(i):
                eix.search_device(qi[(i % 2) * B:(i % 2 + 1) * B].data_ptr(), B, k, 256, out_ids.data_ptr(), out_dis.data_ptr(), stream)
            p0 = capi.prefilter_stats()
            dte = timed(estep, 5, warmup=2)
            p1 = capi.prefilter_stats()
            fe = profiled(estep, 2, STEP_FAMILIES)
            tiles = -(-B // 96)
            sce = fe["ivf_scan"] + fe["ivf_sample_scan"]
            dpad = (d + 63) // 64 * 64
            mf = 2.0 * B * n * dpad / (sce * 1e-3) / 1e12 if sce else 0.0
            res["exhaustive_ivf256"] = {"method": "IVFFLAT nlist 256, nprobe 256: every list probed by every query (fp16-shadow candidate pass, canonical re-rank, certificate)",
                                        "recall": round(r_e, 4), "qps": round(B / dte, 1), "ms_per_step": round(dte * 1e3, 4),
                                        "list_scan_ms": round(sce, 4), "shadow_passes_per_step": tiles,
                                        "bound": "mfma", "mfma_tflops": round(mf, 1), "roofline_frac": round(mf / MFMA_F16_PEAK_TF, 4),
                                        "whole_step_mfma_frac": round(2.0 * B * n * dpad / dte / 1e12 / MFMA_F16_PEAK_TF, 4),
                                        "hbm_frac_side": round(n * (2 * d + 8) / (sce * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sce else None,
                                        "candidate_pass_queries": p1[0] - p0[0], "fallback_queries": p1[1] - p0[1],
                                        "step_kernels_ms": {f: round(v, 4) for f, v in fe.items() if v}, "lists": eix.list_stats()}
            eix.close()
            # no structure for an IVF index to use (recall ~ 1.5 x the fraction of the rows scanned): the operating point is the
            # exhaustive scan of the same rows, batched through the FLAT index's candidate pass (recall 1.0 by construction)
            def fstep(i):
                fl.search_device(qi[(i % 2) * B:(i % 2 + 1) * B].data_ptr(), B, k, 0, out_ids.data_ptr(), out_dis.data_ptr(), stream)
            dtf = timed(fstep, 5, warmup=2)
            ff = profiled(fstep, 2, STEP_FAMILIES)
            res["exhaustive_flat"] = {"method": "exhaustive FLAT index scan (IVFFLAT nlist %d stays below recall 0.95 up to nprobe 256)" % nlist,
                                      "recall": 1.0, "qps": round(B / dtf, 1), "ms_per_step": round(dtf * 1e3, 4),
                                      "bound": "mfma", "whole_step_mfma_tflops": round(2.0 * B * n * dpad / dtf / 1e12, 1),
                                      "whole_step_mfma_frac": round(2.0 * B * n * dpad / dtf / 1e12 / MFMA_F16_PEAK_TF, 4),
                                      "step_kernels_ms": {f: round(v, 4) for f, v in ff.items() if v}}
            # the metric's other half at this operating point -- p50 latency: one query per msvs_index_search call (host pointers, the
            # reference's calling form VIWithDataPart.cpp:922-926) and small batches, over the FLAT index's fp16 shadow (HBM-bound:
            # n x (2d + 8) B per pass) with the canonical re-rank + certificate behind it; results == the batch path's bits
            calls = 4000
            for i in range(50):
                fl.search(qh[i:i + 1], k)
            latf = np.empty(calls)
            same = True
            for i in range(calls):
                t1 = time.perf_counter()
                gi_, gd_ = fl.search(qh[i % 1000:i % 1000 + 1], k)
                latf[i] = time.perf_counter() - t1
                if i < 1000:
                    same = same and bool((gi_[0] == gt[i]).all())
            shadow_b = n * (2 * d + 8)
            res["flat_latency"] = {"calls": calls, "p50_us": round(float(np.percentile(latf, 50)) * 1e6, 1),
                                   "p99_us": round(float(np.percentile(latf, 99)) * 1e6, 1),
                                   "qps_1_thread": round(1.0 / float(latf.mean()), 1), "recall": 1.0,
                                   "single_ids_equal_batch_ids_1000_queries": same,
                                   "hbm_frac_of_p50": round(shadow_b / float(np.percentile(latf, 50)) / 1e9 / HBM_PEAK_GBS, 4),
                                   "api": "msvs_index_search on a FLAT index, 1 query per call, host pointers (H2D of the query, D2H of the k results, python ctypes included)"}
            fb_ = {}
            for b_ in (1, 4, 16, 64, 256):
                def sstep(i, b_=b_):
                    fl.search_device(qi[(i % 8) * b_:(i % 8 + 1) * b_].data_ptr(), b_, k, 0, out_ids.data_ptr(), out_dis.data_ptr(), stream)
                dts = timed(sstep, 20, warmup=3)
                fs_ = profiled(sstep, 4, ("flat_shadow_scan",))
                fb_["batch_%d" % b_] = {"qps": round(b_ / dts, 1), "ms_per_step": round(dts * 1e3, 4),
                                         "shadow_scan_ms": round(fs_["flat_shadow_scan"], 4),
                                         "whole_step_hbm_frac": round(shadow_b / dts / 1e9 / HBM_PEAK_GBS, 4),
                                         "shadow_scan_hbm_frac": round(shadow_b / (fs_["flat_shadow_scan"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if fs_["flat_shadow_scan"] else None}
            res["flat_batches"] = dict(fb_, bytes_per_pass=shadow_b, note="device-resident queries (search_device); moved bytes = the fp16 shadow + norms + ids, read once per step")
            best = "exhaustive_ivf256" if res["exhaustive_ivf256"]["recall"] >= 0.95 and res["exhaustive_ivf256"]["qps"] > res["exhaustive_flat"]["qps"] else "exhaustive_flat"
            res["at_recall_0.95"] = dict(res[best], chosen=best)
        if op != nprobe:
            res["at_config_nprobe"] = run_at(nprobe)
        fl.close()
        iix.close()
        return res

    for kind in ("blobs03", "iid", "latent32", "mid"):
        if solo and kind not in skip:
            leg(kind, lambda kind=kind: operating_point(kind), extra)

    # ---- other BASELINE configurations
    other_cfg = {}

    def c1():
        """FLAT brute force 10k x 128 (configs[0]): the seam-A2 call (host pointers, rows uploaded per call like the
        reference's per-part scan) and the resident-index form."""
        rng = np.random.default_rng(1234)
        xb = rng.standard_normal((10000, 128), dtype=np.float32)
        qb = np.random.default_rng(4321).standard_normal((1000, 128), dtype=np.float32)
        for i in range(20):
            capi.knn(qb[i:i + 1], xb, 10, capi.METRIC_L2)
        lat = []
        for i in range(300):
            t1 = time.perf_counter()
            capi.knn(qb[i:i + 1], xb, 10, capi.METRIC_L2)
            lat.append(time.perf_counter() - t1)
        fl = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, 128)
        fl.add(xb)
        fl.build()
        qd = torch.from_numpy(qb).to(dev)
        o_i = torch.empty((1000, 10), device=dev, dtype=torch.int64)
        o_d = torch.empty((1000, 10), device=dev, dtype=torch.float32)
        dt1 = timed(lambda i: fl.search_device(qd[i % 1000:i % 1000 + 1].data_ptr(), 1, 10, 0, o_i.data_ptr(), o_d.data_ptr(), stream), 200)
        dtb = timed(lambda i: fl.search_device(qd.data_ptr(), 1000, 10, 0, o_i.data_ptr(), o_d.data_ptr(), stream), 50)
        fl.close()
        res = {"workload": "FLAT 10000 x 128 f32 L2 top-10",
               "knn_host_call_p50_us": round(float(np.percentile(lat, 50)) * 1e6, 1),
               "resident_nq1": {"us_per_call": round(dt1 * 1e6, 1), "hbm_frac": round(10000 * 512 / dt1 / 1e9 / HBM_PEAK_GBS, 4)},
               "resident_nq1000": {"qps": round(1000 / dtb, 1), "ms_per_step": round(dtb * 1e3, 4)}}
        if not args.no_cpu_baseline and "cpu" not in skip:
            # configs[0] is the reference's own CPU-runnable case: the same scan on ONE host core (SIMD restatement), per call
            from oracle import oracle as o
            cores = cpu_cores()
            o.simd_knn(qb[:1], xb, 10, o.METRIC_L2, 1)
            t1 = time.perf_counter()
            for i in range(300):
                o.simd_knn(qb[i:i + 1], xb, 10, o.METRIC_L2, 1)
            one = (time.perf_counter() - t1) / 300
            t1 = time.perf_counter()
            reps = 0
            while time.perf_counter() - t1 < 2.0:
                o.simd_knn(qb, xb, 10, o.METRIC_L2, cores)
                reps += 1
            allc = reps * 1000 / (time.perf_counter() - t1)
            res["cpu_baseline"] = {"value": round(1.0 / one, 1), "unit": "queries/s", "cores": 1, "kind": "port",
                                   "us_per_call_one_core": round(one * 1e6, 1), "qps_all_cores_nq1000": round(allc, 1), "all_cores": cores,
                                   "sample": "oracle/simd_baseline.c simd_knn: 300 single-query calls on one core (python ctypes call "
                                             "overhead included on both sides), and the 1000-query batch on %d threads for 2 s" % cores}
            res["seam_a2_note"] = ("the drop-in host-pointer call uploads the 5 MB block per call (%.0f us p50) and is SLOWER than one CPU core "
                                   "(%.0f us) for a 10k-row block; the scan only pays off through the resident form (msvs_cache_* / "
                                   "msvs_block_upload + msvs_knn_resident: %.0f us per call, %.1f M QPS at 1000 queries per call)"
                                   % (res["knn_host_call_p50_us"], one * 1e6, dt1 * 1e6, 1000 / dtb / 1e6))
        return res

    big = {}

    def c3():
        """MSTG stand-in (IVFFLAT; MSTG's graph/partition format is closed source): 10M x 768 cosine, batches of 64."""
        nb, nl, npb, bq = args.big_rows, 4096, 32, 64
        mdl = _latent_model(d, 99, dev, 4096)
        g = torch.Generator(device=dev).manual_seed(1234)
        cix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_COSINE, d, "ncentroids=%d,kmeans_iters=8,train_sample=%d" % (nl, nl * 48))
        t1 = time.time()
        chunk = 1_000_000
        xs = _sample(mdl, min(nb, nl * 48), g, dev)
        cix.train(xs.data_ptr(), n=xs.shape[0], mem=capi.MEM_DEVICE)
        del xs
        buf = torch.empty((chunk, d), device=dev, dtype=torch.float32)
        g = torch.Generator(device=dev).manual_seed(1234)
        for lo in range(0, nb, chunk):
            m = min(chunk, nb - lo)
            _sample(mdl, m, g, dev, out=buf)
            cix.add(buf.data_ptr(), n=m, mem=capi.MEM_DEVICE)
        del buf
        cix.build()
        torch.cuda.synchronize()
        build_s = time.time() - t1
        qs = make_queries(mdl, 8 * bq, 4321, dev)
        o_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
        o_d = torch.empty((bq, k), device=dev, dtype=torch.float32)

        def cstep(i):
            cix.search_device(qs[(i % 8) * bq:(i % 8 + 1) * bq].data_ptr(), bq, k, npb, o_i.data_ptr(), o_d.data_ptr(), stream)
        dt = timed(cstep, 30)
        f3 = profiled(cstep, 8, STEP_FAMILIES)
        uni = sum(cix.scanned_rows(qs[i * bq:(i + 1) * bq].cpu().numpy(), npb)[2] for i in range(8)) / 8
        sc = f3["ivf_scan"] + f3["ivf_sample_scan"]
        rr = rows_read_per_step(cstep, 8)
        big["index"], big["model"], big["nprobe"] = cix, mdl, npb
        res = {"workload": "IVFFLAT (MSTG stand-in) %d x %d cosine, nlist=%d, nprobe=%d, batch %d, top-%d" % (nb, d, nl, npb, bq, k),
               "qps": round(bq / dt, 1), "ms_per_batch": round(dt * 1e3, 4), "build_s": round(build_s, 1),
               "union_rows_per_batch": int(uni), "rows_read_per_batch": int(rr), "list_scan_ms": round(sc, 4),
               "roofline_frac": round(rr * (2 * d + 8) / (sc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sc else None,
               "whole_step_frac": round(rr * (2 * d + 8) / dt / 1e9 / HBM_PEAK_GBS, 4),
               "bytes_moved_per_batch": int(rr * (2 * d + 8)),
               "step_kernels_ms": {f: round(v, 4) for f, v in f3.items() if v}}
        if not args.no_cpu_baseline and "cpu" not in skip:
            # the SIMD CPU restatement on the lists a 16-query sample of one batch probes (exported from the index), repeated
            cores = cpu_cores()
            cstep(0)
            torch.cuda.synchronize()
            gi, gd = o_i.cpu().numpy()[:16], o_d.cpu().numpy()[:16]
            sub = probed_sub_index(cix, qs[:16].cpu().numpy(), npb, capi.METRIC_COSINE)
            oi, od = oracle_on_sub_index(sub, npb, k, capi.METRIC_COSINE, threads=cores)
            v, sample = simd_baseline_on_sub_index(sub, npb, k, min(args.cpu_seconds, 8.0), cores)
            res["cpu_baseline"] = {"value": round(v, 2), "unit": "queries/s", "cores": cores, "kind": "port",
                                   "sample": "oracle/simd_baseline.c on the %d lists the first 16 queries of a batch probe (%d rows), %s"
                                             % (int((np.diff(sub[1]) > 0).sum()), int(sub[1][-1]), sample),
                                   "oracle_check": {"queries": 16, "ids_and_distances_bit_identical":
                                                    bool((oi == gi).all() and (od.view(np.uint32) == gd.view(np.uint32)).all())}}
        return res

    def c4():
        """One GPU's share of BASELINE configs[3] (IVFFLAT 100M x 1536 f32, inner product, nlist 16384, nprobe 64, lists
        list_id % 8): 12.5M rows in 2048 lists, every query probing 8 of them -- the work msvs_shard_search_device leaves on a
        rank (its coarse quantiser covers nq / 8 queries x 16384 centroids = nq x 2048 here).  The sharded family itself runs
        under --gpus N."""
        nb, d4, nl, npb = args.c4_rows, 1536, 2048, 8
        mdl = _latent_model(d4, 99, dev, nl)
        g = torch.Generator(device=dev).manual_seed(1234)
        cix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_IP, d4, ivf_params(nl, nb))
        t1 = time.time()
        xs = _sample(mdl, min(nb, 262144), g, dev)
        cix.train(xs.data_ptr(), n=xs.shape[0], mem=capi.MEM_DEVICE)
        del xs
        chunk = 500_000
        buf = torch.empty((chunk, d4), device=dev, dtype=torch.float32)
        g = torch.Generator(device=dev).manual_seed(1234)
        for lo in range(0, nb, chunk):
            m = min(chunk, nb - lo)
            _sample(mdl, m, g, dev, out=buf)
            cix.add(buf.data_ptr(), n=m, mem=capi.MEM_DEVICE)
        del buf
        cix.build()
        torch.cuda.synchronize()
        build_s = time.time() - t1
        res = {"workload": "one GPU of 8: IVFFLAT %d x %d f32 inner product, %d lists (16384 / 8), %d probes per query (64 / 8), top-%d"
                           % (nb, d4, nl, npb, k), "build_s": round(build_s, 1), "lists": cix.list_stats(), "batches": {}}
        for bq in (4096, 1024, 64):
            qs = make_queries(mdl, 4 * bq, 4321, dev)
            o_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
            o_d = torch.empty((bq, k), device=dev, dtype=torch.float32)

            def cstep(i):
                cix.search_device(qs[(i % 4) * bq:(i % 4 + 1) * bq].data_ptr(), bq, k, npb, o_i.data_ptr(), o_d.data_ptr(), stream)
            capi.release_scratch()  # (the arena of the previous batch size would be given back somewhere inside the timed steps: a 30 ms free + malloc)
            p0 = capi.prefilter_stats()
            dt = timed(cstep, 12)
            p1 = capi.prefilter_stats()
            f4 = profiled(cstep, 4, STEP_FAMILIES)
            uni = sum(cix.scanned_rows(qs[j * bq:(j + 1) * bq].cpu().numpy(), npb)[2] for j in range(4)) / 4
            sc = f4["ivf_scan"] + f4["ivf_sample_scan"]
            mv = rows_read_per_step(cstep, 4) * (2 * d4 + 8)
            res["batches"][str(bq)] = {
                "qps": round(bq / dt, 1), "ms_per_batch": round(dt * 1e3, 4), "list_scan_ms": round(sc, 4),
                "union_rows_per_batch": int(uni), "rows_read_per_batch": int(mv / (2 * d4 + 8)),
                "roofline_frac": round(mv / (sc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sc else None,
                "roofline_gbs": round(mv / (sc * 1e-3) / 1e9, 1) if sc else None,
                "whole_step_frac": round(mv / dt / 1e9 / HBM_PEAK_GBS, 4),
                "candidate_pass_queries": p1[0] - p0[0], "fallback_queries": p1[1] - p0[1],
                "step_kernels_ms": {f: round(v, 4) for f, v in f4.items() if v}}
            if bq == 64:
                # 64 queries of a batch against the parity oracle on the lists they probe (exported from the index's own storage)
                cstep(0)
                torch.cuda.synchronize()
                t2 = time.time()
                ei, ed = oracle_on_index_lists(cix, qs[:bq].cpu().numpy(), npb, k, capi.METRIC_IP, threads=cpu_cores())
                gi, gd = o_i.cpu().numpy(), o_d.cpu().numpy()
                res["oracle_check"] = {"queries": bq, "ids_and_distances_bit_identical":
                                       bool((ei == gi).all() and (ed.view(np.uint32) == gd.view(np.uint32)).all()),
                                       "seconds": round(time.time() - t2, 1)}
        cix.close()
        return res

    def target_100m():
        """One GPU's share of the configuration north_star states its targets on -- 100M x 768-d L2 top-10 over 8 GPUs, lists
        list_id % 8 -- : 12.5M rows in 2048 local lists, 8 local probes per query (an index of nlist 16384 / nprobe 64).  Data:
        SURVEY 8d's clustered model with one blob per local list (2048 centres N(0,1)^768, sigma 0.3).  The source table stays
        resident: the exact ground truth and the oracle check read IT, not the index's storage."""
        nb, d1, nl, npb = args.c4_rows, 768, 2048, 8
        centres = blob_centres(d1, dev, nl)
        x1 = blob_sample(centres, nb, torch.Generator(device=dev).manual_seed(1234), dev)
        t1 = time.time()
        tix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d1, ivf_params(nl, nb))
        tix.train(x1[:262144].contiguous().data_ptr(), n=262144, mem=capi.MEM_DEVICE)
        chunk = 1_000_000
        for lo in range(0, nb, chunk):
            tix.add(x1[lo:lo + chunk].data_ptr(), n=min(chunk, nb - lo), mem=capi.MEM_DEVICE)
        tix.build()
        torch.cuda.synchronize()
        build_s = time.time() - t1
        qs = blob_sample(centres, 4 * 4096, torch.Generator(device=dev).manual_seed(4321), dev)
        # recall@10 of 256 queries against the exact scan of the source table (FLAT index built over it, freed afterwards)
        fl = capi.Index(capi.INDEX_FLAT, capi.METRIC_L2, d1)
        for lo in range(0, nb, chunk):
            fl.add(x1[lo:lo + chunk].data_ptr(), n=min(chunk, nb - lo), mem=capi.MEM_DEVICE)
        fl.build()
        qh = qs[:256].cpu().numpy()
        gt, _ = fl.search(qh, k)
        fl.close()
        got, _ = tix.search(qh, k, "nprobe=%d" % npb)
        res = {"workload": "one GPU of 8 of north_star's target: IVFFLAT %d x %d f32 L2, %d lists (16384 / 8), %d probes per query "
                           "(64 / 8), top-%d" % (nb, d1, nl, npb, k),
               "data": "2048 gaussian blobs (centres N(0,1)^768, seed 99), sigma 0.3, rows seed 1234, queries seed 4321 (SURVEY 8d's "
                       "clustered model, one blob per local list)",
               "build_s": round(build_s, 1), "lists": tix.list_stats(),
               "recall_at_%d" % k: round(recall_at_k(got, gt, k), 4), "recall_queries": 256, "batches": {}}
        for bq in (4096, 1024, 64):
            o_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
            o_d = torch.empty((bq, k), device=dev, dtype=torch.float32)

            def tstep(i):
                tix.search_device(qs[(i % 4) * bq:(i % 4 + 1) * bq].data_ptr(), bq, k, npb, o_i.data_ptr(), o_d.data_ptr(), stream)
            capi.release_scratch()
            p0 = capi.prefilter_stats()
            dt = timed(tstep, 12)
            p1 = capi.prefilter_stats()
            ft = profiled(tstep, 4, STEP_FAMILIES)
            uni = sum(tix.scanned_rows(qs[j * bq:(j + 1) * bq].cpu().numpy(), npb)[2] for j in range(4)) / 4
            sc = ft["ivf_scan"] + ft["ivf_sample_scan"]
            mv = rows_read_per_step(tstep, 4) * (2 * d1 + 8)
            res["batches"][str(bq)] = {
                "qps": round(bq / dt, 1), "ms_per_batch": round(dt * 1e3, 4), "list_scan_ms": round(sc, 4),
                "union_rows_per_batch": int(uni), "rows_read_per_batch": int(mv / (2 * d1 + 8)), "bytes_moved_per_batch": int(mv),
                "roofline_frac": round(mv / (sc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if sc else None,
                "roofline_gbs": round(mv / (sc * 1e-3) / 1e9, 1) if sc else None,
                "whole_step_frac": round(mv / dt / 1e9 / HBM_PEAK_GBS, 4),
                "candidate_pass_queries": p1[0] - p0[0], "fallback_queries": p1[1] - p0[1],
                "step_kernels_ms": {f: round(v, 4) for f, v in ft.items() if v}}
            if bq == 64:
                # the 64 queries of a batch against the parity oracle, the rows of the lists they probe RE-GATHERED FROM THE SOURCE
                # TABLE by id; then the SIMD CPU baseline on the same lists
                tstep(0)
                torch.cuda.synchronize()
                gi, gd = o_i.cpu().numpy(), o_d.cpu().numpy()
                t2 = time.time()
                sub = probed_sub_index(tix, qs[:bq].cpu().numpy(), npb, capi.METRIC_L2,
                                       rows_by_id=lambda ids: x1[torch.from_numpy(ids).to(dev)].cpu().numpy())
                cores = cpu_cores()
                ei, ed = oracle_on_sub_index(sub, npb, k, capi.METRIC_L2, threads=cores)
                res["oracle_check"] = {"queries": bq, "rows": "re-gathered from the source table by id (%d rows of %d lists)"
                                                              % (int(sub[1][-1]), int((np.diff(sub[1]) > 0).sum())),
                                       "ids_and_distances_bit_identical":
                                       bool((ei == gi).all() and (ed.view(np.uint32) == gd.view(np.uint32)).all()),
                                       "seconds": round(time.time() - t2, 1)}
                if not args.no_cpu_baseline and "cpu" not in skip:
                    v, sample = simd_baseline_on_sub_index(sub, npb, k, args.cpu_seconds, cores)
                    res["cpu_baseline"] = {"value": round(v, 2), "unit": "queries/s", "cores": cores, "kind": "port",
                                           "sample": "oracle/simd_baseline.c (AVX fma loops, OpenMP across queries) on the lists the 64 "
                                                     "queries probe, rows from the source table: " + sample}
                del sub
        if "cpu_baseline" in res:
            best = max(b["qps"] for b in res["batches"].values())
            res["gpu_over_cpu"] = {"at_batch_4096": round(res["batches"]["4096"]["qps"] / res["cpu_baseline"]["value"], 1),
                                   "at_batch_64": round(res["batches"]["64"]["qps"] / res["cpu_baseline"]["value"], 1),
                                   "best": round(best / res["cpu_baseline"]["value"], 1),
                                   "note": "north_star: >= 10 x the CPU-path QPS; the CPU figure is a restatement on this box's cores, not the MyScaleDB server"}
        tix.close()
        return res

    def c5():
        """Hybrid (configs[4]): per query vector top-100 + BM25 top-100 over the same rows + RRF(k=60) -> top-10, in
        batches of 64 (device entries for both searches, fusion in libmsvs_host.so), and the BM25 scorer alone."""
        import myscaledb_amd.host as mhost
        nb = args.big_rows
        cix, mdl, npb = big["index"], big["model"], big["nprobe"]
        ps, df_all, total, n_post = build_postings(nb, 200_000)
        rng = np.random.default_rng(6)
        mids = np.argsort(-df_all)[50:2000]
        bq = 64
        qs = make_queries(mdl, 4 * bq, 4321, dev)
        v_i = torch.empty((bq, 100), device=dev, dtype=torch.int64)
        v_d = torch.empty((bq, 100), device=dev, dtype=torch.float32)
        t_i = torch.empty((bq, 100), device=dev, dtype=torch.int64)
        t_d = torch.empty((bq, 100), device=dev, dtype=torch.float32)
        sets = []
        for _ in range(4):
            terms = [rng.choice(mids, int(rng.integers(2, 5)), replace=False) for _ in range(bq)]
            dfs_ = [df_all[t] for t in terms]
            sets.append((terms, dfs_, ps.prepare_batch(terms, dfs_, total)))
        z = np.zeros(100, np.uint64)

        f_s = torch.empty((bq, 10), device=dev, dtype=torch.float32)
        f_l = torch.empty((bq, 10), device=dev, dtype=torch.int64)
        f_n = torch.empty((bq,), device=dev, dtype=torch.int32)

        side = torch.cuda.Stream(device=dev)  # the BM25 scorer (small, issue-bound kernels) runs beside the HBM-bound list scan

        def searches(i):
            terms, dfs, prep = sets[i % 4]
            side.wait_stream(torch.cuda.current_stream())
            ps.bm25_search_batch_device(terms, dfs, nb, total, 100, t_i.data_ptr(), t_d.data_ptr(), side.cuda_stream, prepared=prep)
            cix.search_device(qs[(i % 4) * bq:(i % 4 + 1) * bq].data_ptr(), bq, 100, npb, v_i.data_ptr(), v_d.data_ptr(), stream)
            torch.cuda.current_stream().wait_stream(side)

        def hybrid(i):
            """Both searches and the fusion on the device (msvs_hybrid_fuse_device), the 64 x 10 fused rows read back."""
            searches(i)
            capi.hybrid_fuse_device("rrf", v_d.data_ptr(), v_i.data_ptr(), 100, t_d.data_ptr(), t_i.data_ptr(), 100, bq, 10,
                                    f_s.data_ptr(), f_l.data_ptr(), f_n.data_ptr(), stream, fusion_k=60)
            return f_s.cpu().numpy(), f_l.cpu().numpy(), f_n.cpu().numpy()

        def hybrid_host(i):
            """The round-2 form: results to the host, fusion in libmsvs_host.so (msvs_host_hybrid_search_batch)."""
            searches(i)
            torch.cuda.synchronize()
            vi, vd, ti, td = v_i.cpu().numpy(), v_d.cpu().numpy(), t_i.cpu().numpy(), t_d.cpu().numpy()
            return mhost.hybrid_search_batch("rrf", vd, vi, td, ti, 10, fusion_k=60)  # one C++ loop over the batch
        for i in range(2):
            fused = hybrid(i)
        # the device fusion returns what the host's batched fusion and its per-query entry return
        fused_h = hybrid_host(1)
        assert fused[2].tolist() == fused_h[2].tolist() and fused[1].tolist() == fused_h[1].astype(np.int64).tolist()
        assert (fused[0].view(np.uint32) == fused_h[0].view(np.uint32)).all()
        vi0, vd0, ti0, td0 = v_i.cpu().numpy(), v_d.cpu().numpy(), t_i.cpu().numpy(), t_d.cpu().numpy()
        for qq in (0, 17, 63):
            nt = int((ti0[qq] >= 0).sum())
            s1, _, l1 = mhost.hybrid_search("rrf", (vd0[qq], z, vi0[qq].astype(np.uint64)),
                                            (td0[qq][:nt], z[:nt], ti0[qq][:nt].astype(np.uint64)), 10, fusion_k=60)
            assert l1.tolist() == fused[1][qq][:len(l1)].tolist() and s1.tolist() == fused[0][qq][:len(s1)].tolist()
        per, per_h = [], []
        for i in range(12):
            t1 = time.perf_counter()
            hybrid(i)
            per.append(time.perf_counter() - t1)
        for i in range(6):
            t1 = time.perf_counter()
            hybrid_host(i)
            per_h.append(time.perf_counter() - t1)
        dt = float(np.median(per))  # one call in ~10 takes tens of ms on the host side: median

        def bstep(i):
            terms, dfs, prep = sets[i % 4]
            ps.bm25_search_batch_device(terms, dfs, nb, total, 100, t_i.data_ptr(), t_d.data_ptr(), stream, prepared=prep)
        dtb = timed(bstep, 12)
        fb = profiled(bstep, 4, ("bm25_score",))
        byts = np.mean([sum(int(x_.sum()) * 8 + min(int(x_.sum()), nb) for x_ in dfs) for _, dfs, _ in sets])

        def bm25_leg(B, steps):
            """The BM25 scorer alone at B queries per batch (same query model): the vector side runs 4096-query steps, so does this."""
            o_i = torch.empty((B, 100), device=dev, dtype=torch.int64)
            o_d = torch.empty((B, 100), device=dev, dtype=torch.float32)
            ss = []
            for _ in range(3):
                terms = [rng.choice(mids, int(rng.integers(2, 5)), replace=False) for _ in range(B)]
                dfs_ = [df_all[t] for t in terms]
                ss.append((terms, dfs_, ps.prepare_batch(terms, dfs_, total)))

            def st(i):
                terms, dfs, prep = ss[i % 3]
                ps.bm25_search_batch_device(terms, dfs, nb, total, 100, o_i.data_ptr(), o_d.data_ptr(), stream, prepared=prep)
            for i_ in range(3):  # every query set once: the scratch arenas grow to the batch size before the clock runs
                st(i_)
            torch.cuda.synchronize()
            d_ = timed(st, steps)
            by = np.mean([sum(int(x_.sum()) * 8 + min(int(x_.sum()), nb) for x_ in dfs) for _, dfs, _ in ss])
            return {"ms_per_batch": round(d_ * 1e3, 4), "us_per_query": round(d_ / B * 1e6, 3), "qps": round(B / d_, 1),
                    "algorithmic_mb_per_batch": round(by / 1e6, 1), "gbs": round(by / d_ / 1e9, 1),
                    "hbm_frac": round(by / d_ / 1e9 / HBM_PEAK_GBS, 4)}
        bm_more = {}
        for B_, st_ in ((256, 24), (1024, 18), (4096, 9)):
            try:
                bm_more["bm25_batch%d" % B_] = bm25_leg(B_, st_)
            except Exception as e:  # (a leg must not cost the line)
                bm_more["bm25_batch%d" % B_] = {"error": repr(e)[:200]}
        q0, f0 = capi.bm25_stats()
        return {"workload": "hybrid: IVFFLAT cosine top-100 + BM25 top-100 over %d rows / documents (%d postings) + RRF k=60 -> top-10, "
                            "batches of 64" % (nb, n_post),
                "hybrid_qps": round(bq / dt, 1), "hybrid_ms_per_query": round(dt / bq * 1e3, 4),
                "hybrid_ms_per_batch_median_mean_max": [round(dt * 1e3, 3), round(float(np.mean(per)) * 1e3, 3), round(max(per) * 1e3, 3)],
                "fusion": "on the device (msvs_hybrid_fuse_device), 64 x 10 fused rows read back; == the host fusion bit for bit; the BM25 scorer runs on a second stream beside the vector search",
                "host_fusion_ms_per_batch_median": round(float(np.median(per_h)) * 1e3, 3),
                "bm25_batch64": {"ms_per_batch": round(dtb * 1e3, 4), "us_per_query": round(dtb / bq * 1e6, 2),
                                 "algorithmic_mb_per_batch": round(byts / 1e6, 1),
                                 "gbs": round(byts / dtb / 1e9, 1), "hbm_frac": round(byts / dtb / 1e9 / HBM_PEAK_GBS, 4),
                                 "score_kernels_ms": round(fb["bm25_score"], 4),
                                 "queries_fallbacks_total": [q0, f0]},
                "bm25_model": "algorithmic bytes = SURVEY 8d: 8 B per posting of the query's terms + one fieldnorm byte per touched document; "
                              "the scorer reads (doc, tf / (tf + norm)) records: 8 B per posting, no fieldnorm gather",
                **bm_more}

    if solo and "c1" not in skip:
        leg("C1", c1, other_cfg)
    if solo and not ({"c3", "c5"} <= skip):
        x = None  # the 10M-row legs want the memory
        torch.cuda.empty_cache()
        leg("C3", c3, other_cfg)
        if "c5" not in skip and "index" in big:
            leg("C5", c5, other_cfg)
        if "index" in big:
            big["index"].close()
            big.clear()
    if solo and "c4" not in skip:
        x = None
        torch.cuda.empty_cache()
        leg("C4", c4, other_cfg)
    if solo and "target" not in skip:
        x = None
        torch.cuda.empty_cache()
        leg("target_100m", target_100m, extra)

    if rank == 0:
        # the headline model's own nprobe sweep: where recall@10 >= 0.95 is first reached, and the rate there
        ops = None
        hl = extra.get(args.data)
        if isinstance(hl, dict) and "at_recall_0.95" in hl:
            a95 = hl["at_recall_0.95"]
            ops = {"model": args.data, "recall_by_nprobe": hl.get("recall_at_%d" % k),
                   "first_nprobe_with_recall_0.95": a95.get("nprobe", a95.get("chosen")), "qps_there": a95.get("qps"),
                   "ms_per_step_there": a95.get("ms_per_step"),
                   "value_is": "the rate at the configuration's nprobe = %d (recall %s)" % (nprobe, None if recall is None else round(recall, 4))}
        mid_op = None
        mm = extra.get("mid")
        if isinstance(mm, dict) and "at_recall_0.95" in mm:
            a95, a32 = mm["at_recall_0.95"], mm.get("at_config_nprobe") or mm["at_recall_0.95"]
            mid_op = {"model": "mid", "data": mm.get("data"), "recall_by_nprobe": mm.get("recall_at_%d" % k),
                      "first_nprobe_with_recall_0.95": a95.get("nprobe"),
                      "there": {f: a95.get(f) for f in ("nprobe", "qps", "ms_per_step", "roofline_frac", "whole_step_frac", "pruned_pair_fraction",
                                                        "rows_read_per_step", "union_rows_per_step", "single_query_p50_us", "single_query_p99_us", "cpu_port")},
                      "at_nprobe_32": {f: a32.get(f) for f in ("nprobe", "qps", "ms_per_step", "roofline_frac", "whole_step_frac", "pruned_pair_fraction",
                                                               "rows_read_per_step", "union_rows_per_step")}}
        out = {
            **head(),
            "recall_at_10": None if recall is None else round(recall, 4),
            "p50_ms_batch1": extra.get("latency", {}).get("p50_us", 0) / 1e3 if "latency" in extra and "p50_us" in extra["latency"] else None,
            "roofline": roof,
            "concurrent_batches": concurrent,
            "multi_gpu": multi_gpu,
            "cpu_baseline": cpu,
            "other_batches": extra.get("other_batches"),
            "latency": extra.get("latency"),
            "operating_points": dict(ops or {}, mid=mid_op) if (ops or mid_op) else None,
            "iid": extra.get("iid"),
            "blobs03": extra.get("blobs03"),
            "latent32": extra.get("latent32"),
            "mid": extra.get("mid"),
            "target_100m": extra.get("target_100m"),
            "c4_sharded": extra.get("c4_sharded"),
            "other_configs": other_cfg or None,
            "setup_s": round(setup_s, 1),
        }
        emit(out)
    if world > 1:
        comm.close()
        dist.barrier()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------------
# The driver keeps only a few KB of stdout: the ONE JSON line it parses is a compact digest (<= 6 KB) -- the contract's keys, the
# roofline / cpu_baseline objects without prose, and ONE or two numbers per leg.  The full object (every leg, every note) goes to
# bench_detail.json beside bench.py (+ gpurun_out/ when present) and to stderr.
LINE_BUDGET = 6000


def _g(o, *path, default=None):
    for p_ in path:
        if not isinstance(o, dict) or p_ not in o:
            return default
        o = o[p_]
    return o


def _pick(o, *names):
    return {n_: o[n_] for n_ in names if isinstance(o, dict) and o.get(n_) is not None} or None


def compact_line(out):
    """The driver-facing digest of the full bench object `out` (see main()): numbers only, no prose."""
    roof = out.get("roofline") or {}
    cpu = out.get("cpu_baseline") or {}
    cfg = out.get("config") or {}
    line = {k_: out.get(k_) for k_ in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                       "scaling", "vs_baseline", "dtype", "data")}
    line["config"] = {"workload": cfg.get("workload"), **{k_: cfg.get(k_) for k_ in ("rows", "dim", "nlist", "nprobe", "k", "batch", "streams")},
                      "parallelism": (cfg.get("parallelism") or "")[:48], "data_model": (cfg.get("data_model") or "")[:40]}
    line["recall_at_10"] = out.get("recall_at_10")
    line["p50_ms_batch1"] = out.get("p50_ms_batch1")
    line["roofline"] = {k_: roof.get(k_) for k_ in ("bound", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "launches_per_step",
                                                     "bytes_per_launch", "whole_step_frac", "non_scan_ms_per_step", "pruned_pair_fraction")}
    line["roofline"]["kernel"] = (roof.get("kernel") or "").split(" (")[0]
    line["cpu_baseline"] = {"value": cpu.get("value"), "unit": cpu.get("unit"), "cores": cpu.get("cores"), "kind": cpu.get("kind"),
                            "sample": (cpu.get("sample") or "")[:60],
                            "oracle_bit_identical": _g(cpu, "oracle_check", "ids_and_distances_bit_identical")}
    legs = {}
    ob = out.get("other_batches")
    if isinstance(ob, dict):
        legs["other_batches_qps"] = {b_: v_.get("qps") for b_, v_ in ob.items() if isinstance(v_, dict)}
    cb = out.get("concurrent_batches")
    if cb:
        legs["concurrent_batches"] = _pick(cb, "streams", "qps", "ms_per_step")
    lat = out.get("latency")
    if isinstance(lat, dict):
        legs["latency"] = {"p50_us": lat.get("p50_us"), "p99_us": lat.get("p99_us"),
                           "threads_64_qps": _g(lat, "threads_64", "qps"), "threads_64_p50_us": _g(lat, "threads_64", "p50_us"),
                           "batch32_us_per_call": _g(lat, "host_pointer_small_batches", "32", "us_per_call"),
                           "batch4096_host_qps": _g(lat, "host_pointer_batch4096", "qps")}
    for m_ in ("iid", "blobs03", "latent32", "mid"):
        v_ = out.get(m_)
        if not isinstance(v_, dict):
            continue
        e_ = {}
        for pt in ("at_recall_0.95", "at_config_nprobe"):
            if isinstance(v_.get(pt), dict):
                e_[pt] = _pick(v_[pt], "nprobe", "chosen", "recall", "qps", "ms_per_step", "roofline_frac", "whole_step_frac", "whole_step_mfma_frac",
                               "pruned_pair_fraction")
        if m_ == "iid":
            e_["exhaustive_flat"] = _pick(v_.get("exhaustive_flat"), "recall", "qps", "ms_per_step", "whole_step_mfma_frac", "kernel_mfma_frac")
            e_["flat_latency"] = _pick(v_.get("flat_latency"), "p50_us", "p99_us", "recall", "hbm_frac_of_p50")
            e_.pop("at_recall_0.95", None)  # (== exhaustive_flat)
        if "error" in v_:
            e_["error"] = str(v_["error"])[:80]
        legs[m_] = e_
    t_ = out.get("target_100m")
    if isinstance(t_, dict):
        legs["target_100m"] = {"recall_at_10": t_.get("recall_at_10"),
                               "batches": {b_: _pick(v_, "qps", "ms_per_batch", "roofline_frac", "whole_step_frac")
                                           for b_, v_ in (t_.get("batches") or {}).items()},
                               "oracle_bit_identical": _g(t_, "oracle_check", "ids_and_distances_bit_identical"),
                               "cpu_baseline": _pick(t_.get("cpu_baseline"), "value", "unit", "cores", "kind"),
                               "gpu_over_cpu_best": _g(t_, "gpu_over_cpu", "best"), **({"error": str(t_["error"])[:80]} if "error" in t_ else {})}
    oc = out.get("other_configs") or {}
    if isinstance(oc.get("C1"), dict):
        c_ = oc["C1"]
        legs["C1"] = {"knn_host_call_p50_us": c_.get("knn_host_call_p50_us"), "resident_nq1_us": _g(c_, "resident_nq1", "us_per_call"),
                      "resident_nq1000_qps": _g(c_, "resident_nq1000", "qps"), "cpu_qps_1core": _g(c_, "cpu_baseline", "value"),
                      **({"error": str(c_["error"])[:80]} if "error" in c_ else {})}
    if isinstance(oc.get("C3"), dict):
        c_ = oc["C3"]
        legs["C3"] = dict(_pick(c_, "qps", "ms_per_batch", "roofline_frac", "whole_step_frac", "error") or {},
                          cpu_qps=_g(c_, "cpu_baseline", "value"), cpu_cores=_g(c_, "cpu_baseline", "cores"))
    if isinstance(oc.get("C4"), dict):
        c_ = oc["C4"]
        legs["C4"] = {"batches": {b_: _pick(v_, "qps", "ms_per_batch", "roofline_frac", "whole_step_frac")
                                  for b_, v_ in (c_.get("batches") or {}).items() if isinstance(v_, dict)},
                      "oracle_bit_identical": _g(c_, "oracle_check", "ids_and_distances_bit_identical"),
                      **({"error": str(c_["error"])[:80]} if "error" in c_ else {})}
    if isinstance(oc.get("C5"), dict):
        c_ = oc["C5"]
        legs["C5"] = {"hybrid_qps": c_.get("hybrid_qps"),
                      **{b_: _pick(c_.get(b_), "ms_per_batch", "us_per_query", "hbm_frac") for b_ in ("bm25_batch64", "bm25_batch1024", "bm25_batch4096")
                         if isinstance(c_.get(b_), dict)},
                      **({"error": str(c_["error"])[:80]} if "error" in c_ else {})}
    mg = out.get("multi_gpu")
    if isinstance(mg, dict):
        legs["multi_gpu"] = {"mode": mg.get("mode"),
                             "routed": _pick(mg.get("routed"), "queries_per_step_per_rank", "routed_pairs_per_step_by_rank", "qps", "stage_ms_rank0"),
                             "replicated": _pick(mg.get("replicated"), "qps", "ms_per_step")}
    cs = out.get("c4_sharded")
    if isinstance(cs, dict):
        legs["c4_sharded"] = {"rows_on_rank0": cs.get("rows_on_rank0"), "scaling": cs.get("scaling"),
                              "batches": cs.get("batches"), **({"error": str(cs["error"])[:80]} if "error" in cs else {})}
    line["legs"] = legs
    line["setup_s"] = out.get("setup_s")
    line["detail"] = "bench_detail.json"
    s_ = json.dumps(line, separators=(",", ":"))
    # never let a leg cost the line: shed the widest legs until the digest fits
    while len(s_) > LINE_BUDGET and legs:
        widest = max(legs, key=lambda k_: len(json.dumps(legs[k_])))
        legs[widest] = "see bench_detail.json"
        if all(isinstance(v_, str) for v_ in legs.values()):
            line["legs"] = legs = {}
        s_ = json.dumps(line, separators=(",", ":"))
    return s_


def emit(out):
    """Full object -> bench_detail.json (+ gpurun_out/, stderr); compact digest -> the ONE stdout line."""
    full = json.dumps(out)
    for path in (os.path.join(ROOT, "bench_detail.json"), os.path.join(ROOT, "gpurun_out", "bench_detail.json")):
        try:
            if os.path.isdir(os.path.dirname(path)):
                with open(path, "w") as f:
                    f.write(full + "\n")
        except OSError:
            pass
    sys.stderr.write("bench detail: " + full + "\n")
    sys.stderr.flush()
    print(compact_line(out), flush=True)


if __name__ == "__main__":
    main()
