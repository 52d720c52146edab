"""The two-stage search on one GPU: 1M x 768 rows in blobs (sigma 0.3), nlist 1024, L2, an IVFPQ index (m = 96) beside a row store
of the same rows, against the default IVFFLAT index of the same rows (the same trainer on the same rows and parameters: the same
lists).  Everything runs in one process and one call; every timed shape is warmed up first, the times are HIP events around calls
of the device entries on one stream (median of --reps), and the legs that are compared alternate.

  - the refine launch alone (msvs_refine_device over the first stage's own candidates): --batch queries, kc candidates, k results,
    the device store and the pinned store alternating; its time against the bound of nq * kc * ld * 4 algorithmic bytes at the HBM
    spec rate (8 TB/s) for the device store and at the PCIe Gen5 x16 spec rate (63 GB/s) for the pinned one (rows that several
    queries share are counted once per query: a share above 1 is cache hits, not a faster bus); 1 and 32 queries as latencies;
  - the whole two-stage step: search_refine_device(k, kc) of the PQ index over either store beside search_device(k) of the IVFFLAT
    index and the PQ index's own first stage at k and at kc, same nprobe; recall@k of each against an exact scan of the rows on
    the first 256 queries;
  - first stages beyond 256 candidates (--kcs, default 256, 512 and 1024): search_rounds_device(kc) alone and
    search_refine_rounds_device(k, kc) over the device store, with the recall@k of the latter;
  - device bytes (memory_usage) of the three configurations: PQ + device rows, PQ + pinned rows, IVFFLAT.

Writes one JSON file (default profiles/refine.json) and prints it.

    python -m tools.bench_refine [--rows N] [--dim D] [--nlist L] [--m M] [--batch 4096] [--nprobe P] [--k 10] [--kc 100] [--reps R]
                                 [--kcs 256,512,1024] [--no-pinned] [--query-tables] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import myscaledb_amd.capi as capi  # noqa: E402
from tools.bench_pq_ivf import built, data  # noqa: E402

F = np.float32
HBM_BYTES_PER_S = 8.0e12   # HBM3E spec
PCIE_BYTES_PER_S = 63.0e9  # PCIe Gen5 x16 spec


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--kc", type=int, default=100)
    ap.add_argument("--kcs", default="256,512,1024", help="first stages in rank rounds (search_rounds_device), comma separated; empty: none")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-pinned", action="store_true", help="leave the pinned store out")
    ap.add_argument("--query-tables", action="store_true", help="the PQ index in the query-table form (query_tables=1)")
    ap.add_argument("--out", default=os.path.join("profiles", "refine.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine needs a GPU: there is nothing to measure without one")
    capi.set_device(0)
    dev = torch.device("cuda", 0)
    nq, k, kc = a.batch, a.k, a.kc
    x, q = data(a, nq)
    params = "ncentroids=%d,kmeans_iters=4,train_sample=%d" % (a.nlist, min(a.rows, 64 * a.nlist))
    pq, _ = built(lambda: capi.PqIndex(capi.METRIC_L2, a.dim, params + ",m=%d" % a.m + (",query_tables=1" if a.query_tables else "")), x, a)
    flat, _ = built(lambda: capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, a.dim, params), x, a)
    stores = {"device": capi.Rows(a.dim, a.rows)}
    if not a.no_pinned:
        stores["pinned"] = capi.Rows(a.dim, a.rows, placement=capi.ROWS_HOST_PINNED)
    for rows in stores.values():
        for b in range(0, a.rows, 1 << 17):
            rows.append(x[b:b + (1 << 17)])
    sys.stderr.write("row stores filled\n")
    nt = min(nq, 256)
    truth, _ = capi.knn(q[:nt], x, k, capi.METRIC_L2)

    stream = torch.cuda.current_stream().cuda_stream
    dq = torch.from_numpy(q).to(dev)
    d_cand = torch.empty((nq, kc), device=dev, dtype=torch.int64)
    d_cdis = torch.empty((nq, kc), device=dev, dtype=torch.float32)
    d_ids = torch.empty((nq, k), device=dev, dtype=torch.int64)
    d_dis = torch.empty((nq, k), device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    pq.search_device(dq.data_ptr(), nq, kc, a.nprobe, d_cand.data_ptr(), d_cdis.data_ptr(), stream)  # the refine legs' candidates
    torch.cuda.synchronize()

    def timed(legs, reps):
        """legs: name -> callable that enqueues on the stream; -> name -> the per-call milliseconds, the legs alternating"""
        for _ in range(2):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {n: [] for n in legs}
        for _ in range(reps):
            for n, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        return ms

    def summary(ms):
        return {n: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v))} for n, v in ms.items()}

    ld = (a.dim + 3) // 4 * 4
    out = {"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "m": a.m, "nprobe": a.nprobe, "k": k, "kc": kc, "metric": "L2", "reps": a.reps, "query_tables": int(a.query_tables),
           "version": capi.version(), "refine_alone": {}}
    for n in sorted({nq, 32, 1}, reverse=True):
        legs = {name: (lambda rows: lambda: capi.refine_device(rows, capi.METRIC_L2, dq.data_ptr(), n, d_cand.data_ptr(), kc, k, d_ids.data_ptr(),
                                                               d_dis.data_ptr(), stream))(rows) for name, rows in stores.items()}
        res = summary(timed(legs, a.reps))
        algo = n * kc * ld * 4
        for name, r in res.items():
            bound_ms = 1e3 * algo / (HBM_BYTES_PER_S if name == "device" else PCIE_BYTES_PER_S)
            r.update(algorithmic_bytes=algo, bound_ms=bound_ms, share_of_bound=bound_ms / r["ms_median"], bound="HBM 8 TB/s spec" if name == "device" else "PCIe 63 GB/s spec")
        out["refine_alone"][str(n)] = res

    def recall(ids):
        return float(np.mean([len(set(truth[i].tolist()) & set(ids[i][:k].tolist())) / k for i in range(nt)]))

    legs, results = {}, {}
    for name, rows in stores.items():
        legs["pq_search_refine_" + name] = (lambda rows: lambda: pq.search_refine_device(rows, dq.data_ptr(), nq, k, kc, a.nprobe, d_ids.data_ptr(),
                                                                                        d_dis.data_ptr(), stream))(rows)
    legs["ivfflat_search"] = lambda: flat.search_device(dq.data_ptr(), nq, k, a.nprobe, d_ids.data_ptr(), d_dis.data_ptr(), stream)
    legs["pq_first_stage_k"] = lambda: pq.search_device(dq.data_ptr(), nq, k, a.nprobe, d_ids.data_ptr(), d_dis.data_ptr(), stream)
    legs["pq_first_stage_kc"] = lambda: pq.search_device(dq.data_ptr(), nq, kc, a.nprobe, d_cand.data_ptr(), d_cdis.data_ptr(), stream)
    for n, fn in legs.items():
        if n == "pq_first_stage_kc":
            continue
        fn()
        torch.cuda.synchronize()
        results[n] = d_ids.cpu().numpy()
    out["two_stage"] = {"queries": nq, "times": summary(timed(legs, a.reps)), "recall_at_k": {n: recall(r) for n, r in results.items()}}
    if "pinned" in stores:
        out["two_stage"]["device_and_pinned_agree"] = bool((results["pq_search_refine_device"] == results["pq_search_refine_pinned"]).all())
    # first stages beyond one round of 256 ranks (search_rounds_device: the list scan once per 256 ranks, coarse step and plan once):
    # the first stage alone and the whole step over the device store at every kc of --kcs, recall@k of the whole step
    kcs = [int(v) for v in a.kcs.split(",") if v]
    if kcs:
        d_cand2 = torch.empty((nq, max(kcs)), device=dev, dtype=torch.int64)
        d_cdis2 = torch.empty((nq, max(kcs)), device=dev, dtype=torch.float32)
        legs, results = {}, {}
        for c in kcs:
            legs["pq_first_stage_rounds_kc%d" % c] = (lambda c: lambda: pq.search_rounds_device(dq.data_ptr(), nq, c, a.nprobe, d_cand2.data_ptr(),
                                                                                                d_cdis2.data_ptr(), stream))(c)
            legs["pq_search_refine_rounds_device_kc%d" % c] = (lambda c: lambda: pq.search_refine_rounds_device(
                stores["device"], dq.data_ptr(), nq, k, c, a.nprobe, d_ids.data_ptr(), d_dis.data_ptr(), stream))(c)
        for n, fn in legs.items():
            if "refine" in n:
                fn()
                torch.cuda.synchronize()
                results[n] = d_ids.cpu().numpy()
        out["large_first_stage"] = {"queries": nq, "kcs": kcs, "times": summary(timed(legs, a.reps)),
                                    "recall_at_k": {n: recall(r) for n, r in results.items()}}
    out["device_bytes"] = {"pq": pq.memory_usage, "ivfflat": flat.memory_usage,
                           "pq_plus_rows_" + "device": pq.memory_usage + stores["device"].memory_usage}
    if "pinned" in stores:
        out["device_bytes"]["pq_plus_rows_pinned"] = pq.memory_usage + stores["pinned"].memory_usage
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
