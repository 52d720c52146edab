"""The graph index on one GPU: --rows x --dim rows of one of bench.py's data models (--data mid | iid | blobs03) in a device row
store, a built index of degree --degree, searched through the device entry on one stream.  Reports, gates nothing.

  - the build's wall time (msvs_graph_index_build as a whole: trainer, lists, prune, reverse edges), printed as soon as it is known;
    --join-iters T >= 1 selects the sub-quadratic build (IVF lists of --build-nprobe lists, T join iterations over --join-sample entries);
  - for nq in --batches and ef in --efs: recall@10 against an exact scan of the rows (torch, on the first 256 queries), the median
    time of --reps calls between HIP events after a warm-up call (and their spread, min .. max), queries/s;
  - --bits 32,8,16: the index is built once at 32 bits, exported, and the same structure is handed (set_graph) to a bit_size=8 and a
    bit_size=16 index over the same store, so all forms search one graph; their repetitions alternate inside one process, shape by shape;
    pq8:M / pq4:M add product-quantised forms (pq_m=M, 8- or 4-bit codes) over the same graph, and for each the recall@10 of
    search(k = 100) + refine against the store and the time of a max_iters=1 search beside the whole one (the table build's share);
  - beside them the IVFFLAT index of the same rows (nlist --nlist) at --nprobes, the same way, to read the nprobe of equal recall off;
  - --wide: the wide search (search_wide_device) against search_device at ef 64 and 256, its own range (--wide-efs) and filtered
    searches with --alive of the rows alive (wide_section).

Writes one JSON file (default profiles/graph.json) and prints it.

    python -m tools.bench_graph [--rows N] [--dim D] [--data mid] [--degree 32] [--nlist 1024] [--batches 1,64,4096] [--efs 32,64,128,256]
                                [--bits 32,8,16] [--nprobes 8,16,32,64] [--join-iters T] [--build-nprobe P] [--join-sample S] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import myscaledb_amd.capi as capi  # noqa: E402


def wide_section(a, gx, x, q, batches, timed_all, stream):
    """--wide: search_wide_device beside search_device on the 32-bit index (repetitions alternating), the range only it reaches
    (--wide-efs at the batches >= 64: recall@10, and recall@1000 with k = 1000), and filtered searches (--alive fractions, k = 10)."""
    import torch
    dev, nt = x.device, min(256, len(q))

    def exact(k, alive=None):
        best = torch.full((nt, k), float("inf"), device=dev)
        best_i = torch.full((nt, k), -1, device=dev, dtype=torch.int64)
        for r0 in range(0, a.rows, 1 << 16):
            d2 = (torch.cdist(q[:nt].double(), x[r0:r0 + (1 << 16)].double()) ** 2).float()
            if alive is not None:
                d2[:, ~alive[r0:r0 + (1 << 16)]] = float("inf")
            cat_i = torch.cat([best_i, torch.arange(r0, r0 + d2.shape[1], device=dev).expand(nt, -1)], 1)
            best, sel = torch.topk(torch.cat([best, d2], 1), k, dim=1, largest=False)
            best_i = torch.gather(cat_i, 1, sel)
        return [set(r[np.isfinite(d)].tolist()) for r, d in zip(best_i.cpu().numpy(), best.cpu().numpy())]

    def recall(truth, ids):
        return float(np.mean([len(t & set(g.tolist())) / max(len(t), 1) for t, g in zip(truth, ids[:nt])]))

    def run(fn, b, k, ef, **kw):
        di = torch.empty((b, k), device=dev, dtype=torch.int64)
        dd = torch.empty((b, k), device=dev, dtype=torch.float32)
        return di, lambda: fn(q.data_ptr(), b, k, di.data_ptr(), dd.data_ptr(), ef=ef, stream=stream, **kw)

    def row(name, b, k, ef, ms, **more):
        med = float(np.median(ms))
        return dict({"entry": name, "nq": b, "k": k, "ef": ef, "ms": med, "ms_min": min(ms), "ms_max": max(ms), "qps": b / med * 1e3}, **more)

    res, truth = {"cost": [], "range": [], "filtered": []}, {10: exact(10), 1000: exact(1000)}
    for b in batches:
        for ef in (64, 256):
            (dn, narrow), (dw, wide) = run(gx.search_device, b, 10, ef), run(gx.search_wide_device, b, 10, ef)
            ms = timed_all([narrow, wide])
            same = bool((dn == dw).all())
            res["cost"] += [row("search", b, 10, ef, ms[0]), row("search_wide", b, 10, ef, ms[1], equal_ids=same)]
    for b in (b for b in batches if b >= 64):
        for ef in (int(v) for v in a.wide_efs.split(",")):
            for k in (10, 1000):
                if k <= ef:
                    di, call = run(gx.search_wide_device, b, k, ef)
                    ms = timed_all([call])[0]
                    res["range"].append(row("search_wide", b, k, ef, ms, recall=recall(truth[k], di.cpu().numpy()) if b >= nt else None))
    b = max(batches)
    for frac in (float(v) for v in a.alive.split(",")):
        alive = torch.rand(a.rows, device=dev, generator=torch.Generator(dev).manual_seed(7)) < frac
        bits = torch.from_numpy(capi.pack_bits(alive.cpu().numpy()).view(np.int64)).to(dev)
        t = exact(10, alive)
        for name, fn, ef in [("search", gx.search_device, 256)] + [("search_wide", gx.search_wide_device, int(v)) for v in a.wide_efs.split(",")]:
            di, call = run(fn, b, 10, ef, d_alive=bits.data_ptr(), nbits=a.rows)
            ms = timed_all([call])[0]
            ids = di.cpu().numpy()
            res["filtered"].append(row(name, b, 10, ef, ms, alive=frac, filled=float((ids >= 0).mean()), recall=recall(t, ids) if b >= nt else None))
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="also measure search_wide_device (the 32-bit index): see wide_section")
    ap.add_argument("--wide-efs", default="512,1024,4096")
    ap.add_argument("--alive", default="0.05,0.01", help="--wide: the alive fractions of its filtered searches")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--data", default="mid", choices=("mid", "iid", "blobs03"))
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--efs", default="32,64,128,256")
    ap.add_argument("--bits", default="32", help="forms of the graph index to search: 32, 16, 8, pq8:M, pq4:M (product-quantised, M sub-quantisers)")
    ap.add_argument("--pq-iters", type=int, default=10, help="k-means iterations of the product-quantised forms' codebooks")
    ap.add_argument("--nprobes", default="8,16,32,64", help="of the IVFFLAT index beside it; empty: leave it out")
    ap.add_argument("--join-iters", type=int, default=0, help="0: the exact O(n^2) build; >= 1: IVF lists repaired by the join kernel")
    ap.add_argument("--build-nprobe", type=int, default=8)
    ap.add_argument("--join-sample", type=int, default=8)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join("profiles", "graph.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph needs a GPU: there is nothing to measure without one")
    capi.set_device(0)
    dev = torch.device("cuda", 0)
    batches = [int(v) for v in a.batches.split(",")]
    nq, k = max(batches), 10
    x, q, what = bench.data_model(a.data, a.rows, nq, a.dim, dev)
    x, q = x.contiguous(), q.contiguous()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    nt = min(256, nq)  # the exact answer, by chunks of rows
    best = torch.full((nt, k), float("inf"), device=dev)
    best_i = torch.zeros((nt, k), device=dev, dtype=torch.int64)
    for r0 in range(0, a.rows, 1 << 16):
        d2 = torch.cdist(q[:nt].double(), x[r0:r0 + (1 << 16)].double()) ** 2
        cat_d = torch.cat([best, d2.float()], 1)
        cat_i = torch.cat([best_i, torch.arange(r0, r0 + d2.shape[1], device=dev).expand(nt, -1)], 1)
        best, sel = torch.topk(cat_d, k, dim=1, largest=False)
        best_i = torch.gather(cat_i, 1, sel)
    truth = best_i.cpu().numpy()

    def recall(ids):
        return float(np.mean([len(set(t.tolist()) & set(g.tolist())) / k for t, g in zip(truth, ids[:nt])]))

    di = torch.empty((nq, k), device=dev, dtype=torch.int64)
    dd = torch.empty((nq, k), device=dev, dtype=torch.float32)

    def timed_all(calls):
        """the calls take turns, repetition by repetition -> [ms of every repetition] per call"""
        for call in calls:
            call()  # warm-up: arenas, the kernel's attribute
        torch.cuda.synchronize()
        ms = [[] for _ in calls]
        for _ in range(a.reps):
            for i, call in enumerate(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                ms[i].append(e0.elapsed_time(e1))
        return ms

    def timed(call):
        return float(np.median(timed_all([call])[0]))

    out = {"data": what, "rows": a.rows, "dim": a.dim, "degree": a.degree, "nlist": a.nlist, "graph": [], "ivfflat": []}
    rows = capi.Rows(a.dim, a.rows)
    rows.append(x.data_ptr(), n=a.rows, mem=capi.MEM_DEVICE)
    build = "join_iters=%d,build_nprobe=%d,join_sample=%d" % (a.join_iters, a.build_nprobe, a.join_sample)
    gx = capi.GraphIndex(capi.METRIC_L2, rows, "degree=%d,ncentroids=%d,kmeans_iters=10,%s" % (a.degree, a.nlist, build))
    t0 = time.perf_counter()
    gx.build()
    out["build"], out["build_s"] = build, time.perf_counter() - t0
    print("build (%s): %.2f s" % (build, out["build_s"]), flush=True)
    forms = {32: gx}
    bits = [int(v) if v.isdigit() else v for v in a.bits.split(",")]
    for b in (b for b in (8, 16) if b in bits):
        t0 = time.perf_counter()
        forms[b] = capi.GraphIndex(capi.METRIC_L2, rows, "degree=%d,bit_size=%d" % (a.degree, b))
        forms[b].set_graph(*gx.export())
        out["encode_s" if b == 8 else "encode_h16_s"] = time.perf_counter() - t0  # (with the structure's round trip through the host)
    for f in (f for f in bits if isinstance(f, str)):  # pq8:M / pq4:M: codebooks trained over the store, codes, the same graph
        width, m = f[2:].split(":")
        t0 = time.perf_counter()
        forms[f] = capi.GraphIndex(capi.METRIC_L2, rows, "degree=%d,pq_m=%s,bit_size=%s,kmeans_iters=%d" % (a.degree, m, width, a.pq_iters))
        forms[f].set_graph(*gx.export())
        out.setdefault("pq_encode_s", {})[f] = time.perf_counter() - t0
    forms = {b: forms[b] for b in bits}
    out["graph_bytes"] = {str(b): ix.memory_usage for b, ix in forms.items()}
    out["row_bytes"] = {str(b): rows.memory_usage if b == 32 else 0 for b in forms}  # what the search needs resident besides
    out["pq"] = []
    for f, ix in ((f, ix) for f, ix in forms.items() if isinstance(f, str)):
        # the two-stage search: search(k = 100) + refine against the store, recall@10; and the table build's share of the kernel:
        # max_iters = 1 (tables, seeds, one expansion) against the whole search at ef = 64
        d100 = torch.empty((nt, 100), device=dev, dtype=torch.int64)
        s100 = torch.empty((nt, 100), device=dev, dtype=torch.float32)
        for ef in (int(v) for v in a.efs.split(",")):
            try:
                ix.search_device(q.data_ptr(), nt, 100, d100.data_ptr(), s100.data_ptr(), ef=max(ef, 100), stream=stream)
            except capi.MsvsError as e:
                out["pq"].append({"bits": f, "ef": max(ef, 100), "refused": str(e)})
                continue
            capi.refine_device(rows, capi.METRIC_L2, q.data_ptr(), nt, d100.data_ptr(), 100, k, di.data_ptr(), dd.data_ptr(), stream)
            torch.cuda.synchronize()
            out["pq"].append({"bits": f, "ef": max(ef, 100), "refined_recall@10": recall(di[:nt].cpu().numpy())})
        b = max(batches)
        one, full = timed_all([lambda: ix.search_device(q.data_ptr(), b, k, di.data_ptr(), dd.data_ptr(), ef=64, max_iters=1, stream=stream),
                               lambda: ix.search_device(q.data_ptr(), b, k, di.data_ptr(), dd.data_ptr(), ef=64, stream=stream)])
        out["pq"].append({"bits": f, "nq": b, "ef": 64, "ms_max_iters_1": float(np.median(one)), "ms": float(np.median(full)),
                          "table_share_at_most": float(np.median(one) / np.median(full))})
    for b in batches:
        for ef in (int(v) for v in a.efs.split(",")):
            outs = {f: (torch.empty_like(di), torch.empty_like(dd)) for f in forms}
            calls = {f: (lambda f=f, ix=ix: ix.search_device(q.data_ptr(), b, k, outs[f][0].data_ptr(), outs[f][1].data_ptr(), ef=ef, stream=stream))
                     for f, ix in forms.items()}
            for f in list(calls):  # a form whose LDS image does not fit this ef (pq8:96 at ef = 128) is reported as refused
                try:
                    calls[f]()
                except capi.MsvsError as e:
                    out["graph"].append({"bits": f, "nq": b, "ef": ef, "refused": str(e)})
                    del calls[f]
            for f, ms in zip(calls, timed_all(list(calls.values()))):
                med = float(np.median(ms))
                out["graph"].append({"bits": f, "nq": b, "ef": ef, "ms": med, "ms_min": min(ms), "ms_max": max(ms), "qps": b / med * 1e3,
                                     "recall@10": recall(outs[f][0].cpu().numpy()) if b >= nt else None})
    if a.wide:
        out["wide"] = wide_section(a, gx, x, q, batches, timed_all, stream)
    for ix in forms.values():
        ix.close()
    if 32 not in forms:
        gx.close()
    if a.nprobes:
        ivf = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, a.dim, "ncentroids=%d,kmeans_iters=10" % a.nlist)
        ivf.train(x.data_ptr(), n=a.rows, mem=capi.MEM_DEVICE)
        ivf.add(x.data_ptr(), n=a.rows, mem=capi.MEM_DEVICE)
        ivf.build()
    for b in batches if a.nprobes else ():
        for p in (int(v) for v in a.nprobes.split(",")):
            ms = timed(lambda: ivf.search_device(q.data_ptr(), b, k, p, di.data_ptr(), dd.data_ptr(), stream))
            out["ivfflat"].append({"nq": b, "nprobe": p, "ms": ms, "qps": b / ms * 1e3, "recall@10": recall(di.cpu().numpy()) if b >= nt else None})
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
