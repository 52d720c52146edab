"""IVFSQ against IVFFLAT on one GPU: 1M x 768 rows in blobs (sigma 0.3), nlist 1024, L2, k 10, nprobe 32, batches of 64, 1024 and
4096 queries.  The competitors are the IVFFLAT index of the same rows and centroids, once with its default shadow and once with
shadow=0, and that one again with the candidate pass and the probe pruning switched off (ivfflat_canonical: the same canonical
arithmetic on 4x the bytes).  Whole calls by the host clock around calls that end in a stream
synchronisation, after warm-up, the four alternating; the scan kernels by HIP events (msvs_profile_*) in a pass of its own;
recall@10 of each against an exact scan of the original rows.  Every batch size runs in a child process of its own under a time
limit, and the run stops at the first child that fails.  Writes one JSON file (default profiles/sq_ivf.json).

--bit-size takes the code widths of the SQ indexes to build from the same rows, 8 (named sq), 4 (sq4) and 16 (sq16), as a list:
every one is timed, alternating with the others, and a 4-bit index is also searched through search_refine at kc = 50 and 100 over
a row store of the original rows (recall only).  --competitors 0 leaves the IVFFLAT indexes out.

    python -m tools.bench_sq_ivf [--rows N] [--dim D] [--nlist L] [--batches 64,1024,4096] [--nprobe P] [--k K] [--reps R] [--out FILE]
                                 [--bit-size 8,4,16] [--competitors 0]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myscaledb_amd.capi as capi  # noqa: E402

F = np.float32


def blobs(rng, centres, n):
    out = np.empty((n, centres.shape[1]), F)
    for b in range(0, n, 1 << 16):
        m = min(1 << 16, n - b)
        out[b:b + m] = centres[rng.integers(0, len(centres), m)] + F(0.3) * rng.standard_normal((m, centres.shape[1]), dtype=F)
    return out


def streamed_rows(q, cent, lens, nprobe, nlist):
    """rows the list scan of the SQ index streams: sum over lists of ceil(pairs / T) * len, with sq_index.hip's choice of T (k = 10
    fits every tile) and the probe lists recomputed here in float64 (the boundary probes may differ from the canonical ones)."""
    d = (q.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * q.astype(np.float64) @ cent.T.astype(np.float64) + (cent.astype(np.float64) ** 2).sum(1)[None, :]
    probes = np.argsort(d, axis=1)[:, :nprobe]
    pairs = np.bincount(probes.ravel(), minlength=nlist)
    n_pairs = probes.size
    T = 8 if n_pairs >= 16 * nlist else (4 if n_pairs >= 2 * nlist else 2)
    return int((-(-pairs // T) * lens).sum()), int((pairs * lens).sum()), T


def sq_name(bits):
    return "sq" if bits == 8 else "sq%d" % bits


def child(a, nq):
    capi.set_device(0)
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((a.nlist, a.dim), dtype=F)
    x = blobs(rng, centres, a.rows)
    q = blobs(rng, centres, nq)
    params = "ncentroids=%d,kmeans_iters=4,train_sample=%d" % (a.nlist, min(a.rows, 64 * a.nlist))
    widths = [int(v) for v in a.bit_size.split(",")]
    sqs, t_build = {}, {}
    for bits in widths:
        name = sq_name(bits)
        sq = capi.SqIndex(capi.METRIC_L2, a.dim, params if bits == 8 else params + ",bit_size=%d" % bits)  # (8: created as it always was)
        t0 = time.perf_counter()
        sq.train(x[::max(1, a.rows // (128 * a.nlist))])
        for b in range(0, a.rows, 1 << 17):
            sq.add(x[b:b + (1 << 17)], np.arange(b, min(a.rows, b + (1 << 17)), dtype=np.int64))
        sq.build()
        t_build[name] = time.perf_counter() - t0
        sqs[name] = sq
    sq = sqs[sq_name(widths[0])]  # (the same seed and training rows: the same centroids and lists at every width)
    cent = sq.export(with_lists=False)[0]
    off = np.empty(a.nlist + 1, np.int64)
    capi._check(capi.lib().msvs_sq_index_export(sq._h, None, None, None, capi._p(off, capi.C.c_int64), None, None))
    flats = {}
    for name, shadow in (("ivfflat_shadow", ""), ("ivfflat_f32", ",shadow=0")) if a.competitors else ():
        ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, a.dim, "ncentroids=%d%s" % (a.nlist, shadow))
        ix.set_centroids(cent)
        for b in range(0, a.rows, 1 << 17):
            ix.add(x[b:b + (1 << 17)], np.arange(b, min(a.rows, b + (1 << 17)), dtype=np.int64))
        ix.build()
        flats[name] = ix
    sp = "nprobe=%d" % a.nprobe
    runs = {name: (lambda ix: lambda: ix.search(q, a.k, sp))(ix) for name, ix in sqs.items()}
    for name, ix in flats.items():
        runs[name] = (lambda ix: lambda: ix.search(q, a.k, sp))(ix)

    def canonical():
        """the shadow=0 index through the canonical batched list scan alone: no candidate pass, no probe pruning"""
        capi.set_option("ivf_pass", 0)
        capi.set_option("h16_preprune", 0)
        try:
            return flats["ivfflat_f32"].search(q, a.k, sp)
        finally:
            capi.set_option("ivf_pass")
            capi.set_option("h16_preprune")

    if a.competitors:
        runs["ivfflat_canonical"] = canonical
    results = {name: fn() for name, fn in runs.items()}
    for _ in range(2):  # warm-up of every shape
        for fn in runs.values():
            fn()
    times = {name: [] for name in runs}
    for _ in range(a.reps):  # alternating: other work shares the host
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    kern = {}
    for name, fn in runs.items():  # kernel families by HIP events, in a pass of its own
        capi.profile_enable(True)
        capi.profile_reset()
        fn()
        fams = ("sq_ivf_scan", "ivf_scan", "ivf_plan", "flat_scan", "merge", "coarse_pass")
        kern[name] = {f: dict(zip(("calls", "ms"), capi.profile_get(f))) for f in fams}
        capi.profile_enable(False)
    nt = min(nq, 256)
    truth, _ = capi.knn(q[:nt], x, a.k, capi.METRIC_L2)

    def recall_of(ids):
        return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / a.k for i in range(nt)]))

    recall = {name: recall_of(r[0]) for name, r in results.items()}
    if "sq4" in sqs:  # the 4-bit index as a first stage: the exact re-rank of its kc best over the original rows
        store = capi.Rows(a.dim, a.rows)
        for b in range(0, a.rows, 1 << 17):
            store.append(x[b:b + (1 << 17)])
        for kc in (50, 100):
            recall["sq4_refine_kc%d" % kc] = recall_of(sqs["sq4"].search_refine(store, q[:nt], a.k, kc, sp)[0])
    lens = np.diff(off)
    rows_s, rows_pairs, T = streamed_rows(q, cent, lens, min(a.nprobe, a.nlist), a.nlist)
    ld = (a.dim + 15) // 16 * 16
    row_bytes = {sq_name(b): {4: (ld // 2 + 15) // 16 * 16, 8: ld, 16: 2 * ld}[b] + 4 for b in widths}  # a stored row and its label
    scan = {name: kern[name]["sq_ivf_scan"]["ms"] for name in sqs}
    scan_ms = scan[sq_name(widths[0])]
    f32_ms = kern["ivfflat_canonical"]["ivf_scan"]["ms"] if a.competitors else None
    ldc = row_bytes[sq_name(widths[0])] - 4
    return {
        "queries": nq, "T": T, "build_s": t_build,
        "sq_scan_ms": scan,
        "sq_scan_bytes_per_s_by_width": {name: rows_s * row_bytes[name] / (ms * 1e-3) if ms else None for name, ms in scan.items()},
        "call_ms_median": {n: 1e3 * float(np.median(t)) for n, t in times.items()},
        "call_ms_all": {n: [1e3 * v for v in t] for n, t in times.items()},
        "kernel_ms_hip_events": kern,
        "rows_streamed": rows_s, "rows_probed_pairs": rows_pairs,
        "sq_scan_bytes": rows_s * (ldc + 4),
        "sq_scan_bytes_per_s": rows_s * (ldc + 4) / (scan_ms * 1e-3) if scan_ms else None,
        "canonical_f32_scan_bytes_per_s_same_rows": rows_s * (a.dim * 4 + 4) / (f32_ms * 1e-3) if f32_ms else None,
        "memory_usage": {**{n: ix.memory_usage for n, ix in sqs.items()}, **{n: ix.memory_usage for n, ix in flats.items()}},
        "recall_at_k_vs_exact": recall, "longest_list": int(lens.max()), "empty_lists": int((lens == 0).sum()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=0,
                    help="seconds per batch size (a child process each: it generates the rows, builds three indexes, measures and runs "
                         "the exact scan); 0: 300 + 300 per 2^20 rows")
    ap.add_argument("--bit-size", default="8", help="code widths of the SQ indexes, a list of 8, 4 and 16; the first one's figures fill the sq_scan_* fields")
    ap.add_argument("--competitors", type=int, default=1, help="0: no IVFFLAT indexes beside the SQ ones")
    ap.add_argument("--out", default=os.path.join("profiles", "sq_ivf.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    limit = a.limit if a.limit > 0 else 300 + 300 * max(1, a.rows >> 20)
    if a.child:
        print("RESULT " + json.dumps(child(a, a.child)))
        return
    res = {"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "k": a.k, "nprobe": a.nprobe, "metric": "L2", "version": capi.version(), "bit_size": a.bit_size, "batches": []}
    for nq in [int(v) for v in a.batches.split(",")]:
        cmd = [sys.executable, "-m", "tools.bench_sq_ivf", "--child", str(nq)]
        for key in ("rows", "dim", "nlist", "nprobe", "k", "reps", "competitors"):
            cmd += ["--" + key, str(getattr(a, key))]
        cmd += ["--bit-size", a.bit_size]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("batch %d failed (exit %d): nothing further is started" % (nq, p.returncode))
        res["batches"].append(json.loads(line[0][7:]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (after every batch: what has been measured survives a later child's failure)
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
