"""IVFPQ against IVFSQ and IVFFLAT on one GPU: 1M x 768 rows in blobs (sigma 0.3), nlist 1024, L2, m = 96 and m = 48, nprobe 32,
k = 10 and 100, batches of 64, 1024 and 4096 queries.  The competitors are the IVFSQ index and the default IVFFLAT index of the same
rows; every index trains its coarse centroids with the same trainer on the same rows and parameters, so all have the same lists.
Whole calls by the host clock around calls that end in a stream synchronisation, medians of --reps after warm-up, the indexes
alternating; the scan kernels by HIP events (msvs_profile_*) in a pass of their own, and the PQ scan once more with its row loop
skipped (option pq_ivf_tables_only): the share of the kernel spent building tables; the PQ scan kernel at row-segment lengths
(pq_ivf_rpb) 256 - 2048 against the planned default.  Recall 10-in-10 and 10-in-100 against an exact
scan of the original rows on the first 256 queries; memory_usage and build seconds of every index.  LDS bank conflicts of the PQ scan
(SQ_LDS_BANK_CONFLICT against SQ_LDS_IDX_ACTIVE) come from a counter-only run of a smaller index with lists of the same length.
Every batch size runs in a child process of its own under a time limit, and the run stops at the first child that fails.  Writes one
JSON file (default profiles/pq_ivf.json).

An entry of --ms is M for an 8-bit index or Mx4 for a 4-bit one (bit_size=4), named pqM / pqMx4 in the output: --ms 96,192x4,96x4
puts 8-bit m = 96 beside its equal-bytes 4-bit partner m = 192 and the half-size m = 96 (profiles/pq4_ivf.json).  The counter run
then takes the first 8-bit and the first 4-bit entry, whose scan kernels differ in their first template argument.  --no-competitors leaves the IVFSQ
and IVFFLAT indexes out.

--query-tables builds every PQ index a second time in the query-table form (query_tables=1), named pqMqt / pqMx4qt: the same rows in
the same chunks over the first one's codebook (set_codebook from its export), so the two hold the same codes and differ in the
distance alone; they alternate with the others, the table kernel of the form is the family pq_query_tables, and the prologue share
(pq_ivf_tables_only) is taken for both forms (profiles/pq_qt_ivf.json: --ms 96,48,96x4,48x4 --ks 10 --query-tables --no-competitors).

    python -m tools.bench_pq_ivf [--rows N] [--dim D] [--nlist L] [--ms 96,48] [--batches 64,1024,4096] [--nprobe P] [--ks 10,100]
                                 [--reps R] [--no-counters] [--no-competitors] [--query-tables] [--out FILE]
"""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import myscaledb_amd.capi as capi  # noqa: E402

F = np.float32
# the profiler names the scan "void msvs::pq_ivf_scan_kernel<8, 0, 8, 1>(msvs::PqIvfParams)"; a mangled name (...ILi8E...) is read too
SCAN_BITS = re.compile(r"pq_ivf_scan_kernel(?:<|ILi)(\d+)")
FAMILIES = ("pq_ivf_scan", "pq_query_tables", "sq_ivf_scan", "ivf_scan", "ivf_plan", "flat_scan", "merge", "coarse_pass")


def blobs(rng, centres, n):
    out = np.empty((n, centres.shape[1]), F)
    for b in range(0, n, 1 << 16):
        m = min(1 << 16, n - b)
        out[b:b + m] = centres[rng.integers(0, len(centres), m)] + F(0.3) * rng.standard_normal((m, centres.shape[1]), dtype=F)
    return out


def data(a, nq):
    rng = np.random.default_rng(21)
    centres = rng.standard_normal((a.nlist, a.dim), dtype=F)
    return blobs(rng, centres, a.rows), blobs(rng, centres, nq)


def built(make, x, a):
    """-> (index, build seconds): trained on every (rows / (128 nlist))-th row, fed in chunks of 2^17"""
    t0 = time.perf_counter()
    ix = make()
    ix.train(x[::max(1, a.rows // (128 * a.nlist))])
    for b in range(0, a.rows, 1 << 17):
        ix.add(x[b:b + (1 << 17)], np.arange(b, min(a.rows, b + (1 << 17)), dtype=np.int64))
    ix.build()
    sys.stderr.write("built %s in %.1f s\n" % (type(ix).__name__, time.perf_counter() - t0))
    sys.stderr.flush()
    return ix, time.perf_counter() - t0


def built_twin(first, spec, x, a):
    """-> (the query-table index over `first`'s codebook and the same rows in the same chunks, build seconds without training)"""
    t0 = time.perf_counter()
    cent, cb = first.export(with_lists=False)[:2]
    ix = capi.PqIndex(capi.METRIC_L2, a.dim, pq_params(spec)[1:] + ",query_tables=1")
    ix.set_codebook(cent, cb)
    for b in range(0, a.rows, 1 << 17):
        ix.add(x[b:b + (1 << 17)], np.arange(b, min(a.rows, b + (1 << 17)), dtype=np.int64))
    ix.build()
    return ix, time.perf_counter() - t0


def pq_name(spec):
    m, bits = spec
    return "pq%d" % m if bits == 8 else "pq%dx%d" % (m, bits)


def pq_params(spec):
    m, bits = spec
    return ",m=%d" % m if bits == 8 else ",m=%d,bit_size=%d" % (m, bits)  # (an 8-bit index is created as it always was)


def profiled(fn):
    capi.profile_enable(True)
    capi.profile_reset()
    fn()
    out = {f: dict(zip(("calls", "ms"), capi.profile_get(f))) for f in FAMILIES}
    capi.profile_enable(False)
    return out


def child(a, nq):
    capi.set_device(0)
    x, q = data(a, nq)
    params = "ncentroids=%d,kmeans_iters=4,train_sample=%d" % (a.nlist, min(a.rows, 64 * a.nlist))
    index, build_s = {}, {}
    for spec in a.ms:
        index[pq_name(spec)], build_s[pq_name(spec)] = built(lambda: capi.PqIndex(capi.METRIC_L2, a.dim, params + pq_params(spec)), x, a)
        if a.query_tables:
            index[pq_name(spec) + "qt"], build_s[pq_name(spec) + "qt"] = built_twin(index[pq_name(spec)], spec, x, a)
    if not a.no_competitors:
        index["sq"], build_s["sq"] = built(lambda: capi.SqIndex(capi.METRIC_L2, a.dim, params), x, a)
        index["ivfflat"], build_s["ivfflat"] = built(lambda: capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, a.dim, params), x, a)
    sp = "nprobe=%d" % a.nprobe
    nt = min(nq, 256)
    truth, _ = capi.knn(q[:nt], x, 10, capi.METRIC_L2)
    out = {"queries": nq, "build_s": build_s, "memory_usage": {n: ix.memory_usage for n, ix in index.items()}, "k": {}}
    lens = np.diff(index[pq_name(a.ms[0])].export()[2])
    out["longest_list"], out["empty_lists"] = int(lens.max()), int((lens == 0).sum())
    for k in a.ks:
        runs = {n: (lambda ix: lambda: ix.search(q, k, sp))(ix) for n, ix in index.items()}
        results = {n: fn() for n, fn in runs.items()}
        for _ in range(2):  # warm-up of every shape
            for fn in runs.values():
                fn()
        times = {n: [] for n in runs}
        for _ in range(a.reps):  # alternating: other work shares the host
            for n, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                times[n].append(time.perf_counter() - t0)
        kern = {n: profiled(fn) for n, fn in runs.items()}  # kernel families by HIP events, in a pass of its own
        tables = {}
        capi.set_option("pq_ivf_tables_only", 1)
        try:
            for n in [n for n in runs if n.startswith("pq")]:
                tables[n] = profiled(runs[n])["pq_ivf_scan"]["ms"]
        finally:
            capi.set_option("pq_ivf_tables_only")

        def share(ids, width):
            return float(np.mean([len(set(truth[i].tolist()) & set(ids[i][:width].tolist())) / 10 for i in range(nt)]))

        out["k"][str(k)] = {
            "call_ms_median": {n: 1e3 * float(np.median(t)) for n, t in times.items()},
            "call_ms_all": {n: [1e3 * v for v in t] for n, t in times.items()},
            "kernel_ms_hip_events": kern,
            "pq_scan_ms_tables_only": tables,
            "pq_scan_table_share": {n: (v / kern[n]["pq_ivf_scan"]["ms"] if kern[n]["pq_ivf_scan"]["ms"] else None) for n, v in tables.items()},
            "recall_10_in_10": {n: share(r[0], 10) for n, r in results.items()},
            "recall_10_in_k": {n: share(r[0], k) for n, r in results.items()},
        }
    # the row-segment length: the PQ scan kernel alone (first m, first k) at the planned default (0) and at fixed lengths
    run = lambda: index[pq_name(a.ms[0])].search(q, a.ks[0], sp)
    out["rpb_sweep_scan_ms"] = {}
    try:
        for rpb in (0, 256, 512, 1024, 2048):
            capi.set_option("pq_ivf_rpb", rpb)
            run()
            out["rpb_sweep_scan_ms"][str(rpb)] = float(np.median([profiled(run)["pq_ivf_scan"]["ms"] for _ in range(3)]))
    finally:
        capi.set_option("pq_ivf_rpb")
    return out


def counter_child(a, nq):
    """PQ indexes (the first 8-bit and the first 4-bit entry of --ms) of rows / 8 rows in nlist / 8 lists (lists as long as the full
    shape's), one batch searched twice through each"""
    capi.set_device(0)
    a.rows, a.nlist = max(4096, a.rows // 8), max(8, a.nlist // 8)
    x, q = data(a, nq)
    specs = [next(s for s in a.ms if s[1] == bits) for bits in (8, 4) if any(s[1] == bits for s in a.ms)]
    for spec in specs:
        ix, _ = built(lambda: capi.PqIndex(capi.METRIC_L2, a.dim, "ncentroids=%d,kmeans_iters=4" % a.nlist + pq_params(spec)), x, a)
        for _ in range(2):
            ix.search(q, a.ks[0], "nprobe=%d" % min(a.nprobe, a.nlist))
        ix.close()
    return {"rows": a.rows, "nlist": a.nlist, "queries": nq, "indexes": [pq_name(s) for s in specs], "k": a.ks[0]}


def spawn(a, extra, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, "-m", "tools.bench_pq_ivf"] + extra
    for key in ("rows", "dim", "nlist", "nprobe", "reps"):
        cmd += ["--" + key, str(getattr(a, key))]
    cmd += ["--ms", ",".join(pq_name(s)[2:] for s in a.ms), "--ks", ",".join(map(str, a.ks))]
    if a.no_competitors:
        cmd.append("--no-competitors")
    if a.query_tables:
        cmd.append("--query-tables")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit, cwd=ROOT)  # the child's progress lines (stderr) pass through
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:])
        raise SystemExit("%s failed (exit %d): nothing further is started" % (" ".join(extra), p.returncode))
    return json.loads(line[0][7:])


def counters(a, limit):
    """SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of the PQ scan kernel: a run that collects counters and nothing else"""
    with tempfile.TemporaryDirectory() as tmp:
        shape = spawn(a, ["--counter-child", str(a.counter_batch)], limit,
                      prefix=("rocprofv3", "--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "-d", tmp, "-o", "p", "--"))
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if not dbs:
            return {"shape": shape, "error": "the profiler left no database"}
        c = sqlite3.connect(dbs[0])
        cols = [r[1] for r in c.execute("pragma table_info(counters_collection)")]
        name_col = "kernel_name" if "kernel_name" in cols else "name"
        out = {"shape": shape}
        # one scan kernel, told apart by its first template argument (the bits of a code); the keys are the names the two scans had
        # when they were two kernels, so that earlier profiles stay comparable
        for kernel, bits in (("pq_ivf_scan_kernel", 8), ("pq4_ivf_scan_kernel", 4)):
            sums = {}
            for nm, cn, calls, total in c.execute("select %s, counter_name, count(*), sum(value) from counters_collection group by %s, counter_name"
                                                  % (name_col, name_col)):
                got = SCAN_BITS.search(nm)
                if got and int(got.group(1)) == bits:
                    sums[cn] = sums.get(cn, 0.0) + float(total)
            if not sums:
                continue
            conflict, active = sums.get("SQ_LDS_BANK_CONFLICT"), sums.get("SQ_LDS_IDX_ACTIVE")
            out[kernel] = {"SQ_LDS_BANK_CONFLICT": conflict, "SQ_LDS_IDX_ACTIVE": active,
                           "conflict_share_of_active": conflict / active if conflict is not None and active else None}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--ms", default="96,48", help="sub-quantisers of the PQ indexes: M (8 bits a code) or Mx4 (bit_size=4)")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=0,
                    help="seconds per batch size (a child process each: it generates the rows, builds the indexes, measures and runs the "
                         "exact scan); 0: 300 + 300 per 2^20 rows")
    ap.add_argument("--no-counters", action="store_true", help="skip the counter-only run (it needs rocprofv3)")
    ap.add_argument("--no-competitors", action="store_true", help="the PQ indexes only: no IVFSQ and no IVFFLAT index")
    ap.add_argument("--query-tables", action="store_true", help="every PQ index once more with query_tables=1 over the same codebook")
    ap.add_argument("--counter-batch", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join("profiles", "pq_ivf.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--counter-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.ms = [(int(v.split("x")[0]), int(v.split("x")[1]) if "x" in v else 8) for v in a.ms.split(",")]
    a.ks = [int(v) for v in a.ks.split(",")]
    limit = a.limit if a.limit > 0 else 300 + 300 * max(1, a.rows >> 20)
    if a.child:
        print("RESULT " + json.dumps(child(a, a.child)))
        return
    if a.counter_child:
        print("RESULT " + json.dumps(counter_child(a, a.counter_child)))
        return
    res = {"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "ms": [pq_name(s) for s in a.ms], "ks": a.ks, "nprobe": a.nprobe, "metric": "L2", "version": capi.version(),
           "batches": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():  # after every child: a run that stops early keeps what it has measured
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for nq in [int(v) for v in a.batches.split(",") if v]:  # (--batches "": the counter run alone)
        res["batches"].append(spawn(a, ["--child", str(nq)], limit))
        write()
    if not a.no_counters:
        res["lds_counters"] = counters(a, limit)
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
