"""Searches with more than 256 results on one GPU: what the exact rank-window rounds of the BM25 entries cost, and a hybrid batch
with num_candidates = 300 beside the same batch at 256.

BM25: the 10M-document corpus of bench.py's BM25 leg (bench.build_postings), 2-4 mid-frequency terms per query, batches of 1 and
64, k = 256 / 300 / 1024 / 4096, device entry, stream-ordered, timed around a stream synchronisation after warm-up.  k = 256 is
the unchanged path; it is timed a second time with bm25_emit = 0 (per-chunk lists + one merge: the path a round repeats), which is
what ceil(k / 256) rounds should be held against.
Hybrid: IVFFLAT (cosine) top-k + BM25 top-k + RRF -> top-10 for a 64-query batch, all on the device, k = 256 and 300.

The measuring runs in a CHILD process that reports every step as one JSON line; this process never opens the GPU and holds every
step -- set-up, warm-up and repetitions together -- to its time limit (--setup-seconds for the two set-up steps, --step-seconds
for the others).  A step that runs out of time, or a child that dies, ends the run: the child is killed, the step is recorded
under "errors", nothing more is started on the GPU, and what had been measured is written.  A step that raises is recorded and
the next one runs.  Writes one JSON file (default profiles/large_k.json).

    python -m tools.bench_large_k [--docs N] [--vec-rows N] [--dim D] [--reps R] [--step-seconds S] [--setup-seconds S]
                                  [--skip-hybrid] [--out FILE]
"""
import argparse
import json
import os
import queue
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BM25_STEPS = [(B, k, emit) for B in (1, 64) for k, emit in ((256, 1), (256, 0), (300, 1), (1024, 1), (4096, 1))]


def bm25_name(B, k, emit):
    return "batch%d_k%d%s" % (B, k, "" if emit else "_exact_path")


def step_names(a):
    names = ["setup_bm25"] + [bm25_name(*s) for s in BM25_STEPS]
    if not a.skip_hybrid:
        names += ["setup_hybrid", "num_candidates_256", "num_candidates_300"]
    return names


def timed(step, reps, budget_s):
    """Median seconds of step(i) (each ends in a device synchronisation), at least 3 and at most `reps` repetitions inside the budget."""
    import torch

    out, t_end = [], time.perf_counter() + budget_s
    for i in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(i)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        if len(out) >= 3 and time.perf_counter() > t_end:
            break
    return float(np.median(out)), len(out)


def report(step, **kw):
    print(json.dumps(dict(step=step, **kw)), flush=True)


def worker(a):
    """The child: every step of step_names(a) in order, one JSON line each ("result" or "error")."""
    import torch

    import bench
    import myscaledb_amd.capi as capi

    capi.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    ps, df_all, total, n_post = bench.build_postings(a.docs, a.vocab)
    rng = np.random.default_rng(6)
    mids = np.argsort(-df_all)[50:2000]
    report("setup_bm25", result={"postings": int(n_post), "version": capi.version()})

    def bm25_step(B, k):
        sets = []
        for _ in range(3):
            terms = [rng.choice(mids, int(rng.integers(2, 5)), replace=False) for _ in range(B)]
            dfs = [df_all[t] for t in terms]
            sets.append((terms, dfs, ps.prepare_batch(terms, dfs, total)))
        o_i = torch.empty((B, k), device=dev, dtype=torch.int64)
        o_d = torch.empty((B, k), device=dev, dtype=torch.float32)

        def st(i):
            terms, dfs, prep = sets[i % 3]
            ps.bm25_search_batch_device(terms, dfs, a.docs, total, k, o_i.data_ptr(), o_d.data_ptr(), stream, prepared=prep)
        for i in range(3):  # warm-up: records, scratch arenas
            st(i)
        torch.cuda.synchronize()
        return st, o_i

    for B, k, emit in BM25_STEPS:
        name = bm25_name(B, k, emit)
        try:
            capi.set_option("bm25_emit", None if emit else "0")
            st, o_i = bm25_step(B, k)
            dt, n = timed(st, a.reps, a.step_seconds / 2)
            report(name, result={"ms_per_batch": round(dt * 1e3, 4), "us_per_query": round(dt / B * 1e6, 2), "rounds": -(-k // 256), "reps": n,
                                 "hits_of_query0": int((o_i[0] >= 0).sum().item())})
        except Exception as e:  # (a step must not cost the file)
            report(name, error=repr(e)[:300])
        finally:
            capi.set_option("bm25_emit", None)
    if a.skip_hybrid:
        return
    try:
        bq = 64
        g = torch.Generator(device=dev).manual_seed(9)
        x = torch.randn((a.vec_rows, a.dim), device=dev, dtype=torch.float32, generator=g)
        ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_COSINE, a.dim, bench.ivf_params(1024, a.vec_rows))
        ix.train(x.data_ptr(), n=a.vec_rows, mem=capi.MEM_DEVICE)
        ix.add(x.data_ptr(), n=a.vec_rows, mem=capi.MEM_DEVICE)
        ix.build()
        q = x[torch.randint(0, a.vec_rows, (bq,), device=dev, generator=g)] + 0.3 * torch.randn((bq, a.dim), device=dev, generator=g)
        terms = [rng.choice(mids, int(rng.integers(2, 5)), replace=False) for _ in range(bq)]
        dfs = [df_all[t] for t in terms]
        prep = ps.prepare_batch(terms, dfs, total)
        report("setup_hybrid", result={"vector_rows": a.vec_rows, "dim": a.dim, "nlist": 1024, "nprobe": 32, "queries": bq})
    except Exception as e:
        report("setup_hybrid", error=repr(e)[:300])
        return
    for k in (256, 300):
        name = "num_candidates_%d" % k
        try:
            v_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
            v_d = torch.empty((bq, k), device=dev, dtype=torch.float32)
            t_i = torch.empty((bq, k), device=dev, dtype=torch.int64)
            t_d = torch.empty((bq, k), device=dev, dtype=torch.float32)
            f_s = torch.empty((bq, 10), device=dev, dtype=torch.float32)
            f_l = torch.empty((bq, 10), device=dev, dtype=torch.int64)
            f_n = torch.empty((bq,), device=dev, dtype=torch.int32)

            def hy(i):
                ps.bm25_search_batch_device(terms, dfs, a.docs, total, k, t_i.data_ptr(), t_d.data_ptr(), stream, prepared=prep)
                ix.search_device(q.data_ptr(), bq, k, 32, v_i.data_ptr(), v_d.data_ptr(), stream)
                capi.hybrid_fuse_device("rrf", v_d.data_ptr(), v_i.data_ptr(), k, t_d.data_ptr(), t_i.data_ptr(), k, bq, 10, f_s.data_ptr(),
                                        f_l.data_ptr(), f_n.data_ptr(), stream, fusion_k=60)
            for i in range(2):
                hy(i)
            dt, n = timed(hy, a.reps, a.step_seconds / 2)
            report(name, result={"ms_per_batch": round(dt * 1e3, 3), "ms_per_query": round(dt / bq * 1e3, 4), "reps": n})
        except Exception as e:
            report(name, error=repr(e)[:300])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--vec-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--step-seconds", type=float, default=60.0)
    ap.add_argument("--setup-seconds", type=float, default=300.0)
    ap.add_argument("--skip-hybrid", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "large_k.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {"docs": a.docs, "vocab": a.vocab, "step_seconds": a.step_seconds, "setup_seconds": a.setup_seconds, "bm25": {}, "errors": {}}
    child = subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), "--worker"] + sys.argv[1:], stdout=subprocess.PIPE, text=True,
                             cwd=ROOT)
    lines = queue.Queue()

    def pump():
        for line in child.stdout:
            lines.put(line)
        lines.put(None)
    threading.Thread(target=pump, daemon=True).start()
    pending = step_names(a)
    while pending:
        limit = a.setup_seconds if pending[0].startswith("setup_") else a.step_seconds
        try:
            line = lines.get(timeout=limit)
        except queue.Empty:
            child.kill()
            res["errors"][pending[0]] = "time limit of %.0f s: child killed, %d later step(s) not run" % (limit, len(pending) - 1)
            break
        if line is None:
            res["errors"][pending[0]] = "the child ended (exit status %s): %d later step(s) not run" % (child.wait(), len(pending) - 1)
            break
        try:
            msg = json.loads(line)
        except ValueError:
            continue  # (a library's own output)
        if msg.get("step") not in pending:
            continue
        print(line.strip(), file=sys.stderr, flush=True)  # progress
        del pending[:pending.index(msg["step"]) + 1]  # (a failed set-up skips its steps)
        if "error" in msg:
            res["errors"][msg["step"]] = msg["error"]
        elif msg["step"] == "setup_bm25":
            res.update(msg["result"])
        elif msg["step"] == "setup_hybrid":
            res["hybrid"] = msg["result"]
        elif msg["step"].startswith("num_candidates_"):
            res["hybrid"][msg["step"]] = msg["result"]
        else:
            res["bm25"][msg["step"]] = msg["result"]
    if child.poll() is None:
        try:
            child.wait(timeout=30)
        except subprocess.TimeoutExpired:
            child.kill()
    for B in (1, 64):
        base = res["bm25"].get("batch%d_k256_exact_path" % B)
        for k in (300, 1024, 4096):
            r = res["bm25"].get("batch%d_k%d" % (B, k))
            if base and r:
                r["over_rounds_x_exact_path_at_256"] = round(r["ms_per_batch"] / (r["rounds"] * base["ms_per_batch"]), 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
