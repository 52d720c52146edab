"""Partitioned against flat binary index on one GPU: 4M rows x 64 bytes (clustered), nlist 1024, 1024 queries, k 10, Hamming,
nprobe 64.  Times whole search calls (host clock around calls that end in a stream synchronisation, after warm-up, the two
indexes alternating) and, in a pass of its own, the kernel families by HIP events (msvs_profile_*).  The flat search is the
yardstick; the partitioned one touches ~1/16 of the rows.  Writes one JSON file (default profiles/bin_ivf.json).

    python -m tools.bench_bin_ivf [--rows N] [--nlist L] [--queries Q] [--nprobe P] [--k K] [--reps R] [--rounds-k K1,K2] [--out FILE]

Also (--rounds-k, default 256,1024): the same two searches through search_rounds with each of those k, whole calls and kernel
families, to price a search in rank rounds against one round.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myscaledb_amd.capi as capi  # noqa: E402

POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def noisy(rng, centres, n):
    """n rows: a random centre each, every bit flipped with probability 1/8 (the AND of three random bytes)."""
    out = np.empty((n, centres.shape[1]), np.uint8)
    for b in range(0, n, 1 << 18):
        m = min(1 << 18, n - b)
        shape = (m, centres.shape[1])
        flips = rng.integers(0, 256, shape, dtype=np.uint8) & rng.integers(0, 256, shape, dtype=np.uint8) \
            & rng.integers(0, 256, shape, dtype=np.uint8)
        out[b:b + m] = centres[rng.integers(0, len(centres), m)] ^ flips
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--nbytes", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds-k", default="256,1024", help="k values of the rank-round comparison through search_rounds ('' skips it)")
    ap.add_argument("--out", default=os.path.join("profiles", "bin_ivf.json"))
    a = ap.parse_args()
    capi.set_device(0)
    rng = np.random.default_rng(20)
    centres = rng.integers(0, 256, (a.nlist, a.nbytes), dtype=np.uint8)
    rows = noisy(rng, centres, a.rows)
    q = noisy(rng, centres, a.queries)
    params = "nprobe=%d" % a.nprobe
    # the generating centres are the centroids: the structure is pinned, the build is assignment + grouping only
    ivf = capi.BinIndex(a.nbytes, capi.METRIC_HAMMING, "ncentroids=%d" % a.nlist)
    ivf.set_centroids(centres)
    ivf.add(rows)
    flat = capi.BinIndex(a.nbytes, capi.METRIC_HAMMING)
    flat.add(rows)
    t0 = time.perf_counter()
    ii, idis = ivf.search(q, a.k, params=params)  # (builds the image: assignment on the device, grouping on the host)
    t_build = time.perf_counter() - t0
    fi, fdis = flat.search(q, a.k)
    for _ in range(2):  # warm-up of both shapes
        ivf.search(q, a.k, params=params)
        flat.search(q, a.k)
    t_ivf, t_flat = [], []
    for _ in range(a.reps):  # alternating: other work shares the host
        t0 = time.perf_counter()
        ivf.search(q, a.k, params=params)
        t_ivf.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        flat.search(q, a.k)
        t_flat.append(time.perf_counter() - t0)
    # kernel families by HIP events, in a pass of its own
    capi.profile_enable(True)
    capi.profile_reset()
    ivf.search(q, a.k, params=params)
    flat.search(q, a.k)
    names = ("bin_ivf_coarse", "ivf_plan", "bin_ivf_scan", "merge", "bin_scan")
    kern = {n: dict(zip(("calls", "ms"), capi.profile_get(n))) for n in names}
    capi.profile_enable(False)
    # rows of the probed lists (what the list scan has to look at), from the exported offsets and the probe rule
    off = ivf.export()[1]
    lens = np.diff(off)
    probed = 0
    for b in range(0, a.queries, 64):
        d = POP8[q[b:b + 64, None, :] ^ centres[None, :, :]].sum(axis=2, dtype=np.int64)
        order = np.argsort(d * a.nlist + np.arange(a.nlist)[None, :], axis=1)[:, :min(a.nprobe, a.nlist)]
        probed += int(lens[order].sum())
    # k beyond 256 in rank rounds against one round on the same data: whole calls, alternating, and the scan / merge families of
    # one call each by HIP events (the expectation: about k / 256 times the scan, one plan)
    rounds = {}
    if a.rounds_k:
        ks = [int(v) for v in a.rounds_k.split(",")]
        calls = {(name, k): [] for name in ("ivf", "flat") for k in ks}
        for rep in range(1 + a.reps):  # (the first pass warms up every shape)
            for k in ks:
                for name, ix, p in (("ivf", ivf, params), ("flat", flat, None)):
                    t0 = time.perf_counter()
                    ix.search_rounds(q, k, params=p)
                    if rep:
                        calls[(name, k)].append(time.perf_counter() - t0)
        capi.profile_enable(True)
        for k in ks:
            for name, ix, p in (("ivf", ivf, params), ("flat", flat, None)):
                capi.profile_reset()
                ix.search_rounds(q, k, params=p)
                rounds["%s_k%d" % (name, k)] = {
                    "call_ms_median": 1e3 * float(np.median(calls[(name, k)])), "call_ms_all": [1e3 * t for t in calls[(name, k)]],
                    "kernel_ms_hip_events": {n: dict(zip(("calls", "ms"), capi.profile_get(n))) for n in names}}
        capi.profile_enable(False)
    recall = float(np.mean([len(set(ii[i]) & set(fi[i])) / a.k for i in range(a.queries)]))
    ivf_ms, flat_ms = 1e3 * float(np.median(t_ivf)), 1e3 * float(np.median(t_flat))
    scan_ms = kern["bin_ivf_scan"]["ms"]
    res = {
        "rows": a.rows, "nbytes": a.nbytes, "nlist": a.nlist, "queries": a.queries, "k": a.k, "nprobe": a.nprobe, "metric": "Hamming",
        "ivf_call_ms_median": ivf_ms, "ivf_call_ms_all": [1e3 * t for t in t_ivf],
        "flat_call_ms_median": flat_ms, "flat_call_ms_all": [1e3 * t for t in t_flat],
        "ivf_over_flat": ivf_ms / flat_ms,
        "kernel_ms_hip_events": kern,
        "probed_rows": probed, "probed_fraction": probed / (a.queries * a.rows),
        "probed_bytes": probed * a.nbytes,
        "scan_probed_bytes_per_s": probed * a.nbytes / (scan_ms * 1e-3) if scan_ms else None,
        "flat_scan_bytes_per_s": a.queries * a.rows * a.nbytes / (kern["bin_scan"]["ms"] * 1e-3) if kern["bin_scan"]["ms"] else None,
        "longest_list": int(lens.max()), "empty_lists": int((lens == 0).sum()),
        "recall_at_k_vs_flat": recall, "first_search_with_image_build_s": t_build, "version": capi.version(),
        "rank_rounds": rounds,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
