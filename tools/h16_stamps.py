"""Per-item stamps of the shadow list scan's main launch on the bench's headline step (option h16_stamps, msvs_debug_h16_stamps):

    python tools/h16_stamps.py [key=value[,key=value] ...]        e.g.  python tools/h16_stamps.py h16_items=0 h16_items=1

Every argument is one configuration (option names of DESIGN.md's knob table), run one after the other on the same index.  Builds bench.py's headline index (blobs03, 1M x 768, nlist 1024), warms up, times 40 steps with the stamps off, then runs THREE steps of 4096 queries at nprobe 32 with the stamps
on and prints, for each of them, where a workgroup's time goes: per item the set-up (item popped -> tile resident), the rows (tile resident -> every
wavefront done) and the gap to the next item's pop (the queue's atomic between two barriers); per launch the items per workgroup and
the idle tail (first workgroup out of items -> last workgroup done).  The clock is the 100 MHz wall clock.  SHAPE=rows,batch,nprobe
in the environment changes the shape.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myscaledb_amd.capi as capi  # noqa: E402
from bench import data_model, ivf_params  # noqa: E402


H_STAMP_ITEMS = 64  # h16_scan_kernels.hpp: stamp records per workgroup (record 0 holds the workgroup's item count), 4 words each


def read_stamps():
    buf = np.zeros(4096 * H_STAMP_ITEMS * 4, np.uint64)
    grid = C.c_uint32(0)
    fn = capi.lib().msvs_debug_h16_stamps
    fn.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint32)]
    capi._check(fn(buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size, C.byref(grid)))
    g = grid.value
    return buf[:g * H_STAMP_ITEMS * 4].reshape(g, H_STAMP_ITEMS, 4).astype(np.int64)


def pct(v, qs=(10, 50, 90)):
    v = np.asarray(v, np.float64) / 100.0
    return "/".join("%.2f" % np.percentile(v, q) for q in qs) if v.size else "-"


def summarise(st):
    g = st.shape[0]
    nit = np.minimum(st[:, 0, 0], H_STAMP_ITEMS - 1)
    setup, rows, gap, nval, first, last_end, wg_setup, wg_rows, wg_gap = [], [], [], [], [], [], [], [], []
    for b in range(g):
        k = int(nit[b])
        if not k:
            continue
        it = st[b, 1:k + 1]
        setup.extend(it[:, 1] - it[:, 0])
        rows.extend(it[:, 2] - it[:, 1])
        gap.extend(it[1:, 0] - it[:-1, 2])
        nval.extend((it[:, 3] >> 8) & 0xFFFFFF)
        first.append(it[0, 0])
        last_end.append(it[-1, 2])
        wg_setup.append((it[:, 1] - it[:, 0]).sum())
        wg_rows.append((it[:, 2] - it[:, 1]).sum())
        wg_gap.append((it[1:, 0] - it[:-1, 2]).sum())
    start, end = min(first), max(last_end)
    print("grid %d, workgroups with items %d, items %d; items per workgroup min/mean/max %d/%.2f/%d; queries per item p10/p50/p90/max %s/%d"
          % (g, len(first), len(setup), nit.min(), nit.mean(), nit.max(), "/".join("%d" % np.percentile(nval, q) for q in (10, 50, 90)), max(nval)))
    print("launch span (first pop -> last workgroup done) %.2f us; first pop after the earliest, us p50/max %.2f/%.2f"
          % ((end - start) / 100.0, np.percentile(np.asarray(first) - start, 50) / 100.0, (max(first) - start) / 100.0))
    print("per item, us p10/p50/p90: set-up %s (mean %.2f); rows %s (mean %.2f); gap to the next pop %s (mean %.2f)"
          % (pct(setup), np.mean(setup) / 100.0, pct(rows), np.mean(rows) / 100.0, pct(gap), np.mean(gap) / 100.0 if gap else 0.0))
    print("per workgroup, us mean: set-up %.2f, rows %.2f, gaps %.2f; set-up + gaps p10/p50/p90 %s"
          % (np.mean(wg_setup) / 100.0, np.mean(wg_rows) / 100.0, np.mean(wg_gap) / 100.0, pct(np.asarray(wg_setup) + np.asarray(wg_gap))))
    tail = end - np.asarray(last_end)
    print("idle tail: first workgroup out of items %.2f us before the launch's end; per workgroup us p10/p50/p90 %s, mean %.2f"
          % ((end - min(last_end)) / 100.0, pct(tail), tail.mean() / 100.0))


def main():
    n, B, nprobe = (int(v) for v in os.environ.get("SHAPE", "1000000,4096,32").split(","))
    d, nlist, k = 768, 1024, 10
    dev = torch.device("cuda", 0)
    capi.set_device(0)
    x, q_all, _ = data_model("blobs03", n, 8 * B, d, dev)
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, ivf_params(nlist, n))
    ix.train(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    ix.add(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    ix.build()
    stream = torch.cuda.current_stream().cuda_stream
    oi = torch.empty((B, k), device=dev, dtype=torch.int64)
    od = torch.empty((B, k), device=dev, dtype=torch.float32)

    def step(i):
        ix.search_device(q_all[(i % 8) * B:(i % 8 + 1) * B].data_ptr(), B, k, nprobe, oi.data_ptr(), od.data_ptr(), stream)

    for conf in sys.argv[1:] or [""]:
        kv = dict(p.split("=") for p in conf.split(",") if p)
        for name, value in kv.items():
            capi.set_option(name, value)
        for i in range(5):
            step(i)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(40):
            step(i)
        torch.cuda.synchronize()
        print("options %s: %.4f ms per step (40 steps, stamps off)" % (kv, (time.perf_counter() - t) / 40 * 1e3))
        capi.set_option("h16_stamps", "1")
        for i in range(5, 8):  # three stamped steps, each summarised on its own
            step(i)
            torch.cuda.synchronize()
            print("step %d, options %s" % (i, kv))
            summarise(read_stamps())
        capi.set_option("h16_stamps", None)
        for name in kv:
            capi.set_option(name, None)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
