"""How many queries does coarse_tail_kernel's prune-first path serve (option coarse_prune_first; round 12), and how large is the set S''
of lists a conservative test cannot prune under the nearest list's bound?  Per data model of the bench: 8 batches of 4096 queries on the
headline index with coarse_prune_debug = 1 -- served share, surviving pairs per served query, the distribution of |S''| (flag words of
msvs_debug_prune_first: bit 0 served, bits 8 and up |S''|).
    python tools/prune_first_probe.py [blobs03|iid|mid]"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import myscaledb_amd.capi as capi  # noqa: E402
from bench import data_model, ivf_params  # noqa: E402

dev = torch.device("cuda", 0)
capi.set_option("coarse_prune_debug", "1")
for name in (sys.argv[1:] or ["blobs03", "mid", "iid"]):
    n, d, nlist, nprobe, k, B = 1_000_000, 768, 1024, 32, 10, 4096
    x, q_all, desc = data_model(name, n, 8 * B, d, dev)
    ix = capi.Index(capi.INDEX_IVFFLAT, capi.METRIC_L2, d, ivf_params(nlist, n, ""))
    ix.train(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    ix.add(x.data_ptr(), n=n, mem=capi.MEM_DEVICE)
    ix.build()
    oi = torch.empty((B, k), device=dev, dtype=torch.int64)
    od = torch.empty((B, k), device=dev, dtype=torch.float32)
    st = torch.cuda.current_stream().cuda_stream
    served, kept, members, attempted = 0, 0, [], 0
    for i in range(8):
        ix.search_device(q_all[i * B:(i + 1) * B].data_ptr(), B, k, nprobe, oi.data_ptr(), od.data_ptr(), st)
        have, probes, upre, flags = capi.debug_prune_first(B, nprobe)
        s = (flags & 1) != 0
        served += int(s.sum())
        kept += int((probes[s] >= 0).sum())
        m = flags >> 8
        attempted += int((m > 0).any() or s.any())
        members.append(m)
    m = np.concatenate(members)
    hist = {b: int(((m >= lo) & (m <= hi)).sum()) for b, lo, hi in (("0", 0, 0), ("1", 1, 1), ("2", 2, 2), ("3-4", 3, 4), ("5-8", 5, 8), ("9-16", 9, 16),
                                                                    ("17-32", 17, 32), ("33-64", 33, 64), (">64", 65, 1 << 24))}
    print(name, "batches that attempted: %d of 8; served %d of %d (%.2f %%); pairs per served query %.3f; |S''| %s"
          % (attempted, served, 8 * B, 100.0 * served / (8 * B), kept / max(served, 1), hist), flush=True)
    ix.close()
    del x, q_all
    torch.cuda.empty_cache()
