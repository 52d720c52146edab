"""Search::VectorIndex<..., BinaryVector>::search of the compiled host shim with k beyond MSVS_MAX_K: the host asks the binary index
for the same k as the float one (LIMIT 1000, k + deleted rows), and MsvsBinaryIndex::search passes it to
msvs_bin_index_search_rounds.  shim/test_shim_bin_large_k.cpp builds a BinaryFLAT index over the tie rows of test_bin_large_k.py
(labels in no storage order) and searches it with k = 10 and k = 1000, with and without a filter bitmap; the results == the numpy
reference of that file, ids exactly and distances by their bits."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_bin_large_k import BOUNDARIES, NLABEL, assert_boundaries_inside_ties, ref_topk, same, tie_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "shim", "_build", "test_shim_bin_large_k")
HAM, JAC = 3, 4  # MSVS_METRIC_HAMMING, MSVS_METRIC_JACCARD


def test_driver_is_built():
    assert os.path.exists(EXE), "run `python -c 'import __graft_entry__ as g; g.build()'`"


@pytest.mark.gpu
def test_shim_binary_search_beyond_256_matches_the_sort():
    t = tie_data(64)
    ks = (10, 1000)
    alive = np.random.default_rng(13).random(NLABEL) < 0.6
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "meta.txt"), "w") as f:
            f.write("%d %d %d %d %s\n" % (len(t.rows), t.nbytes, len(t.q), NLABEL, " ".join(str(k) for k in ks)))
        for name, a in (("bx", t.rows), ("blabels", t.labels), ("bq", t.q), ("balive", alive.astype(np.uint8))):
            np.ascontiguousarray(a).tofile(os.path.join(td, name + ".bin"))
        r = subprocess.run([EXE, td], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        for tag, metric in (("ham", HAM), ("jac", JAC)):
            for k in ks:
                for suffix, al in (("", None), ("_f", alive)):
                    ri, rd = ref_topk(t.q, t.rows, t.labels, k, metric, alive=al)
                    if k > 256 and al is None:  # the base query: the round boundaries lie inside runs of equal distances
                        assert_boundaries_inside_ties(rd[0], [b for b in BOUNDARIES if b < k])
                    base = os.path.join(td, "bi_%s_k%d_" % (tag, k))
                    ids = np.fromfile(base + "ids%s.bin" % suffix, np.int64).reshape(len(t.q), k)
                    dis = np.fromfile(base + "dis%s.bin" % suffix, np.float32).reshape(len(t.q), k)
                    same(ids, dis, ri, rd)
