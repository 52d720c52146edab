"""The two-file format of the IVFSQ and IVFPQ indexes (capi.SqIndex / capi.PqIndex .serialize_io, .load_io), pinned to the byte.

Both files are rebuilt here in numpy from export() alone: header with its FNV-1a-64 check word, centroids, vmin / vmax or the
sub-codebooks, list offsets, codes in natural order; then the id header and the ids.  Codebooks are set, never trained; rows are
integer valued; three lists, the last one empty."""
import struct

import numpy as np
import pytest

import myscaledb_amd.capi as capi

pytestmark = pytest.mark.gpu
F = np.float32
L2, IP = capi.METRIC_L2, capi.METRIC_IP
NLIST = 3


def fnv1a(b):
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
    return h


def with_check(head):
    return head + struct.pack("<Q", fnv1a(head))


def rows_and_labels(rng, n, dim):
    """Integer-valued rows around the first two of three centroids (by L2 the third list stays empty) and explicit labels that
    reach the last one a label can be."""
    cent = np.zeros((NLIST, dim), F)
    cent[1], cent[2] = 40, -400
    x =(cent[rng.integers(0, 2, n)] + rng.integers(-3, 4, (n, dim))).astype(F)
    labels = rng.permutation(5 * n)[:n].astype(np.int64)
    labels[n // 2] = 2 ** 32 - 2
    return cent, x, labels


def sq_index(metric, dim, n):
    rng = np.random.default_rng(dim + n)
    cent, x, labels = rows_and_labels(rng, n, dim)
    ix = capi.SqIndex(metric, dim)
    ix.set_codebook(cent, np.full(dim, -4, F), np.arange(dim, dtype=F) % 7 + 4)
    ix.add(x[:n // 3], labels[:n // 3])
    ix.add(x[n // 3:], labels[n // 3:])
    ix.build()
    return ix


def pq_index(metric, dim, m, n):
    rng = np.random.default_rng(dim + n)
    cent, x, labels = rows_and_labels(rng, n, dim)
    ix = capi.PqIndex(metric, dim, "m=%d" % m)
    ix.set_codebook(cent, rng.integers(-4, 5, (m, 256, dim // m)).astype(F))
    ix.add(x[:n // 3], labels[:n // 3])
    ix.add(x[n // 3:], labels[n // 3:])
    ix.build()
    return ix


def id_file(magic, labels):
    return with_check(magic + struct.pack("<Q", len(labels))) + labels.astype("<i8").tobytes()


def check_lists(off, n):
    assert off[0] == 0 and off[-1] == n and off[2] == off[3] and 0 < off[1] < n  # two lists in use, the third empty


@pytest.mark.parametrize("dim", [20, 272])  # the stored row is all tail / one permuted 256-column block and a 16-byte tail
def test_sq_files_to_the_byte(dim):
    n = 130
    ix = sq_index(L2, dim, n)
    cent, lo, hi, off, codes, labels = ix.export()
    check_lists(off, n)
    assert codes.shape == (n, dim) and (labels == 2 ** 32 - 2).sum() == 1
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["sq_data", "sq_ids"]
    data = with_check(b"MSVSSQ01" + struct.pack("<IiQQQQ", 1, L2, dim, NLIST, n, 0)) + cent.astype("<f4").tobytes() \
        + lo.astype("<f4").tobytes() + hi.astype("<f4").tobytes() + off.astype("<i8").tobytes() + codes.tobytes()
    assert bytes(store["sq_data"]) == data
    assert bytes(store["sq_ids"]) == id_file(b"MSVSSQID", labels)
    ld = capi.SqIndex.load_io(store, L2, dim)
    again = {}
    ld.serialize_io(again)
    assert bytes(again["sq_data"]) == data and bytes(again["sq_ids"]) == bytes(store["sq_ids"])
    ld.close()
    ix.close()


# m = 5: two words a row, three padding bytes; 130 rows are two whole blocks of 64 and a partial one.  m = 8, 64 rows: one block.
@pytest.mark.parametrize("dim,m,n", [(20, 5, 130), (8, 8, 64)])
def test_pq_files_to_the_byte(dim, m, n):
    ix = pq_index(L2, dim, m, n)
    cent, cb, off, codes, labels = ix.export()
    check_lists(off, n)
    assert codes.shape == (n, m) and (labels == 2 ** 32 - 2).sum() == 1
    store = {}
    ix.serialize_io(store)
    assert sorted(store) == ["pq_data", "pq_ids"]
    data = with_check(b"MSVSPQ01" + struct.pack("<IiQQQQQ", 1, L2, dim, m, NLIST, n, 0)) + cent.astype("<f4").tobytes() \
        + cb.astype("<f4").tobytes() + off.astype("<i8").tobytes() + codes.tobytes()
    assert bytes(store["pq_data"]) == data
    assert bytes(store["pq_ids"]) == id_file(b"MSVSPQID", labels)
    ld = capi.PqIndex.load_io(store, L2, dim, m)
    again = {}
    ld.serialize_io(again)
    assert bytes(again["pq_data"]) == data and bytes(again["pq_ids"]) == bytes(store["pq_ids"])
    ld.close()
    ix.close()


def test_sq_loaded_geometry_comes_from_the_file():
    ix = sq_index(IP, 100, 130)
    exp = ix.export()
    store = {}
    ix.serialize_io(store)
    ld = capi.SqIndex.load_io(store)  # nothing repeated by the caller
    assert (ld.metric, ld.dim) == (IP, 100)
    for a, b in zip(exp, ld.export()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    ld.close()
    for wrong in ((L2, 100), (IP, 50)):  # a caller's mistake is an error, never a wrongly sized export
        with pytest.raises(ValueError):
            capi.SqIndex.load_io(store, *wrong)
    ix.close()
