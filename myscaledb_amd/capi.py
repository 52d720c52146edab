"""ctypes binding of libmsvs.so (include/msvs.h).  Plumbing only -- no compute happens here.

Fails loudly when the library is missing: there is deliberately no fallback path.
"""
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmsvs.so")

METRIC_L2, METRIC_IP, METRIC_COSINE, METRIC_HAMMING, METRIC_JACCARD = 0, 1, 2, 3, 4
INDEX_FLAT, INDEX_IVFFLAT = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
MAX_K = 256
REFINE_MAX_CAND = 1024  # MSVS_REFINE_MAX_CAND: candidates per query of refine()
ROWS_DEVICE, ROWS_HOST_PINNED = 0, 1  # msvs_rows_placement
MAX_K_ROUNDS = 4096  # MSVS_MAX_K_ROUNDS: the BM25, device-fusion and (non-sharded) vector searches go this far in exact rounds
METRICS = {"L2": METRIC_L2, "IP": METRIC_IP, "Cosine": METRIC_COSINE, "COSINE": METRIC_COSINE, "cosine": METRIC_COSINE}

OK, ERR_INVALID_ARGUMENT, ERR_NOT_IMPLEMENTED, ERR_DEVICE, ERR_OOM, ERR_NOT_READY, ERR_UNSUPPORTED_K, ERR_ID_RANGE, \
    ERR_IO = range(9)
ERR_ABORTED = 236  # MSVS_ERR_ABORTED: a build cancelled through Index.set_cancel
CANCEL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)

SYMBOLS = [
    "msvs_last_error", "msvs_version", "msvs_device_count", "msvs_set_device", "msvs_device_synchronize",
    "msvs_knn_f32", "msvs_normalize_f32", "msvs_index_create", "msvs_index_free", "msvs_index_train",
    "msvs_index_set_centroids", "msvs_index_set_cancel", "msvs_index_add", "msvs_index_build", "msvs_index_ready", "msvs_index_num_data",
    "msvs_index_num_lists", "msvs_index_memory_usage", "msvs_index_search", "msvs_index_search_device",
    "msvs_index_export", "msvs_index_export_list", "msvs_index_list_stats", "msvs_index_serialize", "msvs_index_load", "msvs_merge_topk", "msvs_merge_topk_device",
    "msvs_postings_create", "msvs_postings_create_fields", "msvs_postings_set_alive", "msvs_postings_free",
    "msvs_bm25_search", "msvs_bm25_search_batch", "msvs_bm25_search_batch_device", "msvs_bm25_stats",
    "msvs_release_scratch", "msvs_filter_from_bits", "msvs_filter_from_offsets", "msvs_filter_from_predicate", "msvs_filter_combine", "msvs_filter_count",
    "msvs_filter_to_bits", "msvs_filter_free", "msvs_index_search_filter", "msvs_index_search_filter_device", "msvs_index_scanned_rows",
    "msvs_profile_enable", "msvs_profile_get", "msvs_profile_reset", "msvs_merge_topk_device_strided",
    "msvs_knn_f32_filtered", "msvs_prefilter_stats", "msvs_coarse_stats", "msvs_combine_stats", "msvs_set_option", "msvs_index_serialize_io",
    "msvs_index_load_io", "msvs_index_version", "msvs_index_resource_usage", "msvs_knn_bin",
    "msvs_cache_create", "msvs_cache_free", "msvs_block_upload", "msvs_block_lookup", "msvs_block_release", "msvs_block_info", "msvs_bin_index_create", "msvs_bin_index_free",
    "msvs_bin_index_add", "msvs_bin_index_num_data", "msvs_bin_index_search", "msvs_bin_index_serialize_io", "msvs_bin_index_load_io",
    "msvs_bin_index_create_ivf", "msvs_bin_index_train", "msvs_bin_index_set_centroids", "msvs_bin_index_num_lists",
    "msvs_bin_index_search_params", "msvs_bin_index_export",
    "msvs_knn_bin_rounds", "msvs_bin_index_search_rounds", "msvs_bin_index_search_device", "msvs_bin_index_search_rounds_device",
    "msvs_sq_index_create", "msvs_sq_index_free", "msvs_sq_index_train", "msvs_sq_index_set_codebook", "msvs_sq_index_add",
    "msvs_sq_index_build", "msvs_sq_index_ready", "msvs_sq_index_num_data", "msvs_sq_index_num_lists", "msvs_sq_index_memory_usage",
    "msvs_sq_index_search", "msvs_sq_index_search_device", "msvs_sq_index_export", "msvs_sq_index_serialize_io", "msvs_sq_index_load_io",
    "msvs_sq_index_bit_size",
    "msvs_pq_index_create", "msvs_pq_index_free", "msvs_pq_index_train", "msvs_pq_index_set_codebook", "msvs_pq_index_add",
    "msvs_pq_index_build", "msvs_pq_index_ready", "msvs_pq_index_num_data", "msvs_pq_index_num_lists", "msvs_pq_index_memory_usage",
    "msvs_pq_index_bit_size", "msvs_pq_index_query_tables", "msvs_pq_index_export_row_terms",
    "msvs_pq_index_search", "msvs_pq_index_search_device", "msvs_pq_index_export", "msvs_pq_index_serialize_io", "msvs_pq_index_load_io",
    "msvs_rows_create", "msvs_rows_append", "msvs_rows_num", "msvs_rows_dim", "msvs_rows_normalized", "msvs_rows_memory_usage",
    "msvs_rows_free", "msvs_refine", "msvs_refine_device", "msvs_sq_index_search_refine", "msvs_sq_index_search_refine_device",
    "msvs_pq_index_search_refine", "msvs_pq_index_search_refine_device",
    "msvs_sq_index_search_rounds", "msvs_sq_index_search_rounds_device", "msvs_sq_index_search_refine_rounds",
    "msvs_sq_index_search_refine_rounds_device", "msvs_pq_index_search_rounds", "msvs_pq_index_search_rounds_device",
    "msvs_pq_index_search_refine_rounds", "msvs_pq_index_search_refine_rounds_device",
    "msvs_cache_evict", "msvs_cache_stats", "msvs_knn_resident", "msvs_index_set_delete_bitmap",
    "msvs_index_set_merged_maps", "msvs_comm_unique_id", "msvs_comm_init", "msvs_comm_init_custom",
    "msvs_comm_free", "msvs_comm_all_reduce_u64", "msvs_comm_rank", "msvs_comm_size", "msvs_shard_search_device", "msvs_shard_search_device_async", "msvs_shard_search_drain", "msvs_shard_search_routed_device",
    "msvs_shard_search_routed_filtered_device", "msvs_shard_search_routed_device_async",
    "msvs_hybrid_fuse_device",
]


class MsvsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("msvs error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmsvs.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "-- there is no CPU fallback" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.msvs_last_error.restype = C.c_char_p
        _lib.msvs_version.restype = C.c_char_p
        for n in ("msvs_index_num_data", "msvs_index_num_lists", "msvs_index_memory_usage"):
            getattr(_lib, n).restype = C.c_size_t
            getattr(_lib, n).argtypes = [C.c_void_p]
        _lib.msvs_index_free.argtypes = [C.c_void_p]
        _lib.msvs_index_free.restype = None
        _lib.msvs_postings_free.argtypes = [C.c_void_p]
        _lib.msvs_postings_free.restype = None
        _lib.msvs_index_ready.argtypes = [C.c_void_p]
    return _lib


def _check(rc):
    if rc != 0:
        raise MsvsError(rc, lib().msvs_last_error().decode())


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def pack_bits(mask):
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    padded = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    padded[:n] = mask
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy()


def version():
    return lib().msvs_version().decode()


def device_count():
    n = C.c_int(0)
    _check(lib().msvs_device_count(C.byref(n)))
    return n.value


def set_device(i):
    _check(lib().msvs_set_device(int(i)))


def synchronize():
    _check(lib().msvs_device_synchronize())


def profile_enable(on):
    _check(lib().msvs_profile_enable(int(bool(on))))


def profile_reset():
    _check(lib().msvs_profile_reset())


def profile_get(name):
    """-> (calls, total_ms) of the kernel family `name` since the last reset (synchronises)."""
    c, t = C.c_uint64(0), C.c_double(0)
    _check(lib().msvs_profile_get(name.encode(), C.byref(c), C.byref(t)))
    return c.value, t.value


def set_option(name, value=None):
    """Experiment / test knob (msvs_set_option): value None restores the default."""
    _check(lib().msvs_set_option(name.encode(), None if value is None else str(value).encode()))


def prefilter_stats():
    """-> (queries, fallbacks) of the matrix-core candidate pass on the current device (msvs_prefilter_stats)."""
    q, f = C.c_uint64(0), C.c_uint64(0)
    _check(lib().msvs_prefilter_stats(C.byref(q), C.byref(f)))
    return q.value, f.value


def combine_stats():
    """-> (calls, batches, batched queries) of msvs_index_search's combining front end (msvs_combine_stats)."""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().msvs_combine_stats(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def coarse_stats():
    """-> (queries, fallbacks) of the coarse quantiser's candidate passes on the current device (msvs_coarse_stats)."""
    q, f = C.c_uint64(0), C.c_uint64(0)
    _check(lib().msvs_coarse_stats(C.byref(q), C.byref(f)))
    return q.value, f.value


def knn(x, y, k, metric, alive=None):
    """msvs_knn_f32 / msvs_knn_f32_filtered (seam A2).  x [nx,d], y [ny,d] host arrays, alive bool[ny] or None
    -> (ids int64 [nx,k], dis f32 [nx,k])."""
    y = _f32(y)
    d = y.shape[1]
    x = _f32(x).reshape(-1, d)
    nx = x.shape[0]
    ids = np.empty((nx, k), np.int64)
    dis = np.empty((nx, k), np.float32)
    if alive is None:
        _check(lib().msvs_knn_f32(_p(x, C.c_float), _p(y, C.c_float), C.c_size_t(d), C.c_size_t(k), C.c_size_t(nx),
                                  C.c_size_t(y.shape[0]), int(metric), _p(ids, C.c_int64), _p(dis, C.c_float)))
    else:
        bits = pack_bits(alive)
        _check(lib().msvs_knn_f32_filtered(_p(x, C.c_float), _p(y, C.c_float), C.c_size_t(d), C.c_size_t(k),
                                           C.c_size_t(nx), C.c_size_t(y.shape[0]), int(metric), _p(bits, C.c_uint64),
                                           _p(ids, C.c_int64), _p(dis, C.c_float)))
    return ids, dis


def knn_bin(x, y, k, metric, alive=None, _entry="msvs_knn_bin"):
    """msvs_knn_bin: x [nx, nbytes], y [ny, nbytes] uint8 host arrays -> (ids int64 [nx, k], dis f32 [nx, k])."""
    y = np.ascontiguousarray(y, np.uint8)
    nb = y.shape[1]
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, nb)
    nx = x.shape[0]
    ids = np.empty((nx, k), np.int64)
    dis = np.empty((nx, k), np.float32)
    bits = None if alive is None else pack_bits(alive)
    _check(getattr(lib(), _entry)(_p(x, C.c_uint8), _p(y, C.c_uint8), C.c_size_t(nb), C.c_size_t(k), C.c_size_t(nx),
                                  C.c_size_t(y.shape[0]), int(metric), _p(bits, C.c_uint64), _p(ids, C.c_int64),
                                  _p(dis, C.c_float)))
    return ids, dis


def knn_bin_rounds(x, y, k, metric, alive=None):
    """msvs_knn_bin_rounds: knn_bin with k <= MAX_K_ROUNDS (beyond MAX_K the scan runs once per MAX_K ranks)."""
    return knn_bin(x, y, k, metric, alive, _entry="msvs_knn_bin_rounds")


class BinIndex:
    """msvs_bin_index_t: BinaryFLAT over rows resident on the device (labels = ids given at add, filter indexed by label);
    with params ("ncentroids=N[,niter=I]") the partitioned form: centroids + list-major rows, searched by probing."""

    def __init__(self, nbytes, metric, params=None, _handle=None):
        self._h = C.c_void_p()
        self.nbytes = int(nbytes)
        if _handle is not None:
            self._h = _handle
        elif params is None:
            _check(lib().msvs_bin_index_create(C.c_size_t(nbytes), int(metric), C.byref(self._h)))
        else:
            _check(lib().msvs_bin_index_create_ivf(C.c_size_t(nbytes), int(metric), params.encode(), C.byref(self._h)))

    def train(self, rows):
        rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, self.nbytes)
        _check(lib().msvs_bin_index_train(self._h, _p(rows, C.c_uint8), C.c_size_t(rows.shape[0])))

    def set_centroids(self, centroids):
        c = np.ascontiguousarray(centroids, np.uint8).reshape(-1, self.nbytes)
        _check(lib().msvs_bin_index_set_centroids(self._h, _p(c, C.c_uint8), C.c_size_t(c.shape[0])))

    def add(self, rows, ids=None):
        rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, self.nbytes)
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int64)
            idp = _p(ids, C.c_int64)
        _check(lib().msvs_bin_index_add(self._h, _p(rows, C.c_uint8), idp, C.c_size_t(rows.shape[0])))

    @property
    def num_data(self):
        lib().msvs_bin_index_num_data.restype = C.c_size_t
        return lib().msvs_bin_index_num_data(self._h)

    @property
    def num_lists(self):
        """0 for a flat index."""
        lib().msvs_bin_index_num_lists.restype = C.c_size_t
        return lib().msvs_bin_index_num_lists(self._h)

    def search(self, x, k, alive=None, params=None, nbits=None):
        """params: "nprobe=P" (partitioned index; None = msvs_bin_index_search); alive: bool over labels, nbits: how many of
        them the filter covers (default all of `alive`): labels at or beyond nbits are dead."""
        x = np.ascontiguousarray(x, np.uint8).reshape(-1, self.nbytes)
        ids = np.empty((x.shape[0], k), np.int64)
        dis = np.empty((x.shape[0], k), np.float32)
        bits = None if alive is None else pack_bits(alive)
        nb = C.c_size_t(0 if alive is None else (len(alive) if nbits is None else int(nbits)))
        if params is None:
            _check(lib().msvs_bin_index_search(self._h, _p(x, C.c_uint8), C.c_size_t(x.shape[0]), C.c_size_t(k), _p(bits, C.c_uint64),
                                               nb, _p(ids, C.c_int64), _p(dis, C.c_float)))
        else:
            _check(lib().msvs_bin_index_search_params(self._h, _p(x, C.c_uint8), C.c_size_t(x.shape[0]), C.c_size_t(k), params.encode(),
                                                      _p(bits, C.c_uint64), nb, _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_rounds(self, x, k, alive=None, params=None, nbits=None):
        """search with k <= MAX_K_ROUNDS (msvs_bin_index_search_rounds): beyond MAX_K the scan runs once per MAX_K ranks.
        params: None, "" or "nprobe=P"."""
        x = np.ascontiguousarray(x, np.uint8).reshape(-1, self.nbytes)
        ids = np.empty((x.shape[0], k), np.int64)
        dis = np.empty((x.shape[0], k), np.float32)
        bits = None if alive is None else pack_bits(alive)
        nb = C.c_size_t(0 if alive is None else (len(alive) if nbits is None else int(nbits)))
        _check(lib().msvs_bin_index_search_rounds(self._h, _p(x, C.c_uint8), C.c_size_t(x.shape[0]), C.c_size_t(k),
                                                  None if params is None else params.encode(), _p(bits, C.c_uint64), nb,
                                                  _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_device(self, d_x, nx, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0, _entry="msvs_bin_index_search_device"):
        """msvs_bin_index_search_device: all buffers are raw device addresses (ints; d_x: nx dense rows of nbytes); enqueues on
        `stream` and returns (the first search after an add builds the device image and synchronises the stream)."""
        _check(getattr(lib(), _entry)(self._h, C.c_void_p(int(d_x)) if d_x else None, C.c_size_t(nx), C.c_size_t(k), C.c_size_t(nprobe),
                                      C.c_void_p(int(d_alive)) if d_alive else None, C.c_size_t(nbits),
                                      C.c_void_p(int(d_ids)) if d_ids else None, C.c_void_p(int(d_dis)) if d_dis else None,
                                      C.c_void_p(int(stream)) if stream else None))

    def search_rounds_device(self, d_x, nx, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """search_device with k <= MAX_K_ROUNDS (msvs_bin_index_search_rounds_device)."""
        self.search_device(d_x, nx, k, nprobe, d_ids, d_dis, stream, d_alive, nbits, _entry="msvs_bin_index_search_rounds_device")

    def export(self):
        """Partitioned index -> (centroids [nlist, nbytes], list offsets [nlist + 1], rows and labels in list-major order)."""
        n, nl = self.num_data, self.num_lists
        cent = np.empty((nl, self.nbytes), np.uint8)
        off = np.empty(nl + 1, np.int64)
        rows = np.empty((n, self.nbytes), np.uint8)
        labels = np.empty(n, np.int64)
        _check(lib().msvs_bin_index_export(self._h, _p(cent, C.c_uint8), _p(off, C.c_int64), _p(rows, C.c_uint8), _p(labels, C.c_int64)))
        return cent, off, rows, labels

    def serialize_io(self, store):
        """msvs_bin_index_serialize_io through stream callbacks; `store` = dict NAME -> bytearray (filled in)."""
        _check(lib().msvs_bin_index_serialize_io(self._h, C.byref(_DictIO(store).io)))

    @classmethod
    def load_io(cls, store, nbytes, metric):
        h = C.c_void_p()
        _check(lib().msvs_bin_index_load_io(C.byref(_DictIO(store).io), C.byref(h)))
        return cls(nbytes, metric, _handle=h)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_bin_index_free.argtypes = [C.c_void_p]
            _lib.msvs_bin_index_free.restype = None
            _lib.msvs_bin_index_free(self._h)
            self._h = None

    __del__ = close


class _CodedIndex:
    """What SqIndex and PqIndex share: the handle and every call that differs only in the C prefix (`_c`)."""
    _c = None  # "msvs_sq_index" / "msvs_pq_index"

    def _fn(self, name):
        return getattr(lib(), "%s_%s" % (self._c, name))

    def _size(self, name):
        fn = self._fn(name)
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_void_p]
        return fn(self._h)

    @staticmethod
    def _dev(a):
        """a raw device address (int; 0 / None: null) as a pointer argument"""
        return C.c_void_p(int(a)) if a else None

    def train(self, x, n=None, mem=MEM_HOST):
        """mem=MEM_DEVICE: `x` is a raw device address (int) of n dense rows."""
        if mem == MEM_DEVICE:
            _check(self._fn("train")(self._h, self._dev(x), C.c_size_t(n), mem))
            return
        x = _f32(x).reshape(-1, self.dim)
        _check(self._fn("train")(self._h, _p(x, C.c_float), C.c_size_t(x.shape[0]), MEM_HOST))

    def add(self, x, ids=None, n=None, mem=MEM_HOST):
        """mem=MEM_DEVICE: `x` and `ids` (None: the staging positions) are raw device addresses (ints) of n rows / labels."""
        if mem == MEM_DEVICE:
            _check(self._fn("add")(self._h, self._dev(x), self._dev(ids), C.c_size_t(n), mem))
            return
        x = _f32(x).reshape(-1, self.dim)
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int64)
        _check(self._fn("add")(self._h, _p(x, C.c_float), _p(ids, C.c_int64), C.c_size_t(x.shape[0]), MEM_HOST))

    def build(self):
        _check(self._fn("build")(self._h))

    @property
    def ready(self):
        fn = self._fn("ready")
        fn.argtypes = [C.c_void_p]
        return bool(fn(self._h))

    @property
    def num_data(self):
        return self._size("num_data")

    @property
    def num_lists(self):
        return self._size("num_lists")

    @property
    def memory_usage(self):
        return self._size("memory_usage")

    def search(self, queries, k, params="", alive=None, nbits=None, _entry="search"):
        """params: "nprobe=P"; alive: bool over labels, nbits: how many of them the filter covers (default all of `alive`)."""
        q = _f32(queries).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), np.int64)
        dis = np.empty((q.shape[0], k), np.float32)
        bits = None if alive is None else pack_bits(alive)
        nb = C.c_size_t(0 if alive is None else (len(alive) if nbits is None else int(nbits)))
        _check(self._fn(_entry)(self._h, _p(q, C.c_float), C.c_size_t(q.shape[0]), C.c_size_t(k), params.encode(),
                                _p(bits, C.c_uint64), nb, _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_device(self, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0, _entry="search_device"):
        """All arguments are raw device addresses (ints); enqueues on `stream` and returns immediately."""
        _check(self._fn(_entry)(self._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), C.c_size_t(k), C.c_size_t(nprobe),
                                C.c_void_p(int(d_alive)) if d_alive else None, C.c_size_t(nbits),
                                C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                C.c_void_p(int(stream)) if stream else None))

    def search_refine(self, rows, queries, k, kc, params="", alive=None, nbits=None, _entry="search_refine"):
        """The two-stage search: search(kc)'s labels scored against `rows` (a Rows whose row i is label i), the best k with the
        canonical distances.  params, alive and nbits are search's and apply to the first stage."""
        q = _f32(queries).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), np.int64)
        dis = np.empty((q.shape[0], k), np.float32)
        bits = None if alive is None else pack_bits(alive)
        nb = C.c_size_t(0 if alive is None else (len(alive) if nbits is None else int(nbits)))
        _check(self._fn(_entry)(self._h, rows._h, _p(q, C.c_float), C.c_size_t(q.shape[0]), C.c_size_t(k), C.c_size_t(kc),
                                params.encode(), _p(bits, C.c_uint64), nb, _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_refine_device(self, rows, d_queries, nq, k, kc, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0,
                             _entry="search_refine_device"):
        """search_refine with raw device addresses (ints); enqueues both stages on `stream` and returns immediately."""
        _check(self._fn(_entry)(self._h, rows._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), C.c_size_t(k), C.c_size_t(kc),
                                C.c_size_t(nprobe), self._dev(d_alive), C.c_size_t(nbits), C.c_void_p(int(d_ids)),
                                C.c_void_p(int(d_dis)), self._dev(stream)))

    def search_rounds(self, queries, k, params="", alive=None, nbits=None):
        """search with k <= MAX_K_ROUNDS: beyond MAX_K the list scan runs once per MAX_K ranks (msvs_*_index_search_rounds)."""
        return self.search(queries, k, params, alive, nbits, _entry="search_rounds")

    def search_rounds_device(self, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """search_device with k <= MAX_K_ROUNDS."""
        self.search_device(d_queries, nq, k, nprobe, d_ids, d_dis, stream, d_alive, nbits, _entry="search_rounds_device")

    def search_refine_rounds(self, rows, queries, k, kc, params="", alive=None, nbits=None):
        """search_refine with kc <= REFINE_MAX_CAND: the first stage is search_rounds(kc)."""
        return self.search_refine(rows, queries, k, kc, params, alive, nbits, _entry="search_refine_rounds")

    def search_refine_rounds_device(self, rows, d_queries, nq, k, kc, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """search_refine_device with kc <= REFINE_MAX_CAND."""
        self.search_refine_device(rows, d_queries, nq, k, kc, nprobe, d_ids, d_dis, stream, d_alive, nbits,
                                  _entry="search_refine_rounds_device")

    def serialize_io(self, store):
        """msvs_{sq,pq}_index_serialize_io through stream callbacks; `store` = dict NAME -> bytearray (filled in)."""
        _check(self._fn("serialize_io")(self._h, C.byref(_DictIO(store).io)))

    @classmethod
    def _load(cls, store, file, fmt):
        """-> (handle, the fields `fmt` at byte 12 of the data file's header).  The geometry comes from that header (which the
        load has validated, check word included), never from the caller: export() sizes its buffers by it."""
        h = C.c_void_p()
        _check(getattr(lib(), cls._c + "_load_io")(C.byref(_DictIO(store).io), C.byref(h)))
        return h, struct.unpack_from(fmt, bytes(store[file][:12 + struct.calcsize(fmt)]), 12)

    def _agree(self, kind, **wanted):
        """a loaded index whose geometry the caller also gave: it must be the file's (else closed, ValueError)"""
        for name, want in wanted.items():
            have = getattr(self, name)
            if want is not None and int(want) != have:
                self.close()
                raise ValueError("the %s index file has %s = %d, the caller expects %d" % (kind, name, have, int(want)))
        return self

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            fn = getattr(_lib, self._c + "_free")
            fn.argtypes = [C.c_void_p]
            fn.restype = None
            fn(self._h)
            self._h = None

    __del__ = close


class SqIndex(_CodedIndex):
    """msvs_sq_index_t: the IVFSQ index -- coarse centroids, one per-dimension 8-bit quantiser of the residuals, and per row its
    list, label and dim code bytes (no f32 row is kept).  params as Index's for IVFFLAT ("ncentroids=N,kmeans_iters=I,...") and,
    optionally, bit_size: 4 (4-bit codes) or 16 (binary16 residuals).  .bits is the index's own answer (msvs_sq_index_bit_size): 4,
    8 or 16."""
    _c = "msvs_sq_index"

    def __init__(self, metric, dim, params="", _handle=None):
        self.metric, self.dim = int(metric), int(dim)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _check(lib().msvs_sq_index_create(int(metric), C.c_size_t(dim), params.encode(), C.byref(self._h)))
        self.bits = self._size("bit_size")

    def set_codebook(self, centroids, vmin, vmax, nlist=None, mem=MEM_HOST):
        """mem=MEM_DEVICE: centroids, vmin and vmax are raw device addresses (ints); nlist is the number of centroid rows."""
        if mem == MEM_DEVICE:
            _check(lib().msvs_sq_index_set_codebook(self._h, self._dev(centroids), C.c_size_t(nlist), self._dev(vmin), self._dev(vmax), mem))
            return
        c = _f32(centroids).reshape(-1, self.dim)
        lo, hi = _f32(vmin).reshape(self.dim), _f32(vmax).reshape(self.dim)
        _check(lib().msvs_sq_index_set_codebook(self._h, _p(c, C.c_float), C.c_size_t(c.shape[0]), _p(lo, C.c_float), _p(hi, C.c_float),
                                                MEM_HOST))

    def export(self, with_lists=True):
        """-> (centroids [nlist, dim], vmin [dim], vmax [dim], list offsets [nlist + 1], codes [n, dim] u8 in natural column order
        (bits 4: one code a byte; bits 16: uint16, the binary16 bit patterns), labels [n]) in list-major order; with_lists=False (an
        index not built yet): the codebook only, None for the rest."""
        nl, d = self.num_lists, self.dim
        cent = np.empty((nl, d), np.float32)
        lo, hi = np.empty(d, np.float32), np.empty(d, np.float32)
        off = codes = labels = None
        if with_lists:
            n = self.num_data
            off, codes, labels = np.empty(nl + 1, np.int64), np.empty((n, d), np.uint16 if self.bits == 16 else np.uint8), np.empty(n, np.int64)
        _check(lib().msvs_sq_index_export(self._h, _p(cent, C.c_float), _p(lo, C.c_float), _p(hi, C.c_float), _p(off, C.c_int64),
                                          None if codes is None else codes.ctypes.data_as(C.POINTER(C.c_uint8)), _p(labels, C.c_int64)))
        return cent, lo, hi, off, codes, labels

    @classmethod
    def load_io(cls, store, metric=None, dim=None, bits=None):
        """metric / dim come from the file (SqHeader: magic[8], u32 version, i32 metric, u64 dim, ...), bits from the loaded index;
        where given, they must agree with it (ValueError otherwise)."""
        h, (f_metric, f_dim) = cls._load(store, "sq_data", "<iQ")
        return cls(f_metric, f_dim, _handle=h)._agree("IVFSQ", metric=metric, dim=dim, bits=bits)


class PqIndex(_CodedIndex):
    """msvs_pq_index_t: the IVFPQ index -- coarse centroids, m sub-codebooks of 256 entries (16 with bit_size=4) over the residuals,
    and per row its list, label and m codes (no f32 row is kept).  params as Index's for IVFFLAT plus m and, optionally, bit_size
    ("ncentroids=N,m=M,bit_size=4,kmeans_iters=I,...").  .bits is the index's own answer (msvs_pq_index_bit_size): 4 or 8."""
    _c = "msvs_pq_index"

    def __init__(self, metric, dim, params="", _handle=None, _m=None):
        self.metric, self.dim = int(metric), int(dim)
        self._h = C.c_void_p()
        if _handle is not None:
            self._h, self.m = _handle, int(_m)
        else:
            _check(lib().msvs_pq_index_create(int(metric), C.c_size_t(dim), params.encode(), C.byref(self._h)))
            self.m = int(dict(kv.split("=", 1) for kv in params.replace(" ", "").split(",") if "=" in kv)["m"])
        self.bits = self._size("bit_size")
        fn = lib().msvs_pq_index_query_tables
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        self.query_tables = int(fn(self._h))  # 1: tables that depend on the query alone (create's query_tables=1, or the file's form)

    def export_row_terms(self):
        """-> w [n] f32 in list-major order (export's): the row terms of an L2 index with query_tables=1; MsvsError for any other."""
        w = np.empty(self.num_data, np.float32)
        _check(lib().msvs_pq_index_export_row_terms(self._h, _p(w, C.c_float)))
        return w

    def set_codebook(self, centroids, codebooks, nlist=None, mem=MEM_HOST):
        """codebooks: [m, 1 << bits, dim / m]; mem=MEM_DEVICE: both are raw device addresses (ints), nlist the number of centroid rows."""
        if mem == MEM_DEVICE:
            _check(lib().msvs_pq_index_set_codebook(self._h, self._dev(centroids), C.c_size_t(nlist), self._dev(codebooks), mem))
            return
        c = _f32(centroids).reshape(-1, self.dim)
        cb = _f32(codebooks).reshape(self.m, 1 << self.bits, self.dim // self.m)
        _check(lib().msvs_pq_index_set_codebook(self._h, _p(c, C.c_float), C.c_size_t(c.shape[0]), _p(cb, C.c_float), MEM_HOST))

    def export(self, with_lists=True):
        """-> (centroids [nlist, dim], codebooks [m, 1 << bits, dim / m], list offsets [nlist + 1], codes [n, m] u8 in natural order
        (one code a byte), labels [n]) in list-major order; with_lists=False (an index not built yet): the codebook only, None for
        the rest."""
        nl, d, m = self.num_lists, self.dim, self.m
        cent = np.empty((nl, d), np.float32)
        cb = np.empty((m, 1 << self.bits, d // m), np.float32)
        off = codes = labels = None
        if with_lists:
            n = self.num_data
            off, codes, labels = np.empty(nl + 1, np.int64), np.empty((n, m), np.uint8), np.empty(n, np.int64)
        _check(lib().msvs_pq_index_export(self._h, _p(cent, C.c_float), _p(cb, C.c_float), _p(off, C.c_int64), _p(codes, C.c_uint8),
                                          _p(labels, C.c_int64)))
        return cent, cb, off, codes, labels

    @classmethod
    def load_io(cls, store, metric=None, dim=None, m=None, bits=None, query_tables=None):
        """metric / dim / m come from the file (PqHeader: magic[8], u32 version, i32 metric, u64 dim, u64 m, ...), bits and
        query_tables from the loaded index; where given, they must agree with it (ValueError otherwise)."""
        h, (f_metric, f_dim, f_m) = cls._load(store, "pq_data", "<iQQ")
        return cls(f_metric, f_dim, _handle=h, _m=f_m)._agree("IVFPQ", metric=metric, dim=dim, m=m, bits=bits, query_tables=query_tables)


class Rows:
    """msvs_rows_t: the row store of a two-stage search -- an append-only table of f32 rows in which row i is label i, in device
    memory (ROWS_DEVICE) or in mapped pinned host memory (ROWS_HOST_PINNED).  normalize=True stores normalize()'s rows (cosine)."""

    def __init__(self, dim, capacity, normalize=False, placement=ROWS_DEVICE):
        self.dim = int(dim)
        self._h = C.c_void_p()
        _check(lib().msvs_rows_create(C.c_size_t(dim), int(bool(normalize)), int(placement), C.c_size_t(capacity), C.byref(self._h)))
        self.placement, self.capacity = int(placement), int(capacity)

    def append(self, x, n=None, mem=MEM_HOST):
        """mem=MEM_DEVICE: `x` is a raw device address (int) of n dense rows."""
        if mem == MEM_DEVICE:
            _check(lib().msvs_rows_append(self._h, C.c_void_p(int(x)) if x else None, C.c_size_t(n), mem))
            return
        x = _f32(x).reshape(-1, self.dim)
        _check(lib().msvs_rows_append(self._h, _p(x, C.c_float), C.c_size_t(x.shape[0]), MEM_HOST))

    def _size(self, name):
        fn = getattr(lib(), "msvs_rows_" + name)
        fn.restype, fn.argtypes = C.c_size_t, [C.c_void_p]
        return fn(self._h)

    @property
    def num(self):
        return self._size("num")

    @property
    def normalized(self):
        fn = lib().msvs_rows_normalized
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return bool(fn(self._h))

    @property
    def memory_usage(self):
        """device bytes: the table of a ROWS_DEVICE store, 0 for a pinned one"""
        return self._size("memory_usage")

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_rows_free.argtypes = [C.c_void_p]
            _lib.msvs_rows_free.restype = None
            _lib.msvs_rows_free(self._h)
            self._h = None

    __del__ = close


def refine(rows, metric, queries, cand, k):
    """msvs_refine: cand [nq, kc] labels (int64; < 0 and >= rows.num are skipped) scored against rows -> (ids [nq, k], dis [nq, k])."""
    q = _f32(queries).reshape(-1, rows.dim)
    cand = np.ascontiguousarray(cand, np.int64)
    if cand.ndim != 2:
        cand = cand.reshape(q.shape[0], -1)
    ids = np.empty((q.shape[0], k), np.int64)
    dis = np.empty((q.shape[0], k), np.float32)
    _check(lib().msvs_refine(rows._h, int(metric), _p(q, C.c_float), C.c_size_t(q.shape[0]), _p(cand, C.c_int64), C.c_size_t(cand.shape[1]),
                             C.c_size_t(k), _p(ids, C.c_int64), _p(dis, C.c_float)))
    return ids, dis


def refine_device(rows, metric, d_queries, nq, d_cand, kc, k, d_ids, d_dis, stream=0):
    """msvs_refine_device: all buffers are raw device addresses (ints); enqueues on `stream` and returns immediately."""
    _check(lib().msvs_refine_device(rows._h, int(metric), C.c_void_p(int(d_queries)), C.c_size_t(nq), C.c_void_p(int(d_cand)) if d_cand else None,
                                    C.c_size_t(kc), C.c_size_t(k), C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                    C.c_void_p(int(stream)) if stream else None))


def normalize(x):
    x = _f32(x).copy()
    x2 = x.reshape(-1, x.shape[-1])
    _check(lib().msvs_normalize_f32(_p(x2, C.c_float), C.c_size_t(x2.shape[0]), C.c_size_t(x2.shape[1])))
    return x


def merge_topk(ids, dis, metric):
    """ids/dis [nparts, nq, k] host arrays -> merged (ids [nq,k], dis [nq,k])."""
    ids = np.ascontiguousarray(ids, np.int64)
    dis = _f32(dis)
    nparts, nq, k = ids.shape
    oi, od = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
    _check(lib().msvs_merge_topk(_p(ids, C.c_int64), _p(dis, C.c_float), C.c_size_t(nparts), C.c_size_t(nq),
                                 C.c_size_t(k), int(metric), _p(oi, C.c_int64), _p(od, C.c_float)))
    return oi, od


class Cache:
    """msvs_cache_t: LRU of resident brute-force blocks (seam A2)."""

    def __init__(self, capacity_bytes):
        h = C.c_void_p()
        _check(lib().msvs_cache_create(C.c_size_t(capacity_bytes), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_cache_free.argtypes = [C.c_void_p]
            _lib.msvs_cache_free.restype = None
            _lib.msvs_cache_free(self._h)
            self._h = None

    __del__ = close

    def upload(self, key, mark, rows, normalize=False):
        rows = _f32(rows)
        b = C.c_void_p()
        _check(lib().msvs_block_upload(self._h, key.encode(), C.c_uint64(mark), _p(rows, C.c_float),
                                       C.c_size_t(rows.shape[0]), C.c_size_t(rows.shape[1]), int(normalize), C.byref(b)))
        return b

    def lookup(self, key, mark):
        b = C.c_void_p()
        _check(lib().msvs_block_lookup(self._h, key.encode(), C.c_uint64(mark), C.byref(b)))
        return b if b.value else None

    @staticmethod
    def release(block):
        lib().msvs_block_release.argtypes = [C.c_void_p]
        lib().msvs_block_release.restype = None
        lib().msvs_block_release(block)

    def evict(self, prefix):
        n = C.c_size_t(0)
        _check(lib().msvs_cache_evict(self._h, prefix.encode(), C.byref(n)))
        return n.value

    def stats(self):
        """-> dict(bytes, blocks, hits, misses, evictions)"""
        by, bl = C.c_size_t(0), C.c_size_t(0)
        h, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().msvs_cache_stats(self._h, C.byref(by), C.byref(bl), C.byref(h), C.byref(m), C.byref(e)))
        return dict(bytes=by.value, blocks=bl.value, hits=h.value, misses=m.value, evictions=e.value)


def knn_resident(block, x, k, metric, d, alive=None):
    x = _f32(x).reshape(-1, d)
    nx = x.shape[0]
    ids = np.empty((nx, k), np.int64)
    dis = np.empty((nx, k), np.float32)
    bits = None if alive is None else pack_bits(alive)
    _check(lib().msvs_knn_resident(block, _p(x, C.c_float), C.c_size_t(k), C.c_size_t(nx), int(metric),
                                   _p(bits, C.c_uint64), _p(ids, C.c_int64), _p(dis, C.c_float)))
    return ids, dis


COMM_ID_BYTES = 128
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def comm_unique_id():
    """msvs_comm_unique_id (rank 0): the bytes every rank needs for Comm(id=...)."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _check(lib().msvs_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """msvs_comm_t: RCCL communicator owned by libmsvs (id = bytes from comm_unique_id()), or a caller-supplied
    all-gather (all_gather = python callable(d_send, d_recv, nbytes, stream) -> 0) for tests."""

    def __init__(self, nranks, rank, id=None, all_gather=None):
        h = C.c_void_p()
        self._cb = None
        if all_gather is not None:
            self._cb = ALLGATHER_FN(lambda ctx, s, r, n, st: int(all_gather(s, r, n, st) or 0))
            _check(lib().msvs_comm_init_custom(int(nranks), int(rank), self._cb, None, C.byref(h)))
        else:
            buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(id) if id is not None else None
            _check(lib().msvs_comm_init(buf, int(nranks), int(rank), C.byref(h)))
        self._h = h
        self.nranks, self.rank = nranks, rank

    def drain(self, stream=0):
        """msvs_shard_search_drain: `stream` waits for every batch of msvs_shard_search_device_async still in flight."""
        _check(lib().msvs_shard_search_drain(self._h, C.c_void_p(int(stream)) if stream else None))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_comm_free.argtypes = [C.c_void_p]
            _lib.msvs_comm_free.restype = None
            _lib.msvs_comm_free(self._h)
            self._h = None

    __del__ = close


class _MsvsIO(C.Structure):
    _fields_ = [("ctx", C.c_void_p),
                ("open", C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p, C.c_int)),
                ("write", C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)),
                ("read", C.CFUNCTYPE(C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)),
                ("close", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p))]


class _DictIO:
    """msvs_io_t over a dict NAME -> bytearray: stands in for the host's IDisk-backed streams in tests."""

    def __init__(self, store):
        self.store, self.streams, self.next = store, {}, 1

        def op(_ctx, name, write):
            name = name.decode()
            if write:
                self.store[name] = bytearray()
            elif name not in self.store:
                return None
            h = self.next
            self.next += 1
            self.streams[h] = [name, 0]
            return h

        def wr(_ctx, h, buf, n):
            self.store[self.streams[h][0]] += C.string_at(buf, n)
            return n

        def rd(_ctx, h, buf, n):
            name, pos = self.streams[h]
            data = self.store[name][pos:pos + n]
            C.memmove(buf, bytes(data), len(data))
            self.streams[h][1] = pos + len(data)
            return len(data)

        def cl(_ctx, h):
            self.streams.pop(h, None)
            return 0

        t = _MsvsIO
        self._keep = (t._fields_[1][1](op), t._fields_[2][1](wr), t._fields_[3][1](rd), t._fields_[4][1](cl))
        self.io = _MsvsIO(None, *self._keep)


def index_version():
    lib().msvs_index_version.restype = C.c_char_p
    return lib().msvs_index_version().decode()


class Index:
    """msvs_index_t (seam A1)."""

    def __init__(self, index_type, metric, dim, params="", _handle=None):
        self.dim = int(dim)
        self.metric = metric
        self.index_type = index_type
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        _check(lib().msvs_index_create(int(index_type), int(metric), C.c_size_t(dim), params.encode(), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_index_free(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _ptr(x, mem):
        if mem == MEM_DEVICE:
            return C.c_void_p(int(x))
        return x.ctypes.data_as(C.c_void_p)

    def train(self, x, n=None, mem=MEM_HOST):
        if mem == MEM_HOST:
            x = _f32(x)
            n = x.shape[0]
        _check(lib().msvs_index_train(self._h, self._ptr(x, mem), C.c_size_t(n), mem))

    def set_centroids(self, c):
        c = _f32(c)
        _check(lib().msvs_index_set_centroids(self._h, self._ptr(c, MEM_HOST), C.c_size_t(c.shape[0]), MEM_HOST))

    def add(self, x, ids=None, n=None, mem=MEM_HOST):
        if mem == MEM_HOST:
            x = _f32(x)
            n = x.shape[0]
            idp = None
            if ids is not None:
                ids = np.ascontiguousarray(ids, np.int64)
                idp = ids.ctypes.data_as(C.c_void_p)
        else:
            idp = None if ids is None else C.c_void_p(int(ids))
        _check(lib().msvs_index_add(self._h, self._ptr(x, mem), idp, C.c_size_t(n), mem))

    def build(self):
        _check(lib().msvs_index_build(self._h))

    def set_cancel(self, fn):
        """msvs_index_set_cancel: fn() is polled between the k-means iterations of train, at every add and at build; a true result
        makes that call raise MsvsError with ERR_ABORTED.  None clears it.  The C callback is kept alive on the object."""
        cb = None if fn is None else CANCEL_FN(lambda _ctx: 1 if fn() else 0)
        _check(lib().msvs_index_set_cancel(self._h, cb, None))
        self._cancel_cb = cb

    def export_list(self, l, length):
        """(vecs [length, dim] f32, ids [length] i64) of inverted list l (length from export(with_vecs=False)'s offsets)."""
        vecs = np.empty((length, self.dim), np.float32)
        ids = np.empty(length, np.int64)
        _check(lib().msvs_index_export_list(self._h, C.c_size_t(l), _p(vecs, C.c_float), _p(ids, C.c_int64)))
        return vecs, ids

    def list_stats(self):
        """{nlist, min_len, max_len, imbalance (nlist * sum(len^2) / n^2), train_empty} of a built IVFFLAT index."""
        nl, mn, mx, te = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        imb = C.c_double()
        _check(lib().msvs_index_list_stats(self._h, C.byref(nl), C.byref(mn), C.byref(mx), C.byref(imb), C.byref(te)))
        return {"nlist": nl.value, "min_len": mn.value, "max_len": mx.value, "imbalance": imb.value, "train_empty": te.value}

    @property
    def ready(self):
        return bool(lib().msvs_index_ready(self._h))

    @property
    def num_data(self):
        return lib().msvs_index_num_data(self._h)

    @property
    def num_lists(self):
        return lib().msvs_index_num_lists(self._h)

    @property
    def memory_usage(self):
        return lib().msvs_index_memory_usage(self._h)

    _search_fn = None  # msvs_index_search with integer-address argtypes (the unfiltered fast path below)

    def search(self, queries, k, params="", alive=None):
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        if alive is None:
            # host-pointer call without the per-argument ctypes pointer objects (1.8 us each: a third of the wrapper's overhead on a
            # 40 us single-query call): one result block, raw addresses
            fn = Index._search_fn
            if fn is None:
                fn = lib()["msvs_index_search"]
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
                fn.restype = C.c_int
                Index._search_fn = fn
            out = np.empty(nq * k * 12, np.uint8)
            base = C.addressof(C.c_char.from_buffer(out))
            try:
                qaddr = C.addressof(C.c_char.from_buffer(q))  # (0.3 us; .ctypes.data builds an interface object: 0.9 us)
            except (TypeError, ValueError):  # read-only or empty array
                qaddr = q.ctypes.data
            rc = fn(self._h, qaddr, nq, k, params.encode(), None, 0, base, base + nq * k * 8)
            if rc:
                _check(rc)
            return np.ndarray((nq, k), np.int64, out, 0), np.ndarray((nq, k), np.float32, out, nq * k * 8)
        ids = np.empty((nq, k), np.int64)
        dis = np.empty((nq, k), np.float32)
        bits, nbits = None, 0
        if alive is not None:
            nbits = len(alive)
            bits = pack_bits(alive)
        _check(lib().msvs_index_search(self._h, _p(q, C.c_float), C.c_size_t(nq), int(k), params.encode(),
                                       _p(bits, C.c_uint64), C.c_size_t(nbits), _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_filter(self, queries, k, params, flt):
        """msvs_index_search_filter: the library picks bit test or compacted view from the filter's population count."""
        q = _f32(queries).reshape(-1, self.dim)
        nq = q.shape[0]
        ids = np.empty((nq, k), np.int64)
        dis = np.empty((nq, k), np.float32)
        _check(lib().msvs_index_search_filter(self._h, _p(q, C.c_float), C.c_size_t(nq), int(k), params.encode(), flt._h,
                                              _p(ids, C.c_int64), _p(dis, C.c_float)))
        return ids, dis

    def search_filter_device(self, d_queries, nq, k, nprobe, flt, d_ids, d_dis, stream=0):
        _check(lib().msvs_index_search_filter_device(self._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), int(k), int(nprobe), flt._h,
                                                     C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                                     C.c_void_p(int(stream)) if stream else None))

    def search_device(self, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """All arguments are raw device addresses (ints); enqueues on `stream` and returns immediately."""
        _check(lib().msvs_index_search_device(self._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), int(k), int(nprobe),
                                              C.c_void_p(int(d_alive)) if d_alive else None, C.c_size_t(nbits),
                                              C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                              C.c_void_p(int(stream)) if stream else None))

    def shard_search_device(self, comm, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """msvs_shard_search_device: the whole sharded search (coarse by query + probe all-gather + local scan + packed
        all-gather + merge) on `stream`; raw device addresses."""
        _check(lib().msvs_shard_search_device(self._h, comm._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), int(k),
                                              int(nprobe), C.c_void_p(int(d_alive)) if d_alive else None,
                                              C.c_size_t(nbits), C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                              C.c_void_p(int(stream)) if stream else None))

    def shard_search_routed_device(self, comm, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """msvs_shard_search_routed[_filtered]_device: this rank's OWN nq queries (0 allowed), routed to the ranks that own lists they
        still need after the pre-pruning, searched there under that rank's filter (d_alive: THIS rank's bitmap); collective.  Returns
        the (query, rank) pairs this rank served."""
        served = C.c_uint64(0)
        q = C.c_void_p(int(d_queries)) if d_queries else None
        oi, od = C.c_void_p(int(d_ids)) if d_ids else None, C.c_void_p(int(d_dis)) if d_dis else None
        st = C.c_void_p(int(stream)) if stream else None
        if d_alive:
            _check(lib().msvs_shard_search_routed_filtered_device(self._h, comm._h, q, C.c_size_t(nq), int(k), int(nprobe), C.c_void_p(int(d_alive)),
                                                                  C.c_size_t(nbits), oi, od, st, C.byref(served)))
        else:
            _check(lib().msvs_shard_search_routed_device(self._h, comm._h, q, C.c_size_t(nq), int(k), int(nprobe), oi, od, st, C.byref(served)))
        return served.value

    def shard_search_routed_device_async(self, comm, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0, served=None,
                                         want_event=True):
        """msvs_shard_search_routed_device_async: two routed steps in flight.  Returns the done event of the PREVIOUS call's batch (None at
        the first call; never asked for with want_event=False: a caller that stays on one stream and drains at the end needs none, and an
        event record between two kernels is ~8 us of idle device); `served` (a ctypes c_uint64 the caller keeps alive) receives this
        batch's routed pairs when ITS back phase runs."""
        ev = C.c_void_p()
        _check(lib().msvs_shard_search_routed_device_async(self._h, comm._h, C.c_void_p(int(d_queries)) if d_queries else None, C.c_size_t(nq), int(k),
                                                           int(nprobe), C.c_void_p(int(d_alive)) if d_alive else None, C.c_size_t(nbits),
                                                           C.c_void_p(int(d_ids)) if d_ids else None, C.c_void_p(int(d_dis)) if d_dis else None,
                                                           C.c_void_p(int(stream)) if stream else None,
                                                           C.byref(served) if served is not None else None, C.byref(ev) if want_event else None))
        return ev.value

    def shard_search_device_async(self, comm, d_queries, nq, k, nprobe, d_ids, d_dis, stream=0, d_alive=0, nbits=0):
        """msvs_shard_search_device_async: two batches in flight; returns the batch's done event (a hipEvent_t address)."""
        ev = C.c_void_p()
        _check(lib().msvs_shard_search_device_async(self._h, comm._h, C.c_void_p(int(d_queries)), C.c_size_t(nq), int(k),
                                                    int(nprobe), C.c_void_p(int(d_alive)) if d_alive else None,
                                                    C.c_size_t(nbits), C.c_void_p(int(d_ids)), C.c_void_p(int(d_dis)),
                                                    C.c_void_p(int(stream)) if stream else None, C.byref(ev)))
        return ev.value

    def scanned_rows(self, queries, nprobe):
        q = _f32(queries).reshape(-1, self.dim)
        rows, streamed, unique = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().msvs_index_scanned_rows(self._h, _p(q, C.c_float), C.c_size_t(q.shape[0]), int(nprobe),
                                             C.byref(rows), C.byref(streamed), C.byref(unique)))
        return rows.value, streamed.value, unique.value

    def export(self, with_vecs=True):
        """(centroids, list offsets, rows in storage order, ids in storage order); with_vecs=False leaves the rows on the
        device (a 10M x 768 index is 30 GB) and returns None for them."""
        n, nl, d = self.num_data, self.num_lists, self.dim
        cent = np.empty((nl, d), np.float32) if self.index_type == INDEX_IVFFLAT else None
        off = np.empty(nl + 1, np.int64)
        vecs = np.empty((n, d), np.float32) if with_vecs else None
        ids = np.empty(n, np.int64)
        _check(lib().msvs_index_export(self._h, _p(cent, C.c_float), _p(off, C.c_int64), _p(vecs, C.c_float),
                                       _p(ids, C.c_int64)))
        return cent, off, vecs, ids

    def serialize(self, path_prefix):
        """-> files <path_prefix>-data_bin.vidx3, <path_prefix>-id_list.vidx3 (stdio convenience)."""
        _check(lib().msvs_index_serialize(self._h, path_prefix.encode()))

    @classmethod
    def load(cls, path_prefix, index_type, metric, dim):
        h = C.c_void_p()
        _check(lib().msvs_index_load(path_prefix.encode(), C.byref(h)))
        return cls(index_type, metric, dim, _handle=h)

    def serialize_io(self, store):
        """msvs_index_serialize_io through stream callbacks; `store` = dict NAME -> bytearray (filled in)."""
        _check(lib().msvs_index_serialize_io(self._h, C.byref(_DictIO(store).io)))

    @classmethod
    def load_io(cls, store, index_type, metric, dim):
        h = C.c_void_p()
        _check(lib().msvs_index_load_io(C.byref(_DictIO(store).io), C.byref(h)))
        return cls(index_type, metric, dim, _handle=h)

    def set_delete_bitmap(self, alive):
        """VIWithMeta::setDeleteBitmap: bool[n] over the index labels (1 = alive), resident; None clears."""
        if alive is None:
            _check(lib().msvs_index_set_delete_bitmap(self._h, None, C.c_size_t(0)))
        else:
            bits = pack_bits(alive)
            _check(lib().msvs_index_set_delete_bitmap(self._h, _p(bits, C.c_uint64), C.c_size_t(len(alive))))

    def set_merged_maps(self, row_ids_map, inverted_row_ids_map, inverted_row_sources_map, own_id):
        a = np.ascontiguousarray(row_ids_map, np.uint64)
        b = np.ascontiguousarray(inverted_row_ids_map, np.uint64)
        c = np.ascontiguousarray(inverted_row_sources_map, np.uint8)
        _check(lib().msvs_index_set_merged_maps(self._h, _p(a, C.c_uint64), C.c_size_t(a.size), _p(b, C.c_uint64),
                                                _p(c, C.c_uint8), C.c_size_t(b.size), C.c_uint32(own_id)))

    def resource_usage(self):
        """-> (memory_usage_bytes, disk_usage_bytes, build_memory_usage_bytes)"""
        m, dk, b = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _check(lib().msvs_index_resource_usage(self._h, C.byref(m), C.byref(dk), C.byref(b)))
        return m.value, dk.value, b.value


class _Scalar(C.Structure):
    _fields_ = [("i", C.c_int64), ("f", C.c_double)]


_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3, np.dtype(np.int8): 4,
           np.dtype(np.int16): 5, np.dtype(np.int32): 6, np.dtype(np.int64): 7, np.dtype(np.float32): 8, np.dtype(np.float64): 9}
OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "between": 6}
FILTER_AND, FILTER_OR, FILTER_AND_NOT = 0, 1, 2


class Filter:
    """msvs_filter_t: a search filter (one bit per row offset of the part) resident on the device."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_bool(cls, alive):
        bits = pack_bits(alive)
        h = C.c_void_p()
        _check(lib().msvs_filter_from_bits(_p(bits, C.c_uint64), C.c_size_t(len(alive)), C.byref(h)))
        return cls(h)

    @classmethod
    def from_offsets(cls, offsets, nbits, device_ptr=None):
        """getFilterFromPipeline: the passing `_part_offset`s (duplicates allowed, offsets >= nbits ignored).  offsets: array-like
        (uploaded), or, for UInt64 offsets already on the device, their count plus device_ptr."""
        h = C.c_void_p()
        if device_ptr is not None:
            n = int(offsets)
            ptr, mem = C.cast(C.c_void_p(int(device_ptr)), C.POINTER(C.c_uint64)), MEM_DEVICE
        else:
            off = np.ascontiguousarray(offsets, np.uint64)
            n, ptr, mem = off.size, _p(off, C.c_uint64), MEM_HOST
        _check(lib().msvs_filter_from_offsets(ptr, C.c_size_t(n), C.c_size_t(nbits), mem, C.byref(h)))
        return cls(h)

    @classmethod
    def from_predicate(cls, column, op, lo, hi=0, device_ptr=None):
        """`column OP lo` (OP in OPS; "between": lo <= x <= hi).  column: numpy array (uploaded), or pass its dtype-carrying
        empty view plus device_ptr / len via (dtype, nrows) tuple for a column already on the device.  Values are compared, the
        constant is not cast into the column type; an integer constant outside int64 raises ValueError."""
        if device_ptr is not None:
            dt, n = column
            ptr, mem = C.c_void_p(int(device_ptr)), MEM_DEVICE
        else:
            col = np.ascontiguousarray(column)
            dt, n = col.dtype, col.size
            ptr, mem = col.ctypes.data_as(C.c_void_p), MEM_HOST
        isf = np.dtype(dt).kind == "f"
        if not isf:  # msvs_scalar_t carries an int64: ctypes would wrap anything else silently
            for c in (lo, hi):
                if not -2 ** 63 <= int(c) < 2 ** 63:
                    raise ValueError("integer constant %d does not fit msvs_scalar_t.i (int64)" % int(c))
        sl = _Scalar(0 if isf else int(lo), float(lo) if isf else 0.0)
        sh = _Scalar(0 if isf else int(hi), float(hi) if isf else 0.0)
        h = C.c_void_p()
        lib().msvs_filter_from_predicate.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, _Scalar, _Scalar,
                                                     C.POINTER(C.c_void_p)]
        _check(lib().msvs_filter_from_predicate(ptr, _DTYPES[np.dtype(dt)], n, mem, OPS[op], sl, sh, C.byref(h)))
        return cls(h)

    def combine(self, other, mode=FILTER_AND):
        _check(lib().msvs_filter_combine(self._h, other._h, int(mode)))
        return self

    def count(self):
        a, n = C.c_uint64(0), C.c_size_t(0)
        _check(lib().msvs_filter_count(self._h, C.byref(a), C.byref(n)))
        return a.value, n.value

    def to_bool(self):
        alive, nbits = self.count()
        words = np.zeros(max(1, (nbits + 63) // 64), np.uint64)
        _check(lib().msvs_filter_to_bits(self._h, _p(words, C.c_uint64)))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:nbits].astype(bool)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_filter_free.argtypes = [C.c_void_p]
            _lib.msvs_filter_free.restype = None
            _lib.msvs_filter_free(self._h)
            self._h = None

    __del__ = close


def release_scratch():
    f = C.c_size_t(0)
    _check(lib().msvs_release_scratch(C.byref(f)))
    return f.value


def hybrid_fuse_device(fusion, d_vec_dis, d_vec_ids, kv, d_txt_scores, d_txt_ids, kt, nq, topk, d_out_scores, d_out_labels, d_n_out,
                       stream=0, fusion_k=60, fusion_weight=0.5, vector_scan_direction=1):
    """msvs_hybrid_fuse_device: RRF ("rrf") / RSF ("rsf") fusion of a batch's vector and text result lists, all device
    pointers (ints), stream-ordered.  Outputs [nq][topk] f32 scores, i64 labels (-1 past n_out[q]), u32 n_out."""
    _check(lib().msvs_hybrid_fuse_device(C.c_int(1 if fusion == "rsf" else 0), C.c_void_p(d_vec_dis), C.c_void_p(d_vec_ids),
                                         C.c_size_t(kv), C.c_void_p(d_txt_scores), C.c_void_p(d_txt_ids), C.c_size_t(kt),
                                         C.c_size_t(nq), C.c_uint64(fusion_k), C.c_float(fusion_weight), C.c_int(vector_scan_direction),
                                         C.c_size_t(topk), C.c_void_p(d_out_scores), C.c_void_p(d_out_labels), C.c_void_p(d_n_out),
                                         C.c_void_p(stream)))


def debug_prune_stats():
    """(pairs the probe pruning of the shadow list scan dropped, pairs it looked at) -- counted only under rerank_stats = 1."""
    out = (C.c_uint64 * 2)()
    _check(lib().msvs_debug_prune_stats(out))
    return int(out[0]), int(out[1])


def debug_prune_first(nq, nprobe):
    """The pre-pruning of this thread's last IVFFLAT search (option coarse_prune_debug = 1) -> (have, probes [nq][nprobe] with -1 for a
    dropped pair, upre [nq], flags [nq]: bit 0 = the coarse tail's prune-first path served the query, bit 1 = the tail's band formed,
    bits 8 and up = the lists that path could not prune under the nearest list's bound).  have = False: that search had no pre-pruning."""
    probes = np.full((nq, nprobe), -1, np.int32)
    upre = np.full(nq, np.inf, np.float32)
    flags = np.zeros(nq, np.uint32)
    have = C.c_int(0)
    fn = lib().msvs_debug_prune_first
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]
    _check(fn(probes.ctypes.data, upre.ctypes.data, flags.ctypes.data, nq, nprobe, C.byref(have)))
    return bool(have.value), probes, upre, flags


def debug_prune_first_served():
    """Queries the coarse tail's prune-first path has served, cumulative -- counted only under coarse_prune_debug = 1."""
    out = C.c_uint64(0)
    _check(lib().msvs_debug_prune_first_served(C.byref(out)))
    return int(out.value)


def debug_rerank_rows():
    """(candidate rows the re-rank's first stage evaluated, rows its second chance evaluated), cumulative -- counted only under
    rerank_stats = 1."""
    out = (C.c_uint64 * 4)()
    _check(lib().msvs_debug_rerank_rows(out))
    return int(out[0]), int(out[1])


def debug_rerank_skipped_chunks():
    """Chunks of second-chance buffers the re-rank skipped whole because the first stage's hint left none of their keys
    (rerank_chain = 1), cumulative -- counted only under rerank_stats = 1."""
    out = (C.c_uint64 * 4)()
    _check(lib().msvs_debug_rerank_rows(out))
    return int(out[2])


def debug_rerank_second_chance():
    """Queries whose first certificate failed and that entered the second chance of the re-rank, cumulative -- counted only under
    rerank_stats = 1."""
    out = (C.c_uint64 * 4)()
    _check(lib().msvs_debug_rerank_rows(out))
    return int(out[3])


def debug_scan_rows():
    """(rows the shadow main launches read, rows their sample launches read), cumulative -- counted only under rerank_stats = 1."""
    out = (C.c_uint64 * 2)()
    _check(lib().msvs_debug_scan_rows(out))
    return int(out[0]), int(out[1])


def bm25_stats():
    """(queries through the sample / emit path, of which fallbacks)."""
    q, f = C.c_uint64(0), C.c_uint64(0)
    _check(lib().msvs_bm25_stats(C.byref(q), C.byref(f)))
    return q.value, f.value


class Postings:
    """msvs_postings_t (seam B): flat-array export of one part's inverted index.  fieldnorm_ids: [num_docs] (one text
    column) or [num_fields, num_docs] with term_field[t] = the column of term t."""

    def __init__(self, post_off, doc_ids, tfs, fieldnorm_ids, term_field=None):
        post_off = np.ascontiguousarray(post_off, np.int64)
        doc_ids = np.ascontiguousarray(doc_ids, np.uint32)
        tfs = np.ascontiguousarray(tfs, np.uint32)
        fieldnorm_ids = np.ascontiguousarray(np.atleast_2d(fieldnorm_ids), np.uint8)
        self.num_fields, self.num_docs = fieldnorm_ids.shape
        tf_ = None if term_field is None else np.ascontiguousarray(term_field, np.uint8)
        h = C.c_void_p()
        _check(lib().msvs_postings_create_fields(_p(post_off, C.c_int64), C.c_size_t(post_off.size - 1), _p(tf_, C.c_uint8),
                                                 _p(doc_ids, C.c_uint32), _p(tfs, C.c_uint32), _p(fieldnorm_ids, C.c_uint8),
                                                 C.c_size_t(self.num_fields), C.c_size_t(self.num_docs), C.byref(h)))
        self._h = h

    def set_alive(self, alive):
        """Resident lightweight-delete bitmap of the part (None clears)."""
        if alive is None:
            _check(lib().msvs_postings_set_alive(self._h, None, C.c_size_t(0)))
        else:
            bits = pack_bits(alive)
            _check(lib().msvs_postings_set_alive(self._h, _p(bits, C.c_uint64), C.c_size_t(len(alive))))

    def _batch_args(self, queries, dfs, groups, total_tokens):
        qoff = np.zeros(len(queries) + 1, np.uint32)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).ravel() for x in xs]) if len(xs) else [], dt)
        qterms, df = cat(queries, np.uint32), cat(dfs, np.uint64)
        qg = None if groups is None else cat(groups, np.uint32)
        tokens = np.ascontiguousarray(np.broadcast_to(np.asarray(total_tokens, np.uint64), (self.num_fields,)))
        return qoff, qterms, qg, df, tokens

    def bm25_search_batch(self, queries, dfs, total_docs, total_tokens, k, alive=None, groups=None, operator_or=True):
        """queries / dfs (/ groups): one sequence per query.  Returns lists of (rows, scores)."""
        nq = len(queries)
        qoff, qterms, qg, df, tokens = self._batch_args(queries, dfs, groups, total_tokens)
        bits, nbits = None, 0
        if alive is not None:
            nbits = len(alive)
            bits = pack_bits(alive)
        rows, scores, cnt = np.empty((nq, k), np.uint64), np.empty((nq, k), np.float32), np.zeros(nq, np.uint32)
        _check(lib().msvs_bm25_search_batch(self._h, C.c_size_t(nq), _p(qoff, C.c_uint32), _p(qterms, C.c_uint32),
                                            _p(qg, C.c_uint32), _p(df, C.c_uint64), C.c_uint64(int(total_docs)),
                                            _p(tokens, C.c_uint64), 1 if operator_or else 0, _p(bits, C.c_uint64),
                                            C.c_size_t(nbits), C.c_size_t(k), _p(rows, C.c_uint64), _p(scores, C.c_float),
                                            _p(cnt, C.c_uint32)))
        return [(rows[q, :cnt[q]].copy(), scores[q, :cnt[q]].copy()) for q in range(nq)]

    def prepare_batch(self, queries, dfs, total_tokens, groups=None):
        """The flat argument arrays of a batch, built once (a serving front end keeps them in this form anyway)."""
        return (len(queries),) + self._batch_args(queries, dfs, groups, total_tokens)

    def bm25_search_batch_device(self, queries, dfs, total_docs, total_tokens, k, d_row_ids, d_scores, stream=0,
                                 d_alive=0, nbits=0, groups=None, operator_or=True, prepared=None):
        """Stream-ordered: int64 ids (-1 = no hit) / f32 scores into DEVICE buffers [nq, k] given by address.
        prepared: the result of prepare_batch (queries / dfs / total_tokens / groups are then ignored)."""
        nq, qoff, qterms, qg, df, tokens = prepared if prepared is not None else self.prepare_batch(queries, dfs, total_tokens, groups)
        _check(lib().msvs_bm25_search_batch_device(self._h, C.c_size_t(nq), _p(qoff, C.c_uint32), _p(qterms, C.c_uint32),
                                                   _p(qg, C.c_uint32), _p(df, C.c_uint64), C.c_uint64(int(total_docs)),
                                                   _p(tokens, C.c_uint64), 1 if operator_or else 0, C.c_void_p(d_alive),
                                                   C.c_size_t(nbits), C.c_size_t(k), C.c_void_p(d_row_ids),
                                                   C.c_void_p(d_scores), C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.msvs_postings_free(self._h)
            self._h = None

    __del__ = close

    def bm25_search(self, qterms, df, total_docs, total_tokens, k, alive=None):
        qterms = np.ascontiguousarray(qterms, np.uint32)
        df = np.ascontiguousarray(df, np.uint64)
        bits, nbits = None, 0
        if alive is not None:
            nbits = len(alive)
            bits = pack_bits(alive)
        rows, scores = np.empty(k, np.uint64), np.empty(k, np.float32)
        n = C.c_size_t(0)
        _check(lib().msvs_bm25_search(self._h, _p(qterms, C.c_uint32), _p(df, C.c_uint64), C.c_size_t(qterms.size),
                                      C.c_uint64(int(total_docs)), C.c_uint64(int(total_tokens)), _p(bits, C.c_uint64),
                                      C.c_size_t(nbits), C.c_size_t(k), _p(rows, C.c_uint64), _p(scores, C.c_float),
                                      C.byref(n)))
        return rows[:n.value], scores[:n.value]
