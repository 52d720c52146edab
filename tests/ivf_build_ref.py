"""The numpy reference of the IVF build feed (ivf_build_kernels.hpp, msvs_index_train) and the comparisons the tests of it make:
nearest-centroid assignment in int64 / float64, the ambiguity rule for float data, one Lloyd step with the kernel's two roundings.
Nothing here touches the device: test_ivf_build.py feeds it what the device produced, test_ivf_build_ref.py deliberately wrong answers."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of f32


def lists_of_ids(off, ids, n):
    """list of every row from an export's offsets and labels (labels = 0 .. n - 1, the staging order)"""
    off, ids = np.asarray(off, np.int64), np.asarray(ids, np.int64)
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert sorted(ids.tolist()) == list(range(n))
    out = np.empty(n, np.int64)
    out[ids] = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return out


def int_scores(x, c, ip):
    """|c|^2 - 2 <c, x> (L2) or -<c, x> (IP) of integer-valued rows and centroids in int64: [n, nlist], exact.  A centroid that is
    not finite scores int64 max: it receives no rows."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    ok = np.isfinite(c).all(axis=1)
    ci = np.where(ok[:, None], c, 0.0)
    assert (x == np.rint(x)).all() and (ci == np.rint(ci)).all(), "exact assignment needs integer-valued data"
    xi, ci = x.astype(np.int64), ci.astype(np.int64)
    dot = xi @ ci.T
    s = -dot if ip else (ci * ci).sum(axis=1)[None, :] - 2 * dot
    # every partial sum of the kernel is an integer below 2^24: f32 holds it exactly, whatever the order of the additions
    bound = np.abs(xi) @ np.abs(ci).T
    assert int((bound if ip else (ci * ci).sum(axis=1)[None, :] + 2 * bound).max(initial=0)) < 2 ** 24
    s[:, ~ok] = np.iinfo(np.int64).max
    return s


def exact_assign(x, c, ip):
    """argmin of int_scores, ties to the lowest centroid id (numpy's argmin takes the first minimum)"""
    return np.argmin(int_scores(x, c, ip), axis=1).astype(np.int64)


def check_exact(got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d rows in the wrong list, first (row, got, want): %s" % (
        bad.size, got.size, [(int(r), int(got[r]), int(want[r])) for r in bad[:5]])


def float_scores(x, c, ip):
    """-> (scores [n, nlist] in float64, B [n, nlist]): B bounds the error of the kernel's f32 score,
    (d + 2) 2^-24 (|c|^2 + 2 sum |c_k x_k|) for L2 (d roundings in the product, d in the norm, one in the last fma) and
    (d + 2) 2^-24 sum |c_k x_k| for IP."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    d = x.shape[1]
    dot, adot = x @ c.T, np.abs(x) @ np.abs(c).T
    if ip:
        return -dot, (d + 2) * U * adot
    cn = (c * c).sum(axis=1)[None, :]
    return cn - 2 * dot, (d + 2) * U * (cn + 2 * adot)


def ambiguous_rows(s, B):
    """Rows where a second centroid lies within the two scores' error bounds of the best one -- from the reference alone.
    -> (best [n], ambiguous [n], touched [nlist]: the centroids an ambiguous row may go to)"""
    n = s.shape[0]
    best = np.argmin(s, axis=1)
    r = np.arange(n)
    near = s - s[r, best][:, None] - (B + B[r, best][:, None]) <= 0
    near[r, best] = False
    amb = near.any(axis=1)
    near[r, best] = amb
    return best, amb, near.any(axis=0)


def check_float_assign(got, x, c, ip, max_ambiguous=0.01):
    """The rule for float data: a row passes if score64(got) - min score64 <= B(got) + B(best), which makes it match the reference
    exactly wherever the reference's gap to every other centroid exceeds the bounds.  At most `max_ambiguous` of the rows may be
    ambiguous -- asserted on the reference before the device's answer is looked at.  -> (best, ambiguous mask)."""
    s, B = float_scores(x, c, ip)
    best, amb, _ = ambiguous_rows(s, B)
    assert amb.mean() <= max_ambiguous, "the reference itself is ambiguous on %d of %d rows" % (amb.sum(), amb.size)
    got = np.asarray(got, np.int64)
    assert got.shape == best.shape and (got >= 0).all() and (got < c.shape[0]).all()
    r = np.arange(s.shape[0])
    over = s[r, got] - s[r, best] - (B[r, got] + B[r, best])
    bad = np.flatnonzero(over > 0)
    assert bad.size == 0, "%d of %d rows beyond the bound, first (row, got, best, excess): %s" % (
        bad.size, got.size, [(int(i), int(got[i]), int(best[i]), float(over[i])) for i in bad[:5]])
    assert (got[~amb] == best[~amb]).all()
    return best, amb


def lloyd_means(x, assign, prev):
    """One centroid update on integer-valued rows as centroid_update_kernel does it: the sum (exact: integers below 2^24), rounded to
    f32, times f32(1) / f32(m) -- two roundings.  An empty cluster keeps `prev`.  -> (centroids f32, member counts)."""
    x64 = np.asarray(x, np.float64)
    assert (x64 == np.rint(x64)).all()
    nlist = prev.shape[0]
    out = np.array(prev, np.float32, copy=True)
    cnt = np.bincount(assign, minlength=nlist)
    for j in np.flatnonzero(cnt):
        rows = x64[assign == j]
        assert np.abs(rows).sum(axis=0).max() < 2 ** 24
        out[j] = rows.sum(axis=0).astype(np.float32) * (np.float32(1) / np.float32(cnt[j]))
    return out, cnt


def check_bit_equal(got, want, rows=None):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    ne = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    if rows is not None:
        ne &= rows
    bad = np.flatnonzero(ne)
    assert bad.size == 0, "%d of %d centroids differ, first %d: got %s want %s" % (bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])


def f32_means(xs, assign, prev):
    """centroid_update_kernel on any f32 rows, to the bit: each component summed in f32 from 0 in member order (ascending position in
    the sample `xs`), then times f32(1) / f32(m)."""
    xs = np.asarray(xs, np.float32)
    out = np.array(prev, np.float32, copy=True)
    cnt = np.bincount(assign, minlength=prev.shape[0])
    for j in np.flatnonzero(cnt):
        acc = np.zeros(xs.shape[1], np.float32)
        for row in xs[assign == j]:
            acc = acc + row
        out[j] = acc * (np.float32(1) / np.float32(cnt[j]))
    return out, cnt


class Mt19937_64:
    """std::mt19937_64 (the 64-bit Mersenne Twister of Matsumoto and Nishimura as ISO C++ fixes it), seeded with one value."""
    N, M, MASK = 312, 156, (1 << 64) - 1

    def __init__(self, seed):
        mt = [seed & self.MASK]
        for i in range(1, self.N):
            mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & self.MASK)
        self.mt, self.i = mt, self.N

    def __call__(self):
        mt = self.mt
        if self.i >= self.N:
            for k in range(self.N):
                y = (mt[k] & 0xFFFFFFFF80000000) | (mt[(k + 1) % self.N] & 0x7FFFFFFF)
                mt[k] = mt[(k + self.M) % self.N] ^ (y >> 1) ^ (0xB5026F5AA96619E9 if y & 1 else 0)
            self.i = 0
        y = mt[self.i]
        self.i += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        y ^= y >> 43
        return y & self.MASK


def train_sample(n, ns, seed):
    """The rows msvs_index_train samples, in sample order: a partial Fisher-Yates over 0 .. n - 1 driven by mt19937_64(seed) with
    j = i + rng() % (n - i).  The first nlist of them are the seeds."""
    rng = Mt19937_64(seed)
    perm = list(range(n))
    for i in range(ns):
        j = i + rng() % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm[:ns], np.int64)


def int_rows(rng, n, d, lo, hi):
    """n distinct integer-valued rows with components in [lo, hi], in a seeded order"""
    x = np.unique(rng.integers(lo, hi + 1, (4 * n + 64, d)), axis=0)
    assert x.shape[0] >= n
    return x[rng.permutation(x.shape[0])[:n]].astype(np.float32)


def lloyd_step(xs, prev):
    """One k-means iteration of msvs_index_train on the sample `xs` (L2 assignment whatever the index's metric, then the means).
    Integer-valued rows and centroids: the exact argmin.  Otherwise the float rule: `touched` marks the centroids an ambiguous row
    may go to; their means are not pinned.  -> (centroids f32, member counts, touched [nlist])"""
    xs, prev = np.asarray(xs, np.float32), np.asarray(prev, np.float32)
    int_x = bool((xs == np.rint(xs)).all())
    if int_x and bool((prev == np.rint(prev)).all()):
        a, touched = exact_assign(xs, prev, False), np.zeros(prev.shape[0], bool)
    else:
        a, _, touched = ambiguous_rows(*float_scores(xs, prev, False))
    want, cnt = (lloyd_means if int_x else f32_means)(xs, a, prev)
    return want, cnt, touched
