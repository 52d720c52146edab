"""The reference and the comparisons of test_ivf_build.py checked on their own, without a device: they accept a right answer and reject
deliberately wrong ones -- a tie that goes to the higher id, the last partial centroid tile ignored, a mean divided by m + 1."""
import numpy as np
import pytest

import ivf_build_ref as R


def tie_case():
    rng = np.random.default_rng(130)
    cent = rng.integers(-2, 3, (130, 3)).astype(np.float32)
    x = rng.integers(-2, 3, (300, 3)).astype(np.float32)
    return x, cent


def test_mersenne_twister_is_the_standard_one():
    rng = R.Mt19937_64(5489)
    for _ in range(9999):
        rng()
    assert rng() == 9981545732273789042  # ISO C++ [rand.predef]: the 10000th value of a default-constructed mt19937_64
    s = R.train_sample(50, 20, 3)
    assert len(set(s.tolist())) == 20 and s.min() >= 0 and s.max() < 50
    assert (R.train_sample(50, 20, 3) == s).all() and (R.train_sample(50, 20, 4) != s).any()


def test_lists_of_ids():
    off, ids = np.array([0, 2, 2, 5]), np.array([3, 4, 0, 1, 2])
    assert R.lists_of_ids(off, ids, 5).tolist() == [2, 2, 2, 0, 0]
    with pytest.raises(AssertionError):
        R.lists_of_ids(off, np.array([3, 4, 0, 1, 1]), 5)


@pytest.mark.parametrize("ip", [False, True])
def test_exact_check_rejects_a_tie_that_goes_to_the_higher_id(ip):
    x, cent = tie_case()
    s = R.int_scores(x, cent, ip)
    want = R.exact_assign(x, cent, ip)
    R.check_exact(want, want)
    tied = (s == s.min(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied.mean() > 0.4
    highest = s.shape[1] - 1 - np.argmin(s[:, ::-1], axis=1)
    assert (s[np.arange(len(x)), highest] == s.min(axis=1)).all()  # as good a centroid, but not the lowest
    with pytest.raises(AssertionError):
        R.check_exact(highest, want)
    one = want.copy()
    r = np.flatnonzero(tied)[0]
    one[r] = highest[r]
    with pytest.raises(AssertionError):
        R.check_exact(one, want)


@pytest.mark.parametrize("ip", [False, True])
def test_checks_reject_an_ignored_last_centroid_tile(ip):
    rng = np.random.default_rng(2)
    n, d, nlist = 300, 20, 129  # the second tile holds one centroid
    cent = rng.integers(-8, 9, (nlist, d)).astype(np.float32)
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    cent[128] = 8 * (1 - 2 * (np.arange(d) % 2))
    x[17] = cent[128]  # a row only the last centroid wins
    want = R.exact_assign(x, cent, ip)
    assert want[17] == 128
    with pytest.raises(AssertionError):
        R.check_exact(R.exact_assign(x, cent[:128], ip), want)
    xf = rng.standard_normal((1500, d), dtype=np.float32)
    cf = rng.standard_normal((nlist, d), dtype=np.float32)
    if ip:
        cf[128] *= 2  # (by inner product a short centroid wins nothing)
    s, _ = R.float_scores(xf, cf, ip)
    best = np.argmin(s, axis=1)
    assert (best == 128).any()
    R.check_float_assign(best, xf, cf, ip)
    with pytest.raises(AssertionError):
        R.check_float_assign(np.argmin(s[:, :128], axis=1), xf, cf, ip)


def test_float_check_allows_only_what_the_bound_allows():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 17), dtype=np.float32)
    c = rng.standard_normal((40, 17), dtype=np.float32)
    c[21] = c[4]
    c[21, 0] = np.nextafter(c[4, 0], np.float32(9))  # one ulp from centroid 4: every row they win is ambiguous between the two
    s, B = R.float_scores(x, c, False)
    best, amb, touched = R.ambiguous_rows(s, B)
    assert amb.any() and set(np.flatnonzero(touched)) == {4, 21} and set(best[amb]) <= {4, 21}
    swapped = best.copy()
    swapped[amb] = 25 - best[amb]
    R.check_float_assign(swapped, x, c, False, max_ambiguous=1.0)
    with pytest.raises(AssertionError):  # the cap is on the reference alone
        R.check_float_assign(best, x, c, False, max_ambiguous=0.0)
    second = np.argsort(s, axis=1)[:, 1]
    wrong = best.copy()
    r = np.flatnonzero(~amb)[0]
    wrong[r] = second[r]
    with pytest.raises(AssertionError):
        R.check_float_assign(wrong, x, c, False, max_ambiguous=1.0)


def test_mean_check_rejects_a_division_by_m_plus_1():
    rng = np.random.default_rng(4)
    xs = R.int_rows(rng, 600, 20, -8, 8)
    seeds = xs[:130]
    want, cnt, touched = R.lloyd_step(xs, seeds)
    assert (cnt > 0).all() and not touched.any()
    a = R.exact_assign(xs, seeds, False)
    exact = np.stack([xs[a == j].astype(np.float64).mean(axis=0) for j in range(130)])
    assert np.abs(want - exact).max() <= 2 * R.U * 8  # two roundings of a value of at most 8
    R.check_bit_equal(want.copy(), want)
    sums = np.stack([xs[a == j].astype(np.float64).sum(axis=0) for j in range(130)])
    off_by_one = sums.astype(np.float32) * (np.float32(1) / (cnt + 1).astype(np.float32))[:, None]
    with pytest.raises(AssertionError):
        R.check_bit_equal(off_by_one, want)
    divided = (sums / cnt[:, None]).astype(np.float32)  # one rounding instead of the kernel's two: not the same bits everywhere
    assert (divided != want).any()
    # the f32 summation in member order agrees on exact data, and is what pins rows that are not integers
    same, _ = R.f32_means(xs, a, seeds)
    R.check_bit_equal(same, want)
    xn = (xs / np.sqrt((xs * xs).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)
    fm, _ = R.f32_means(xn, a, xn[:130])
    bad = xn.astype(np.float64)
    wrong = np.stack([bad[a == j].sum(axis=0) / (cnt[j] + 1) for j in range(130)]).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_bit_equal(wrong, fm)
