"""The definition of the device generator (tests/device_rng.py, the NumPy restatement of csrc/device_common.h) is a sound
generator: keep rates, correlations along every axis the kernels key it by (row, column, stream, step, seed), duplicate
words, and the moments / distribution of the Box-Muller and categorical draws.

Every bound is a condition on the generator, fixed before looking: |z| <= 5 on a statistic that is standard normal for
independent uniform words (some 5 x 10^4 statistics in all: a sound generator exceeds 5 somewhere with probability of about 3%),
p-values above 1e-4 (a few hundred tests), duplicates below a Poisson bound at 5 sd.  What this file measures (it prints
every figure): worst |z| 4.53 (two streams at p = 0.2; 4.43 from step to step at p = 0.8), 74 duplicate words over the 432
masks (80.5 expected, bound 125), smallest KS p-value 0.016, smallest chi-square p-value 0.0018 (c = 7, of 36 tests)."""
import itertools

import numpy as np
import pytest

import device_rng as R

SEEDS = [0, 1, 7, 99, 1234, 2 ** 63 + 5]
STEPS = range(6)
STREAMS = range(12)
RATES = [0.1, 0.2, 0.5, 0.8]
ROWS = COLS = 200
ZMAX = 5.0


def _standardised(w, p):
    """keep bits -> mean 0, variance 1 under the null (p = 0.5: the +-1 mask)."""
    q = float(np.float32(p))
    return (R.keep(w, p).astype(np.float64) - (1.0 - q)) / np.sqrt(q * (1.0 - q))


def _z_corr(a, b):
    return float((a * b).mean() * np.sqrt(a.size))


def test_scalar_restatement_agrees_with_the_vectorised_one():
    """hash_cell once more in plain Python integers: guards the uint32 wrap-around of the array form."""
    def cell(key, r, c):
        x = (((key & 0xFFFFFFFF) + r * 0x9E3779B1) ^ ((key >> 32) + c * 0x85EBCA77)) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    rows, cols = [0, 1, 36, 37, 2 ** 31 - 1, 2 ** 32 - 1], [0, 1, 47, 95, 0xFFFFFFFF]
    for seed, step, sid in [(0, 0, 0), (1234, 3, 4), (2 ** 63 + 5, 5, 100), (99, 2 ** 40, 12)]:
        key = R.stream_key(seed, step, sid)
        assert key == (seed ^ ((step * 0xD1B54A32D192ED03) % 2 ** 64) ^ ((sid * 0xA0761D6478BD642F) % 2 ** 64))
        got = R.hash_cell(key, rows, cols)
        assert got.dtype == np.uint32
        for i, r in enumerate(rows):
            for j, c in enumerate(cols):
                assert int(got[i, j]) == cell(key, r, c), (seed, step, sid, r, c)
    assert R.rng_key(0, 0, 100) == 100 << 56 and R.rng_key(5, 1, 0) == 5 ^ 0xD1B54A32D192ED03


def test_step_value_is_the_count_of_opened_steps():
    assert [R.step_value(n) for n in (1, 2, 3)] == [1, 2, 3] and R.step_value(1, restored=41) == 42


def test_keep_threshold_edges():
    assert R.keep_threshold(0.5) == 2 ** 31
    assert R.keep_threshold(1.0) == 2 ** 32 - 1                      # p * 2^32 = 2^32 saturates ...
    assert R.keep_threshold(1.5) == 2 ** 32 - 1
    assert R.keep_threshold(np.nextafter(np.float32(1), np.float32(0))) == 2 ** 32 - 256       # ... the float32 below 1 does not
    assert R.keep_threshold(0.2) == int(float(np.float32(0.2)) * 2 ** 32) == 858993472        # (the rate is a float32)
    assert R.keep_threshold(0.0) is None
    w = np.array([[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]], dtype=np.uint32)
    assert R.keep(w, 0.5).tolist() == [[0, 0, 0, 1, 1]]              # kept iff word >= threshold
    assert R.keep(w, 1.0).tolist() == [[0, 0, 0, 0, 1]]
    assert R.keep(w, 0.0).tolist() == [[1, 1, 1, 1, 1]]              # p = 0: dropout is off
    masks = R.dropout_masks(3, 1, 0.0, 0.5, 5, 8)
    assert all(m.dtype == np.uint8 and m.shape == (5, 8) for m in masks)
    assert all(masks[i].all() for i in range(0, 12, 2)) and not any(masks[i].all() for i in range(1, 12, 2))


def test_mask_layout_discriminator_halves_and_global_rows():
    seed, step, B, h = 1234, 2, 9, 16
    w4, w5 = R.words(seed, step, 4, 40, h), R.words(seed, step, 5, 40, h)
    m = R.dropout_masks(seed, step, 0.2, 0.3, B, h)
    assert np.array_equal(m[4], R.keep(w4[:B], 0.2)) and np.array_equal(m[6], R.keep(w4[B:2 * B], 0.2))
    assert np.array_equal(m[5], R.keep(w5[:B], 0.3)) and np.array_equal(m[7], R.keep(w5[B:2 * B], 0.3))
    g = R.dropout_masks(seed, step, 0.2, 0.3, B, h, row0=3, global_rows=20)      # a rank's rows [3, 12) of 20
    assert np.array_equal(g[4], R.keep(w4[3:12], 0.2)) and np.array_equal(g[6], R.keep(w4[23:32], 0.2))
    assert np.array_equal(g[7], R.keep(w5[23:32], 0.3))
    assert np.array_equal(g[0], R.keep(R.words(seed, step, 0, 40, h)[3:12], 0.2))
    # the ranks' draws tile the single process's: rows [0, 20) in shares of 10
    one = R.dropout_masks(seed, step, 0.2, 0.3, 20, h, global_rows=20)
    parts = [R.dropout_masks(seed, step, 0.2, 0.3, 10, h, row0=o, global_rows=20) for o in (0, 10)]
    for i in range(12):
        assert np.array_equal(one[i], np.concatenate([p[i] for p in parts])), i
    z = R.prior(seed, step, "gauss", 20, 6)
    assert np.array_equal(z[10:], R.prior(seed, step, "gauss", 10, 6, row0=10))
    assert np.array_equal(R.prior(seed, step, "categorical", 20, 6)[10:], R.prior(seed, step, "categorical", 10, 6, row0=10))
    assert not R.prior(seed, step, "bernoulli", 4, 6).any()
    assert np.array_equal(R.prior(seed, step, "categorical", 8, 6, scale=2.5).sum(1), np.full(8, 2.5, dtype=np.float32))


def test_keep_rates():
    worst = 0.0
    for seed, step, sid in itertools.product(SEEDS, STEPS, STREAMS):
        w = R.words(seed, step, sid, ROWS, COLS)
        for p in RATES:
            q = float(np.float32(p))
            z = (R.keep(w, p).mean() - (1.0 - q)) / np.sqrt(q * (1.0 - q) / w.size)
            worst = max(worst, abs(z))
    print(f"keep rate: worst |z| {worst:.2f}")
    assert worst <= ZMAX


@pytest.mark.parametrize("p", RATES)
def test_masks_are_uncorrelated_along_rows_columns_and_streams(p):
    worst = {"row lag 1": 0.0, "row lag 2": 0.0, "col lag 1": 0.0, "col lag 2": 0.0, "streams": 0.0}
    for seed, step in itertools.product(SEEDS, STEPS):
        ms = [_standardised(R.words(seed, step, sid, ROWS, COLS), p) for sid in STREAMS]
        for m in ms:
            for name, a, b in (("row lag 1", m[1:], m[:-1]), ("row lag 2", m[2:], m[:-2]),
                               ("col lag 1", m[:, 1:], m[:, :-1]), ("col lag 2", m[:, 2:], m[:, :-2])):
                worst[name] = max(worst[name], abs(_z_corr(a, b)))
        for i, j in itertools.combinations(STREAMS, 2):
            worst["streams"] = max(worst["streams"], abs(_z_corr(ms[i], ms[j])))
    print(f"p = {p}: worst |z| {worst}")
    assert max(worst.values()) <= ZMAX, worst


@pytest.mark.parametrize("p", RATES)
def test_masks_are_uncorrelated_from_step_to_step_and_seed_to_seed(p):
    worst = {"steps": 0.0, "seeds": 0.0}
    for seed in SEEDS:
        ms = [_standardised(R.words(seed, step, 4, ROWS, COLS), p) for step in range(40)]
        for i, j in itertools.combinations(range(40), 2):
            worst["steps"] = max(worst["steps"], abs(_z_corr(ms[i], ms[j])))
    for base in SEEDS:
        ms = [_standardised(R.words((base + k) & R.M64, 3, 4, ROWS, COLS), p) for k in range(40)]
        for i, j in itertools.combinations(range(40), 2):
            worst["seeds"] = max(worst["seeds"], abs(_z_corr(ms[i], ms[j])))
    print(f"p = {p}: worst |z| {worst}")
    assert max(worst.values()) <= ZMAX, worst


def test_duplicate_words_stay_at_the_birthday_rate():
    n_masks, dups = 0, 0
    for seed, step, sid in itertools.product(SEEDS, STEPS, STREAMS):
        w = R.words(seed, step, sid, ROWS, COLS)
        dups += w.size - np.unique(w).size
        n_masks += 1
    expect = n_masks * (ROWS * COLS) ** 2 / 2.0 ** 33
    print(f"{dups} duplicate words over {n_masks} masks, {expect:.1f} expected")
    assert dups <= expect + 5.0 * np.sqrt(expect)


@pytest.mark.parametrize("sid", [R.PRIOR_STREAM, R.EPS_STREAM])
def test_gaussian_draws(sid):
    from scipy import stats
    worst, ks_min = 0.0, 1.0
    for seed, step in itertools.product(SEEDS, STEPS):
        v = R.gauss(seed, step, sid, 128, 64)
        n = v.size
        zs = [v.mean() * np.sqrt(n), (v.var() - 1.0) / np.sqrt(2.0 / n), ((v ** 4).mean() - 3.0) / np.sqrt(96.0 / n),
              _z_corr(v[1:], v[:-1]), _z_corr(v[:, 1:], v[:, :-1])]
        worst = max(worst, max(abs(z) for z in zs))
        ks_min = min(ks_min, stats.kstest(v.ravel(), "norm").pvalue)
        assert np.abs(v).max() <= np.sqrt(48 * np.log(2.0)) + 1e-12      # f1 >= 2^-24 bounds the radius
    print(f"stream {sid}: worst |z| {worst:.2f}, smallest KS p-value {ks_min:.3g}")
    assert worst <= ZMAX
    assert ks_min > 1e-4


def test_gaussian_prior_is_the_eps_form_on_its_own_stream_and_float32():
    z = R.prior(7, 2, "gauss", 37, 12, scale=0.5, row0=5)
    g = R.gauss(7, 2, R.PRIOR_STREAM, 37, 12, row0=5)
    assert z.dtype == np.float32 and np.array_equal(z, g.astype(np.float32) * np.float32(0.5))
    assert np.array_equal(R.vae_eps(7, 2, R.EPS_STREAM, 37, 12), R.gauss(7, 2, 12, 37, 12).astype(np.float32))
    assert not np.array_equal(R.vae_eps(7, 2, 12, 37, 12), R.vae_eps(7, 3, 12, 37, 12))


@pytest.mark.parametrize("c", [7, 12, 50])
def test_categorical_prior_is_uniform_over_the_classes(c):
    from scipy import stats
    p_min = 1.0
    for seed, step in itertools.product(SEEDS, STEPS):
        cls = R.categorical_classes(seed, step, 20000, c)
        p_min = min(p_min, stats.chisquare(np.bincount(cls, minlength=c)).pvalue)
    print(f"c = {c}: smallest chi-square p-value {p_min:.3g}")
    assert p_min > 1e-4
    z = R.prior(1234, 2, "categorical", 50, c)
    assert np.array_equal(z.sum(1), np.ones(50)) and np.array_equal(z.argmax(1), R.categorical_classes(1234, 2, 50, c))
