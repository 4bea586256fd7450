"""DenoisingAutoEncoder(corrupt_draws=...): the constructor's contract, and the zero-corruption flags of the device generator
(stream 13 of csrc/device_common.h, restated by tests/device_rng.py) held to what a sound generator gives: the kept share,
no correlation with the dropout stream 0 of the same (step, row, column), none from step n to n + 1 - within |z| <= 5, the
bounds of tests/test_device_rng_cpu.py.  tests/test_dae_draws_gpu.py holds the kernels to the same restatement."""
import itertools

import numpy as np
import pytest

import device_rng as R

ZERO_STREAM, GAUSS_STREAM = 13, 14      # csrc/dae_corrupt.h kDaeZeroStream / kDaeGaussStream
SEEDS = [0, 7, 1234, 2 ** 63 + 5]
STEPS = range(1, 7)
ROWS, COLS = 200, 5000
ZMAX = 5.0


def _standardised(w, p):
    q = float(np.float32(p))
    return (R.keep(w, p).astype(np.float64) - (1.0 - q)) / np.sqrt(q * (1.0 - q))


def _z_corr(a, b):
    return float((a * b).mean() * np.sqrt(a.size))


def test_constructor_contract():
    from aaerec.dae import DenoisingAutoEncoder, DAERecommender
    assert DenoisingAutoEncoder(verbose=False).corrupt_draws == "torch"
    for corrupt in ("zeros", "gauss"):
        assert DenoisingAutoEncoder(corrupt=corrupt, corrupt_draws="step", verbose=False).corrupt_draws == "step"
        with pytest.raises(ValueError):
            DenoisingAutoEncoder(corrupt=corrupt, corrupt_draws="step", rng_mode="reference", verbose=False)
        with pytest.raises(ValueError):
            DenoisingAutoEncoder(corrupt=corrupt, corrupt_draws="numpy", verbose=False)
    assert DenoisingAutoEncoder(rng_mode="reference", verbose=False).corrupt_draws == "torch"
    assert DAERecommender(corrupt_draws="step", verbose=False).model_params["corrupt_draws"] == "step"      # (kwargs are forwarded)


def test_the_new_streams_are_free():
    """0-11 are the dropout masks, 12 the VAE's eps, 100 the prior (device_rng.py)."""
    taken = set(range(12)) | {R.EPS_STREAM, R.PRIOR_STREAM}
    assert ZERO_STREAM not in taken and GAUSS_STREAM not in taken and ZERO_STREAM != GAUSS_STREAM


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_kept_share(p):
    q, worst = float(np.float32(p)), 0.0
    for seed, step in itertools.product(SEEDS, STEPS):
        k = R.keep(R.words(seed, step, ZERO_STREAM, ROWS, COLS), p)
        worst = max(worst, abs((k.mean() - (1.0 - q)) / np.sqrt(q * (1.0 - q) / k.size)))
    print(f"p = {p}: kept share, worst |z| {worst:.2f}")
    assert worst <= ZMAX


def test_p_zero_keeps_everything():
    assert R.keep(R.words(3, 1, ZERO_STREAM, 4, 50), 0.0).all()


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_flags_are_uncorrelated_with_dropout_stream_0_and_from_step_to_step(p):
    worst = {"stream 0": 0.0, "steps": 0.0}
    for seed in SEEDS:
        ms = {step: _standardised(R.words(seed, step, ZERO_STREAM, ROWS, COLS), p) for step in range(1, 8)}
        for step in STEPS:
            worst["stream 0"] = max(worst["stream 0"], abs(_z_corr(ms[step], _standardised(R.words(seed, step, 0, ROWS, COLS), p))))
            worst["steps"] = max(worst["steps"], abs(_z_corr(ms[step], ms[step + 1])))
    print(f"p = {p}: worst |z| {worst}")
    assert max(worst.values()) <= ZMAX, worst
