"""The deferred first-layer Adam's references against each other, without a GPU (tests/lazy_adam.py): the float32
restatement of lazy_replay on its ring of per-step scalars must stay within HALF of the derived bounds of the float64
reference - the other half is the margin of the device's 1-ulp rcpf / sqrtf -, the truncated tail within the bound the
comment in csrc/kernels.h derives, and the schedule must make a wrong table index and every learning-rate change visible
(or the GPU test that uses the same schedule and bounds would be vacuous)."""
import functools

import numpy as np
import pytest

import lazy_adam as L
from lazy_adam import KEYS, Plan, START_STEPS

GAPS = (1, 2, 127, 128, 129, 130, 200, 1500, 4000)


def _ratio(got, want, tol):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(np.max(np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)))


def _plans(T0):
    """Every gap of GAPS occurs: Plan.main has 1, 2, 3, 30, 127 .. 130, 200 and 244, Plan.cut the segments of exactly 128
    and 129, the long plans 1 500 (a row touched once at 1 400 of 1 500 steps, one never) and 4 000 (never)."""
    return [("main", Plan.main(T0)), ("main+predict+dense", Plan.main(T0, predict=True, dense_at=250, ae_only=True)), ("cut", Plan.cut(T0)),
            ("long1500", Plan.long(T0, 1500, 1400)), ("long4000", Plan.long(T0, 4000, 2))]


@functools.lru_cache(maxsize=None)
def _worst(T0, shift=0):
    worst = {k: 0.0 for k in KEYS}
    for name, pl in _plans(T0):
        if shift and name != "main":
            continue
        for i in range(pl.P):
            st64, tol, st32 = pl.restated(i, shift=shift)
            for k in KEYS:
                # half of the bound - but of its rounding part: the mismatch between the kernel's exact powers 0.9^rest /
                # 0.999^rest and the fp32 constants' powers is systematic, and the restatement attains all of it
                sys = tol["systematic"][k]
                worst[k] = max(worst[k], _ratio(st32[k], st64[k], 2 * sys + (tol[k] - sys)))
    return worst


@pytest.mark.parametrize("T0", START_STEPS)
def test_float32_restatement_stays_within_half_of_the_bounds(T0):
    worst = _worst(T0)
    print(f"T0={T0}: worst |replay32 - replay64| / bound:", {k: round(v, 4) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 0.5, (T0, k, v)


@pytest.mark.parametrize("T0", START_STEPS)
def test_dropped_tail_is_within_the_bound_of_the_kernels_comment(T0):
    """kernels.h: after kLazyReplay steps the increments left sum to < 32 lr 0.9005^128 per optimiser (|m| / sqrt(v) <= 3.2,
    shrinking by 0.9 / 0.9995 per step) - for every lazy segment of a row, so per segment here."""
    for name, pl in _plans(T0):
        limit = 2 * 32 * pl.lr_max() * 0.9005 ** L.K_REPLAY
        for i in range(pl.P):
            pts = [0] + pl.sync_points(i) + [pl.S]
            n_long = sum(1 for a, b in zip(pts, pts[1:]) if b - a > L.K_REPLAY)
            _, tail, _ = pl.reference(i)
            assert np.all(tail <= max(1, n_long) * limit), (T0, name, i, float(tail.max()), limit, n_long)
            if n_long == 0:
                assert not tail.any()


def test_ring_is_read_at_the_slot_of_the_replayed_step_across_the_wrap():
    """Replayed step j of a segment from t0 reads slot (t0 + 1 + j) & 65535, and that slot holds the entry of step t0 + 1 + j -
    for segments on either side of and across step 65 536, and twice round the ring."""
    for T0 in (L.WRAP, 2 * L.CAP - 5):
        pl = Plan.main(T0)
        crossed = 0
        for i in range(pl.P):
            reads = []
            st = {k: pl.states[k][i] for k in KEYS}
            pts = [T0 + s for s in pl.sync_points(i)]
            L.replay32(st, T0, pts, T0 + pl.S, pl.lr_gen_of, pl.lr_reg_of, reads=reads)
            assert reads and all(want == held for want, held in reads), (T0, i)
            steps = [w for w, _ in reads]
            crossed += any((a & (L.CAP - 1)) > (b & (L.CAP - 1)) for a, b in zip(steps, steps[1:]))
        assert crossed >= 3, (T0, crossed)          # (several rows' replays run over the wrap)
    reads = []
    pl = Plan.main(L.WRAP)
    L.replay32({k: pl.states[k][0] for k in KEYS}, L.WRAP, [], L.WRAP + 300, pl.lr_gen_of, pl.lr_reg_of, shift=-1, reads=reads)
    assert all(held == want - 1 for want, held in reads[1:])          # what the shifted index of the next test reads


@pytest.mark.parametrize("shift", [-1, 1])
@pytest.mark.parametrize("T0", START_STEPS)
def test_a_shifted_table_index_breaks_the_bounds(T0, shift):
    """The restatement with the table read one slot off: the schedule's rate changes make that visible far beyond the
    bounds (at a constant rate and bias corrections near 1 it changes nothing)."""
    worst = _worst(T0, shift)
    print(f"T0={T0} shift={shift}: worst error / bound of p:", worst["p"])
    assert worst["p"] > 100.0, (T0, shift, worst)


@pytest.mark.parametrize("T0", START_STEPS)
@pytest.mark.parametrize("kind", ["main", "cut"])
def test_every_rate_change_moves_some_probe_far_beyond_its_tolerance(T0, kind):
    """At every set_lr of the schedule some probe element's float64 increment of that step differs between the old and
    the new rates by more than 100 times the element's tolerance at the end of the run."""
    pl = Plan.main(T0) if kind == "main" else Plan.cut(T0)
    tols = [pl.reference(i)[2]["p"] for i in range(pl.P)]
    for s in sorted(pl.lr):
        old, new = pl.rates(s - 1), pl.lr[s]
        best = 0.0
        for i in range(pl.P):
            d = np.abs(pl.increment64(i, s, new) - pl.increment64(i, s, old))
            best = max(best, float(np.max(np.where(d > 0, d / np.maximum(tols[i], 1e-300), 0.0))))
        print(f"{kind} T0={T0}: change at step {s} {old} -> {new}: increment difference / tolerance = {best:.3g}")
        assert best > 100.0, (kind, T0, s, best)
