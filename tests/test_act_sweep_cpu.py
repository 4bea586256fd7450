"""The activation sweep without a GPU: the oracle's hand-written act_fwd / act_bwd against the real torch.nn classes in float64
over each class's whole domain (tests/act_sweep.py: kinks, x*, the switch at 20, +-24, the extremes), the sweep's own
properties the GPU probes rely on, and the float32 emulation of the device's output-only derivative of GELU / SiLU / Mish /
Hardswish against the envelope the GPU probes hold the kernels to."""
import numpy as np
import pytest

import act_sweep as A
from oracle import aae_oracle as O

f32 = np.float32


@pytest.mark.parametrize("name", A.NAMES)
def test_sweep_holds_every_special_point_of_the_class(name):
    for rows, width in A.SHAPES:
        x = A.sweep(name, rows, width)
        assert x.shape == (rows, width) and x.dtype == f32 and np.isfinite(x).all()
        assert np.array_equal(x, A.sweep(name, rows, width))
        flat = x.ravel()
        for p in A.specials(name):
            p32 = f32(p)
            for q in (p32, np.nextafter(p32, f32(-np.inf)), np.nextafter(p32, f32(np.inf))):
                assert (flat == q).any(), (name, p, q)
            # (+ half a float32 step at 20: the outermost point rounds; the innermost may round onto the neighbour there)
            near = (np.abs(flat.astype(np.float64) - float(p32)) <= A.NEAR + 1e-6) & (flat != p32)
            assert near.sum() >= A.NEAR_N, (name, p, near.sum())
        for e in A.EXTREMES:
            assert (flat == f32(e)).any()
        grid = flat[(np.abs(flat) <= 24)]
        assert np.diff(np.sort(grid)).max() <= 48.0 / (rows * width // 2) + 1e-6      # no hole in [-24, 24]
        # position and magnitude are unrelated: no row or column is all of one kind
        assert np.abs(x).max(axis=1).min() > 6 and np.abs(x).min(axis=1).max() < 6
        assert np.abs(x).max(axis=0).min() > 2


@pytest.mark.parametrize("name", A.NAMES)
def test_oracle_activations_match_torch_in_float64_over_the_whole_domain(name):
    """O.act_fwd and O.act_bwd(.., g = 1) against getattr(torch.nn, name)() in float64 with autograd.  Points within 1e-3 of a
    kink but not on it are left out (the oracle's own float32 forms, x / 6 + 0.5 for one, may round such a point across the
    kink); a point ON a kink stays, torch's convention there is the reference.
    Forward |d| <= 1e-6 max(1, |y|), derivative |d| <= 2e-6: the worst cases over a 68 000-point sweep of [-24, 24] and the
    extremes were 2.9e-7 and 9.9e-7 - the bounds are those with headroom for another libm."""
    worst_f = worst_g = 0.0
    for rows, width in A.SHAPES:
        x = A.sweep(name, rows, width).ravel()
        x = x[~A.near_kink(name, x, 1e-3)]
        want_y, want_g = A.ref_single(name, x)
        y = O.act_fwd(name, x)
        g = O.act_bwd(name, x, y, np.ones_like(x))
        assert y.dtype == f32 and g.dtype == f32 and np.isfinite(y).all() and np.isfinite(g).all()
        ef = np.abs(y - want_y) / np.maximum(1.0, np.abs(want_y))
        eg = np.abs(g - want_g)
        worst_f, worst_g = max(worst_f, ef.max()), max(worst_g, eg.max())
        i, j = int(ef.argmax()), int(eg.argmax())
        print(f"{name} {rows}x{width}: forward {ef[i]:.2e} at x = {x[i]!r}; derivative {eg[j]:.2e} at x = {x[j]!r} (got {g[j]!r}, want {want_g[j]!r})")
        assert ef[i] <= 1e-6, (name, x[i], y[i], want_y[i])
        assert eg[j] <= 2e-6, (name, x[j], g[j], want_g[j])


@pytest.mark.parametrize("name", A.NAMES)
def test_sup_of_the_derivative_and_the_share_of_points_the_probes_leave_out(name):
    """What the GPU probes take from this module, on the reference alone: sup |f'| of the class bounds the float64 derivative
    over the sweep (and is not loose by more than 1 %), and for both scales and both shapes the points within 1e-4 of a kink in
    either layer (not on it) are at most 2 % of the case."""
    for rows, width in A.SHAPES:
        _, g = A.ref_single(name, A.sweep(name, rows, width).ravel())
        assert np.abs(g).max() <= A.SUP_DF[name] * (1 + 1e-7) and np.abs(g).max() >= 0.99 * A.SUP_DF[name], (name, np.abs(g).max())
        for s in A.SCALES:
            c = A.composite(name, rows, width, s)
            share = A.excluded(name, c["x"], c["u"]).mean()
            print(f"{name} {rows}x{width} s = {s:g}: {share:.4%} left out")
            assert share <= 0.02, (name, rows, width, s, share)
            assert np.isfinite(c["h2"]).all() and np.isfinite(c["d"]).all()


def _dense(name):
    xs = float(A.XSTAR[name])
    d = np.logspace(-7, 0.5, 4000)
    return np.concatenate([xs + d, xs - d, np.linspace(-24, 24, 40001), A.EXTREMES]).astype(f32)


@pytest.mark.parametrize("name", A.NM)
def test_emulated_inverse_keeps_the_envelope_the_device_is_held_to(name):
    """The float32 NumPy emulation of nm_mark / nm_grad_from_y (24 bracketed Newton steps on the branch the last bit names;
    Hardswish in closed form) against the float64 derivative of the real class: within act_sweep.eps_nm - max(far, min(near,
    c / |x - x*|)) - on 48 000 points (log-spaced distances of 1e-7 .. 3 from x* on both sides, [-24, 24], the extremes) and on
    the sweeps, for every model of the transcendental functions' error in act_sweep.MODELS: correctly rounded float32 and
    twelve sign patterns of erff / tanhf / log1pf at 4 units in the last place and __expf at 1 + |x| / 2.  The GPU probes hold
    the kernels to this same envelope: the bound comes from the algorithm and the functions' error bounds, not from a kernel."""
    xs = [_dense(name)] + [A.sweep(name, r, w).ravel() for r, w in A.SHAPES]
    for k, model in enumerate(A.MODELS):
        for x in xs:
            x = x[~A.near_kink(name, x, 1e-4)]
            _, want = A.ref_single(name, x)
            got = A.nm_grad_from_y32(name, A.nm_fwd32(name, x, model), model)
            assert np.isfinite(got).all()
            err, tol = np.abs(got - want), A.eps_nm(name, x)
            i = int((err / tol).argmax())
            print(f"{name} model {k}: worst {err[i]:.2e} of {tol[i]:.2e} at x = {x[i]!r} (x - x* = {x[i] - A.XSTAR[name]:.2e})")
            assert err[i] <= tol[i], (name, k, x[i], got[i], want[i], tol[i])
    # the envelope stays a real check: a wrong branch between 1e-2 and 1 from x* is an error of 2 |f'(x)|, over 4 x the envelope
    x = _dense(name)
    x = x[(np.abs(x - A.XSTAR[name]) > 1e-2) & (np.abs(x - A.XSTAR[name]) < 1)]
    _, want = A.ref_single(name, x)
    assert (2 * np.abs(want) > 4 * A.eps_nm(name, x)).all()
