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


# ---- bf16 mode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMES)
def test_bf16_sweep_leaves_out_at_most_two_per_cent(name):
    """On the reference alone, for both probes, shapes and scales: the points that may match either continuation (h1 within its
    fp32 error of the midpoint of two bf16 values, act_sweep.composite_bf16) - those of them whose two continuations differ by
    more than the tolerances, act_sweep.weakened - plus the kink exclusions are at most 2 % of a case; expected about
    tolerance / half the bf16 spacing = 2e-6 / 2^-9 .. 2^-8 = 0.05 - 0.1 % for the former.  Every class but GELU stays under 0.6 %
    with ALL its ambiguous points counted, which is asserted too.  Both continuations are finite."""
    for rows, width in A.SHAPES:
        for s in A.SCALES:
            for probe in ("decoder", "encoder"):
                c = A.composite_bf16(name, rows, width, s, probe)
                amb, out = c["amb"].mean(), A.excluded_bf16(name, c).mean()
                print(f"{name} {rows}x{width} s = {s:g} {probe}: {amb:.4%} ambiguous, {out:.4%} left out")
                assert (A.weakened(name, rows, width, s, c) | A.excluded_bf16(name, c)).mean() <= 0.02, (name, rows, width, s, probe, amb, out)
                assert name == "GELU" or c["amb"].mean() <= 0.006, (name, rows, width, s, probe, amb, out)
                assert all(np.isfinite(c[k][j]).all() for k in ("u", "h2", "d") for j in (0, 1))
                # continuation 0 is the mode's rounding: s R(h1) with the oracle's bf16_round on the float32 h1
                assert np.array_equal(c["u"][0], s * O.bf16_round(c["h1"].astype(f32)).astype(np.float64))
                # an ambiguous point's two continuations are neighbouring bf16 values around h1
                a = c["amb"]
                lo, hi = np.minimum(c["u"][0], c["u"][1])[a] / s, np.maximum(c["u"][0], c["u"][1])[a] / s
                lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
                assert (np.abs(hi - lo) <= 2.0 ** -7 * np.abs(hi) + 1e-37).all() and (lo != hi).all()      # (+ the subnormal bf16 values)


def _probe_model(name, H, s, w1):
    eye, zero = np.eye(H, dtype=f32), np.zeros(H, dtype=f32)
    p = {"enc.lin1.weight": w1, "enc.lin1.bias": zero, "enc.lin2.weight": f32(s) * eye, "enc.lin2.bias": zero,
         "enc.lin3.weight": eye, "enc.lin3.bias": zero, "dec.lin1.weight": eye, "dec.lin1.bias": zero,
         "dec.lin2.weight": f32(s) * eye, "dec.lin2.bias": zero, "dec.lin3.weight": A.out_layer_bf16(H),
         "dec.lin3.bias": np.zeros(A.N_ITEMS, dtype=f32)}
    return O.OracleAAE(p, activation=name, dropout=(0.0, 0.0), bf16=True)


@pytest.mark.parametrize("name", A.NAMES)
def test_bf16_reference_rounds_where_the_oracle_rounds(name):
    """The rounding points of act_sweep.composite_bf16 / upstream_bf16, held to the mode's definition: the probes' model in
    OracleAAE(bf16=True) - _mlp_fwd, _bce, _mlp_bwd as they stand - gives the reference's h2, z, dzc / g2 and ga1 / G within the
    tolerances tests/test_act_sweep_gpu.py holds the kernels to (the oracle's activations are float32 NumPy: the forward
    tolerance is 4 x their error by construction; its derivatives are written in x).  A rounding the reference puts elsewhere -
    the first decoder layer's input left unrounded, z taken before its rounding, a product whose gradient operand is not
    rounded - moves these by up to 2^-8 relative on most points."""
    for rows, H in A.SHAPES:
        for s in A.SCALES:
            # decoder probe: zc = X through dec.lin1 = I, dec.lin2 = s I, the output layer; every document holds item 0
            c = A.composite_bf16(name, rows, H, s, "decoder")
            keep = ~A.excluded_bf16(name, c)
            ora = _probe_model(name, H, s, np.zeros((H, A.N_ITEMS), dtype=f32))
            ip, idx, val = np.arange(rows + 1), np.zeros(rows, dtype=np.int32), np.ones(rows, dtype=f32)
            logits, dc = ora._mlp_fwd("dec", c["x"], None)
            _, glog, _ = ora._bce(logits, ip, idx, val)
            _, _, gzc = ora._mlp_bwd("dec", glog, dc)
            g2 = A.upstream_bf16(name, rows, H, s)
            assert (g2 > 0).all() and g2.min() >= 0.25 * g2.max()
            ef = A.bf16_errors(c, keep, dc["h2"].astype(np.float64), "h2", lambda k: A.bf16_forward_tol(name, rows, H, s, c, k))
            ed = A.bf16_errors(c, keep, gzc.astype(np.float64) / g2, "d", lambda k: A.bf16_ratio_tol(name, s, c, k))
            assert ef.max() <= 1 and ed.max() <= 1, (name, rows, H, s, "decoder", ef.max(), ed.max(), c["x"][np.unravel_index(ed.argmax(), ed.shape)])
            # encoder probe: enc.lin1 column i = row i of X, document i = item i
            c = A.composite_bf16(name, rows, H, s, "encoder")
            keep = ~A.excluded_bf16(name, c)
            w1 = np.zeros((H, A.N_ITEMS), dtype=f32)
            w1[:, :rows] = c["x"].T
            ora = _probe_model(name, H, s, w1)
            z, ec = ora.encode(np.arange(rows + 1), np.arange(rows, dtype=np.int32), np.ones(rows, dtype=f32), None)
            assert np.array_equal(ec["a1"].view(np.uint32), c["x"].view(np.uint32))
            G = A.enc_upstream(rows, H)
            _, ga1, _ = ora._mlp_bwd("enc", G, ec, need_dx=False)
            zt = [A.bf16_z(name, rows, H, s, c, k) for k in (0, 1)]
            ez = [np.abs(z - zt[k][0]) / zt[k][1] for k in (0, 1)]
            ez = np.where(keep, np.where(c["amb"], np.minimum(ez[0], ez[1]), ez[0]), 0.0)
            ed = A.bf16_errors(c, keep, ga1.astype(np.float64) / G, "d", lambda k: A.bf16_ratio_tol(name, s, c, k))
            assert ez.max() <= 1 and ed.max() <= 1, (name, rows, H, s, "encoder", ez.max(), ed.max(), c["x"][np.unravel_index(ed.argmax(), ed.shape)])
