"""Every activation class over its whole domain on each hidden-layer kernel family, through the C ABI.

Two element-wise probes per case (tests/act_sweep.py has the points and the tolerances).  A small fp32 model with n_hidden =
n_code = H, no condition, no dropout, whose hidden stacks are loaded as [identity, s I] with zero biases: an identity product
is exact on the fp32 pipe and on the three-term bf16 split alike, so a stack computes f(s f(x)) element by element and its
backward pass g f'(s f(x)) s f'(x) - the activation code of csrc/device_common.h and nothing else.

  decoder probe   aae_ae_decode_backward(zc = X): AAE_T_ACT_DH2 = f(s f(X)); dzc = g2 f'(s f(X)) s f'(X), g2 = dL/d(h2) of an
                  all-positive output layer (every document holds the same single item), taken from the float64 reference
  encoder probe   enc.lin1 column i = row i of X, document i = item i: AAE_T_ACT_A1 = X BIT FOR BIT (the probe feeds what it
                  claims), z = f(s f(X)), and after aae_ae_encoder_backward(dz = G): AAE_T_ACT_GA1 = G f'(s f(X)) s f'(X)

The reference is the same composite of the real torch.nn class in float64 with autograd - never the oracle, never a kernel.
Kernel paths: the six r1-r5 classes on the 4-row chain kernel (default), the wide-batch kernel (X16_ROWS = 16), the 16-row fp32
chain kernel (CHAIN16) and the per-layer GEMM epilogues (NO_CHAIN); the fourteen r6 classes on chain_kernel<.., true> (default)
and NO_CHAIN.  The first layer's activation runs in the enc_gather_kernel epilogue on every chain path.

Forward: |d| <= max(2e-6, 4 x the oracle's own error against float64 on the class's sweep) max(1, |y|).
Derivative (as the ratio to the upstream gradient): |s| L (eps(x) + eps(s f(x))) + 1e-5 |expected|, L = sup |f'|, eps = 1e-6 for
the sixteen classes whose derivative is a closed form in the output, and for GELU / SiLU / Mish / Hardswish the envelope of
the float32 emulation of the device's inverse under the error bounds of erff, tanhf, log1pf and __expf (act_sweep.eps_nm,
held by test_act_sweep_cpu.py; the bound the comment in device_common.h states).
A point ON a kink stays (torch's convention is the reference); a point within 1e-4 of a kink in either layer, not on it, is
left out (at most 2 % of a case: test_act_sweep_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import act_sweep as A
from oracle import aae_oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32

from act_sweep import N_ITEMS, enc_upstream, forward_tolerance, out_layer      # noqa: E402  (shared with the CPU test of the bf16 reference)

PATHS = {"default": None, "x16": ("X16_ROWS", 16), "chain16": ("CHAIN16", 1), "no_chain": ("NO_CHAIN", 1)}
CASES = [(n, p) for n in A.R15 for p in ("default", "x16", "chain16", "no_chain")] + \
        [(n, p) for n in A.R6 for p in ("default", "no_chain")]


@functools.lru_cache(maxsize=None)
def upstream(name, rows, H, s):
    """g2 = dL/d(h2) of the decoder probe in float64: mean BCE of sigmoid(h2 V3^T) against the one item every document holds."""
    c = A.composite(name, rows, H, s)
    V = out_layer(H).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-(c["h2"] @ V.T)))
    p[:, 0] -= 1.0
    g2 = (p / (rows * N_ITEMS)) @ V
    g2.setflags(write=False)
    return g2


def params(H, s, w1):
    eye, zero = np.eye(H, dtype=f32), np.zeros(H, dtype=f32)
    return {"enc.lin1.weight": w1, "enc.lin1.bias": zero, "enc.lin2.weight": f32(s) * eye, "enc.lin2.bias": zero,
            "enc.lin3.weight": eye, "enc.lin3.bias": zero, "dec.lin1.weight": eye, "dec.lin1.bias": zero,
            "dec.lin2.weight": f32(s) * eye, "dec.lin2.bias": zero, "dec.lin3.weight": out_layer(H),
            "dec.lin3.bias": np.zeros(N_ITEMS, dtype=f32)}


def make_model(name, path, rows, H):
    """The handle on the asked path - or a skip that names the call, if aae_create refuses the shape with AAE_EINVAL (no
    combination does today).  Any other error, and any error of a later call, fails the test."""
    from aaerec import _hip
    opt = PATHS[path]
    if opt:
        _hip.set_option(opt[0], opt[1])
    try:
        return _hip.HipAAE(N_ITEMS, H, H, cond_inc=0, max_batch=rows, activation=name, dropout=(0.0, 0.0), rng_mode="inject")
    except _hip.AaeHipError as e:
        if "error -1:" not in str(e):
            raise
        pytest.skip(f"aae_create on path {path} refused {rows} rows x {H}: {e}")
    finally:
        if opt:
            _hip.set_option(opt[0], None)     # (a handle reads its switches once, at creation)


def compare(report, what, name, path, s, c, got, want, tol, keep):
    """got against want within tol on the kept points; every miss goes to the report (worst ten printed), the worst error of
    the case to stdout (DESIGN.md's table is filled in from these lines)."""
    assert np.isfinite(got).all(), (what, name, path, s, "not finite at x =", c["x"][~np.isfinite(got)][:10])
    err = np.where(keep, np.abs(got - want), 0.0)
    i = np.unravel_index(int(err.argmax()), err.shape)
    print(f"ACTSWEEP {name} {path} {got.shape[0]}x{got.shape[1]} s={s:g} {what} worst {err[i]:.3e} at x = {c['x'][i]!r} "
          f"(tolerance there {np.broadcast_to(tol, err.shape)[i]:.3e})")
    bad = err > tol
    if bad.any():
        order = np.argsort((err / tol).ravel())[::-1][:10]
        lines = [f"{what}: {int(bad.sum())} of {int(keep.sum())} points beyond the tolerance; class {name}, path {path}, s = {s:g}"]
        for k in order:
            j = np.unravel_index(int(k), err.shape)
            if bad[j]:
                lines.append(f"    x = {c['x'][j]!r}  f(x) = {c['h1'][j]:.9g}  s f(x) = {c['u'][j]:.9g}  got {got[j]:.9g}  want {want[j]:.9g}"
                             f"  (|d| {err[j]:.3e} > {np.broadcast_to(tol, err.shape)[j]:.3e})")
        report.append("\n".join(lines))


def run_decoder_probe(m, name, path, rows, H, s, report):
    from aaerec import _hip
    c = A.composite(name, rows, H, s)
    g2 = upstream(name, rows, H, s)
    assert (g2 > 0).all() and g2.min() >= 0.25 * g2.max(), ("the upstream gradient is not of one sign and magnitude", g2.min(), g2.max())
    keep = ~A.excluded(name, c["x"], c["u"])
    m.load_params(params(H, s, np.zeros((H, N_ITEMS), dtype=f32)))      # (every backward call also runs the optimiser)
    csr = _hip.DeviceCSR.from_arrays(np.arange(rows + 1), np.zeros(rows, dtype=np.int32), np.ones(rows, dtype=f32), N_ITEMS, m.device)
    m.ae_encode(csr, 0, rows)       # opens the step
    dzc = m.ae_decode_backward(torch.from_numpy(c["x"].copy()))
    m.join()
    h2 = m.tensor(_hip.T_ACT_DH2)[:rows, :H].cpu().numpy().astype(np.float64)
    dzc = dzc.cpu().numpy().astype(np.float64)
    ftol = forward_tolerance(name, rows, H, s) * np.maximum(1.0, np.abs(c["h2"]))
    compare(report, "decoder forward", name, path, s, c, h2, c["h2"], ftol, keep)
    compare(report, "decoder derivative", name, path, s, c, dzc / g2, c["d"], A.ratio_tol(name, s, c["x"], c["u"], c["d"]), keep)


def run_encoder_probe(m, name, path, rows, H, s, report):
    from aaerec import _hip
    c = A.composite(name, rows, H, s)
    G = enc_upstream(rows, H)
    keep = ~A.excluded(name, c["x"], c["u"])
    w1 = np.zeros((H, N_ITEMS), dtype=f32)
    w1[:, :rows] = c["x"].T                                              # column i = row i of the sweep
    m.load_params(params(H, s, w1))
    csr = _hip.DeviceCSR.from_arrays(np.arange(rows + 1), np.arange(rows, dtype=np.int32), np.ones(rows, dtype=f32), N_ITEMS, m.device)
    z = m.ae_encode(csr, 0, rows)
    a1 = m.tensor(_hip.T_ACT_A1)[:rows, :H].cpu().numpy()
    m.ae_decode_backward(z)
    m.ae_encoder_backward(torch.from_numpy(G.copy()))
    m.join()
    assert np.array_equal(a1.view(np.uint32), c["x"].view(np.uint32)), \
        ("AAE_T_ACT_A1 is not the sweep bit for bit", name, path, c["x"][a1.view(np.uint32) != c["x"].view(np.uint32)][:10])
    z = z.cpu().numpy().astype(np.float64)
    ga1 = m.tensor(_hip.T_ACT_GA1)[:rows, :H].cpu().numpy().astype(np.float64)
    ftol = forward_tolerance(name, rows, H, s) * np.maximum(1.0, np.abs(c["h2"]))
    compare(report, "encoder forward", name, path, s, c, z, c["h2"], ftol, keep)
    compare(report, "encoder derivative", name, path, s, c, ga1 / G, c["d"], A.ratio_tol(name, s, c["x"], c["u"], c["d"]), keep)


@pytest.mark.parametrize("rows,H", A.SHAPES)
@pytest.mark.parametrize("name,path", CASES)
def test_activation_sweep(name, path, rows, H):
    m = make_model(name, path, rows, H)
    report = []
    try:
        for s in A.SCALES:
            run_decoder_probe(m, name, path, rows, H, s, report)
            run_encoder_probe(m, name, path, rows, H, s, report)
    finally:
        m.close()
    assert not report, "\n" + "\n".join(report)


# ---- bf16 mode (dtype = 'bf16') -------------------------------------------------------------------------------------------------
# The same sweeps, shapes and scales on a bf16 handle: bf16 mode has a kernel family of its own (the column-owner chain4 of the
# default path, the k-slice form, chain16x3_kernel<true>, chain_kernel<true, ..>, kGemmBf16 and its per-layer epilogues).  The
# reference is the same float64 composite with bf16_round where the mode applies it - act_sweep.composite_bf16 has the rounding
# points, derived from OracleAAE._linear / _mlp_bwd and held to the oracle's own run of these probes by test_act_sweep_cpu.py -
# and dec.lin3 made of bf16 values, so that the output-layer product rounds the activations alone.
# Forward: the fp32 sweep's tolerance after the last rounding; z = R(h2) against R of the reference (act_sweep.bf16_z).
# Derivative: the fp32 sweep's ratio_tol + 2^-7 |expected| (two bf16 roundings of the gradient, 2^-8 each).  Coarse against the
# fp32 sweep's 1e-6 - and still far inside a lost branch bit (the sign of f' left of x*), a wrong class dispatch, or an
# EXT = false instantiation (LeakyReLU's derivative for classes 6 - 19), which is what this test is for.
# An ambiguous point (h1 within its fp32 error of the midpoint of two bf16 values) may match either neighbour's continuation.
PATHS_BF16 = dict(PATHS, kslices=("CHAIN_KSLICES", 1))
CASES_BF16 = [(n, p) for n in A.R15 for p in ("default", "kslices", "x16", "chain16", "no_chain")] + \
             [(n, p) for n in A.R6 for p in ("default", "no_chain")]


def make_model_bf16(name, path, rows, H):
    """(no skip: bf16 mode refuses no shape or path of these cases, and an error of aae_create fails the test)"""
    from aaerec import _hip
    opt = PATHS_BF16[path]
    if opt:
        _hip.set_option(opt[0], opt[1])
    try:
        return _hip.HipAAE(N_ITEMS, H, H, cond_inc=0, max_batch=rows, activation=name, dropout=(0.0, 0.0), rng_mode="inject", dtype="bf16")
    finally:
        if opt:
            _hip.set_option(opt[0], None)


def compare_bf16(report, what, name, path, s, c, keep, got, want, tol):
    """got against want[k] within tol[k] on the kept points - continuation 0, and for an ambiguous point the better of the two;
    misses to the report, the worst error of the case to stdout (DESIGN.md's table)."""
    assert np.isfinite(got).all(), (what, name, path, s, "not finite at x =", c["x"][~np.isfinite(got)][:10])
    e = [np.abs(got - want[k]) for k in (0, 1)]
    pick = np.where(c["amb"] & (e[1] / tol[1] < e[0] / tol[0]), 1, 0)
    err = np.where(keep, np.where(pick == 1, e[1], e[0]), 0.0)
    tl = np.where(pick == 1, tol[1], tol[0])
    i = np.unravel_index(int((err / tl).argmax()), err.shape)
    print(f"ACTSWEEP bf16 {name} {path} {got.shape[0]}x{got.shape[1]} s={s:g} {what} worst {err[i]:.3e} at x = {c['x'][i]!r} "
          f"(tolerance there {tl[i]:.3e})")
    bad = err > tl
    if bad.any():
        lines = [f"{what}: {int(bad.sum())} of {int(keep.sum())} points beyond the tolerance; class {name}, path {path}, s = {s:g}, bf16"]
        for k in np.argsort((err / tl).ravel())[::-1][:10]:
            j = np.unravel_index(int(k), err.shape)
            if bad[j]:
                lines.append(f"    x = {c['x'][j]!r}  f = {c['h1'][j]:.9g}  s R(f) = {c['u'][0][j]:.9g}  got {got[j]:.9g}  want {want[0][j]:.9g}"
                             f"{' or %.9g' % want[1][j] if c['amb'][j] else ''}  (|d| {err[j]:.3e} > {tl[j]:.3e})")
        report.append("\n".join(lines))


def run_decoder_probe_bf16(m, name, path, rows, H, s, report):
    from aaerec import _hip
    c = A.composite_bf16(name, rows, H, s, "decoder")
    g2 = A.upstream_bf16(name, rows, H, s)
    assert (g2 > 0).all() and g2.min() >= 0.25 * g2.max(), ("the upstream gradient is not of one sign and magnitude", g2.min(), g2.max())
    keep = ~A.excluded_bf16(name, c)
    p = params(H, s, np.zeros((H, N_ITEMS), dtype=f32))
    p["dec.lin3.weight"] = A.out_layer_bf16(H)
    m.load_params(p)
    csr = _hip.DeviceCSR.from_arrays(np.arange(rows + 1), np.zeros(rows, dtype=np.int32), np.ones(rows, dtype=f32), N_ITEMS, m.device)
    m.ae_encode(csr, 0, rows)
    dzc = m.ae_decode_backward(torch.from_numpy(c["x"].copy()))
    m.join()
    h2 = m.tensor(_hip.T_ACT_DH2)[:rows, :H].cpu().numpy().astype(np.float64)
    dzc = dzc.cpu().numpy().astype(np.float64)
    compare_bf16(report, "decoder forward", name, path, s, c, keep, h2, c["h2"], [A.bf16_forward_tol(name, rows, H, s, c, k) for k in (0, 1)])
    compare_bf16(report, "decoder derivative", name, path, s, c, keep, dzc / g2, c["d"], [A.bf16_ratio_tol(name, s, c, k) for k in (0, 1)])


def run_encoder_probe_bf16(m, name, path, rows, H, s, report):
    from aaerec import _hip
    c = A.composite_bf16(name, rows, H, s, "encoder")
    G = enc_upstream(rows, H)
    keep = ~A.excluded_bf16(name, c)
    w1 = np.zeros((H, N_ITEMS), dtype=f32)
    w1[:, :rows] = c["x"].T
    p = params(H, s, w1)
    p["dec.lin3.weight"] = A.out_layer_bf16(H)
    m.load_params(p)
    csr = _hip.DeviceCSR.from_arrays(np.arange(rows + 1), np.arange(rows, dtype=np.int32), np.ones(rows, dtype=f32), N_ITEMS, m.device)
    z = m.ae_encode(csr, 0, rows)
    a1 = m.tensor(_hip.T_ACT_A1)[:rows, :H].cpu().numpy()
    m.ae_decode_backward(z)
    m.ae_encoder_backward(torch.from_numpy(G.copy()))
    m.join()
    assert np.array_equal(a1.view(np.uint32), c["x"].view(np.uint32)), \
        ("AAE_T_ACT_A1 is not the sweep bit for bit: the sparse first layer rounds nothing", name, path, c["x"][a1.view(np.uint32) != c["x"].view(np.uint32)][:10])
    z = z.cpu().numpy().astype(np.float64)
    ga1 = m.tensor(_hip.T_ACT_GA1)[:rows, :H].cpu().numpy().astype(np.float64)
    zt = [A.bf16_z(name, rows, H, s, c, k) for k in (0, 1)]
    compare_bf16(report, "encoder forward", name, path, s, c, keep, z, [zt[0][0], zt[1][0]], [zt[0][1], zt[1][1]])
    compare_bf16(report, "encoder derivative", name, path, s, c, keep, ga1 / G, c["d"], [A.bf16_ratio_tol(name, s, c, k) for k in (0, 1)])


@pytest.mark.parametrize("rows,H", A.SHAPES)
@pytest.mark.parametrize("name,path", CASES_BF16)
def test_activation_sweep_bf16(name, path, rows, H):
    m = make_model_bf16(name, path, rows, H)
    report = []
    try:
        for s in A.SCALES:
            run_decoder_probe_bf16(m, name, path, rows, H, s, report)
            run_encoder_probe_bf16(m, name, path, rows, H, s, report)
    finally:
        m.close()
    assert not report, "\n" + "\n".join(report)
