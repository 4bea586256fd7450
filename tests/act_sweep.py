"""The activation sweep shared by tests/test_act_sweep_cpu.py and tests/test_act_sweep_gpu.py: the points, the float64
torch.nn reference of the two-layer composite the probes run, the exclusion rule around the kinks, the tolerances, and a float32
NumPy emulation of the device's output-only derivative of the four non-monotone classes (csrc/device_common.h nm_grad_from_y).
Plain NumPy / torch on the CPU: nothing here touches the library."""
import functools

import numpy as np
import torch

f32 = np.float32

R15 = ["ReLU", "SELU", "Tanh", "Sigmoid", "ELU", "LeakyReLU"]                     # every chain kernel carries them
R6 = ["Softplus", "Hardtanh", "ReLU6", "CELU", "Softsign", "Hardsigmoid", "LogSigmoid", "Softshrink", "Hardshrink", "Identity",
      "GELU", "SiLU", "Mish", "Hardswish"]                                      # chain_kernel<.., true> and the per-layer epilogues
NAMES = R15 + R6
NM = ["GELU", "SiLU", "Mish", "Hardswish"]

# where the derivative of the class jumps (ELU / CELU at alpha = 1 are C1 at 0; Softplus' switch at 20 moves f and f' by 2e-9)
KINKS = {"ReLU": [0.0], "SELU": [0.0], "LeakyReLU": [0.0], "Hardtanh": [-1.0, 1.0], "ReLU6": [0.0, 6.0], "Hardsigmoid": [-3.0, 3.0],
         "Softshrink": [-0.5, 0.5], "Hardshrink": [-0.5, 0.5], "Hardswish": [-3.0, 3.0]}
# argmin of the non-monotone classes: device_common.h nm_xstar, digit for digit
XSTAR = {"GELU": f32(-0.75179160), "SiLU": f32(-1.27846455), "Mish": f32(-1.19245934), "Hardswish": f32(-1.5)}
# sup |f'| (SELU: scale * alpha, the left limit at 0; GELU / SiLU / Mish: the overshoot of f' beyond 1; Hardswish: 1.5 at x = 3);
# test_act_sweep_cpu.py holds them against the float64 reference
SUP_DF = {n: 1.0 for n in NAMES}
SUP_DF.update({"SELU": 1.7580993408473766, "Sigmoid": 0.25, "Hardsigmoid": 1.0 / 6.0, "GELU": 1.12891, "SiLU": 1.0999, "Mish": 1.0894,
               "Hardswish": 1.5})
EXTREMES = [-90.0, -40.0, 30.0, 88.0]
NEAR, NEAR_N = 1e-2, 200
SHAPES = [(64, 40), (20, 207)]
SCALES = [1.0, -2.0]


def specials(name):
    pts = [0.0] + KINKS.get(name, [])
    if name in XSTAR:
        pts.append(float(XSTAR[name]))
    if name in ("Softplus", "Mish"):
        pts.append(20.0)
    return sorted(set(pts))


def sweep(name, rows, width):
    """rows x width float32 pre-activations for one class: every special point of the class (0, the kinks, x*, the switch at 20)
    with its two float32 neighbours and NEAR_N points within +-NEAR of it, the extremes, and an even grid on [-24, 24] for the
    rest; shuffled with a fixed seed, so that row / column and magnitude are unrelated.

    Around a kink the near points are evenly spaced (the +-1e-4 band the device tests leave out then holds two of them); around
    a smooth special point - x* above all - their distance grows quadratically from 1e-6, where the inverse is worst conditioned.
    LeakyReLU takes 30 of the 200 below 0 instead of 100: its slope of 0.01 maps ALL of (-1e-2, 0) into the second layer's own
    +-1e-4 band around 0, where the device tests leave a point out whatever it is - the other 170 go where they are tested."""
    total = rows * width
    pts = []
    for p in specials(name):
        p32 = f32(p)
        pts += [p32, np.nextafter(p32, f32(-np.inf)), np.nextafter(p32, f32(np.inf))]
        below = 30 if name == "LeakyReLU" else NEAR_N // 2
        for n, sign in ((below, -1.0), (NEAR_N - below, 1.0)):
            k = np.arange(n, dtype=np.float64)
            d = NEAR * (k + 0.5) / n if p in KINKS.get(name, []) else 1e-6 + (NEAR - 1e-6) * (k / (n - 1)) ** 2
            pts += list((float(p32) + sign * d).astype(f32))
    pts += [f32(e) for e in EXTREMES]
    grid = np.linspace(-24.0, 24.0, total - len(pts)).astype(f32)
    x = np.concatenate([np.asarray(pts, dtype=f32), grid])
    assert x.size == total and grid.size >= total // 2
    return np.random.default_rng(20).permutation(x).reshape(rows, width)


def module(name):
    return getattr(torch.nn, name)()


def ref_single(name, x):
    """f(x), f'(x) of the real class in float64 (autograd)."""
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    y = module(name)(t)
    y.sum().backward()
    return y.detach().numpy(), t.grad.numpy()


@functools.lru_cache(maxsize=None)
def composite(name, rows, width, s):
    """The probes' element-wise composite on the sweep in float64: x, h1 = f(x), u = s h1, h2 = f(u), d = dh2/dx (autograd;
    torch's convention wherever a point sits on a kink).  Read-only arrays, shared by every test that needs them."""
    x = sweep(name, rows, width)
    t = torch.tensor(x.astype(np.float64), requires_grad=True)
    f = module(name)
    h1 = f(t)
    u = s * h1
    h2 = f(u)
    h2.sum().backward()
    out = dict(x=x, h1=h1.detach().numpy(), u=u.detach().numpy(), h2=h2.detach().numpy(), d=t.grad.numpy())
    for v in out.values():
        v.setflags(write=False)
    return out


def near_kink(name, v, band):
    """within `band` of a kink of the class, but not on it"""
    v = np.asarray(v, dtype=np.float64)
    m = np.zeros(v.shape, dtype=bool)
    for k in KINKS.get(name, []):
        m |= (np.abs(v - k) <= band) & (v != k)
    return m


def excluded(name, x, u, band=1e-4):
    """A point within 1e-4 of a kink in either layer, but not on it: a one-ulp difference of the forward value flips its branch
    legitimately."""
    return near_kink(name, x, band) | near_kink(name, u, band)


# ---- float32 emulation of device_common.h's inverse (nm_mark / nm_f_df / nm_grad_from_y) -----------------------------------------
# The ALGORITHM in float32, not the device's arithmetic: with model = None every transcendental is NumPy's / SciPy's (erf in
# float64, rounded), i.e. correctly rounded float32.  The device calls erff, tanhf, log1pf and the __expf intrinsic instead; an
# Intrinsics model stands in for those: each result is moved by the function's error bound, up or down by a fixed hash of the
# argument's bits (a function of x alone, as on the device: the same x gives the same value in every Newton step).
#   erff, tanhf, log1pf   LIB_ULPS = 4 units in the last place (the largest figure HIP's math tables give for these three)
#   __expf(x)             v_exp_f32(x log2 e): one unit for the instruction, and the rounding of the product x log2 e - half a
#                         unit of |x| log2 e - goes through 2^t as a relative error of ln 2 times that: 1 + |x| / 2 units
LIB_ULPS = 4.0


class Intrinsics:
    def __init__(self, salt):
        self.salt = np.uint32((salt * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF)

    def move(self, v, x, ulps, tag):
        bits = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
        with np.errstate(over="ignore"):
            h = ((bits ^ self.salt ^ np.uint32(tag * 0x85EBCA6B & 0xFFFFFFFF)) * np.uint32(2654435761)) >> np.uint32(31)
        sign = np.where(h == 1, 1.0, -1.0)
        return (v.astype(np.float64) * (1.0 + sign * ulps * 2.0 ** -23)).astype(f32)


def _exp32(x, model):
    with np.errstate(over="ignore", under="ignore"):
        v = np.exp(x.astype(f32))
    return v if model is None else model.move(v, x, 1.0 + 0.5 * np.abs(x.astype(np.float64)), 1)


def _lib32(fn, x, model, tag, saturates=False):
    """(saturates: erff and tanhf return exactly +-1 where the function rounds to it, and never more)"""
    with np.errstate(over="ignore", under="ignore"):
        v = fn(x.astype(f32)).astype(f32)
    if model is None:
        return v
    m = model.move(v, x, LIB_ULPS, tag)
    return np.where(np.abs(v) == 1, v, np.clip(m, f32(-1), f32(1))).astype(f32) if saturates else m


def _erf32(x, model):
    from scipy.special import erf
    return _lib32(lambda t: erf(t.astype(np.float64)), x, model, 2, saturates=True)


def _sig32(x, model=None):
    x = x.astype(f32)
    e = _exp32(-np.abs(x), model)
    return np.where(x >= 0, f32(1) / (f32(1) + e), e / (f32(1) + e)).astype(f32)


def _softplus32(x, model=None):
    return np.where(x > 20, x, _lib32(np.log1p, _exp32(np.minimum(x, f32(20)), model), model, 3)).astype(f32)


def nm_f_df32(name, x, model=None):
    x = x.astype(f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if name == "GELU":
            cdf = f32(0.5) * (f32(1) + _erf32(x * f32(0.70710678118654752), model))
            pdf = f32(0.3989422804014327) * _exp32(f32(-0.5) * x * x, model)
            return (x * cdf).astype(f32), (cdf + x * pdf).astype(f32)
        if name == "SiLU":
            sg = _sig32(x, model)
            return (x * sg).astype(f32), (sg * (f32(1) + x * (f32(1) - sg))).astype(f32)
        t, sg = _lib32(np.tanh, _softplus32(x, model), model, 4, saturates=True), _sig32(x, model)
        return (x * t).astype(f32), (t + x * sg * (f32(1) - t * t)).astype(f32)


def nm_fwd32(name, x, model=None):
    """act_fwd of a non-monotone class: the output with the branch bit in its last bit."""
    x = x.astype(f32)
    if name == "Hardswish":
        y = (x * np.clip(x + f32(3), f32(0), f32(6)) * f32(1.0 / 6.0)).astype(f32)
    elif name == "GELU":
        y = (x * f32(0.5) * (f32(1) + _erf32(x * f32(0.70710678118654752), model))).astype(f32)
    else:
        y = nm_f_df32(name, x, model)[0]
    u = (y.view(np.uint32) & np.uint32(0xFFFFFFFE)) | (x < XSTAR[name]).astype(np.uint32)
    return u.view(f32)


def nm_grad_from_y32(name, ym, model=None):
    """nm_grad_from_y: f'(x) from the marked output alone - 24 bracketed Newton steps, Hardswish in closed form."""
    ym = np.ascontiguousarray(ym, dtype=f32)
    bits = ym.view(np.uint32)
    left = (bits & np.uint32(1)) != 0
    ybits = bits & np.uint32(0xFFFFFFFE)
    y = ybits.view(f32)
    if name == "Hardswish":
        r = (np.sqrt(np.maximum(f32(9) + f32(24) * y, f32(0))) * f32(1.0 / 6.0)).astype(f32)
        out = np.where(left, -r, r)
        out = np.where(left & (y == 0), f32(0), out)
        return np.where(y >= 3, f32(1), out).astype(f32)
    xs = XSTAR[name]
    lo = np.where(left, f32(-40), xs).astype(f32)
    hi = np.where(left, xs, np.maximum(y, f32(0)) + f32(2)).astype(f32)
    x = np.where(left, xs - f32(1), np.maximum(y, xs + f32(0.5))).astype(f32)
    with np.errstate(all="ignore"):
        for _ in range(24):
            f, df = nm_f_df32(name, x, model)
            r = f - y
            above = np.where(left, r > 0, r < 0)
            lo, hi = np.where(above, x, lo), np.where(above, hi, x)
            xn = (x - r / df).astype(f32)
            x = np.where((xn > lo) & (xn < hi), xn, f32(0.5) * (lo + hi)).astype(f32)
    return nm_f_df32(name, x, model)[1]


MODELS = [None] + [Intrinsics(k) for k in range(12)]


# ---- tolerances ----------------------------------------------------------------------------------------------------------------
# The error of f'(x) that the inverse of a non-monotone class leaves, as an envelope in the distance from x*:
#     eps(v) = max(far, min(near, c / |v - x*|))
# The stored output carries an error eta (its rounding, the branch bit, the error of the functions it was computed with).
# Around x*, y - y* = f''/2 (x - x*)^2: the inverse cannot tell x from x* within sqrt(2 eta / f''), which costs f'' times that in
# f' (`near`); beyond, it lands eta / |f'(x)| = eta / (f'' |x - x*|) away, which costs eta / |x - x*| (`c`); far from x* what is
# left is the evaluation of f and f' themselves (`far`: GELU's 1 + erf(x / sqrt 2) cancels on the left branch).
# The constants are 1.5 times the maxima of the emulation above against float64 over 48 000 points and the sweeps, taken over
# MODELS: correctly rounded float32 and twelve sign patterns of the functions' error bounds (a sample of the patterns, hence
# the 1.5; test_act_sweep_cpu.py holds every model to them).  They come from the algorithm and the functions' published error bounds, not from a kernel; the GPU
# probes hold the kernels to them as they stand.  (Correctly rounded float32 alone gives: near 2.2e-4, c 1.3e-7, far 1.6e-5 for
# GELU and 6e-6 for SiLU / Mish; Hardswish's closed form calls no such function.)
NM_NEAR = {"GELU": 6.5e-4, "SiLU": 4e-4, "Mish": 9.5e-4, "Hardswish": 1.8e-4}
NM_C = {"GELU": 5.5e-7, "SiLU": 3.5e-7, "Mish": 1.8e-6, "Hardswish": 1e-7}
NM_FAR = {"GELU": 1.5e-4, "SiLU": 3e-5, "Mish": 4.5e-5, "Hardswish": 1.7e-6}


def eps_nm(name, v):
    dist = np.abs(np.asarray(v, dtype=np.float64) - float(XSTAR[name]))
    with np.errstate(divide="ignore"):
        return np.maximum(NM_FAR[name], np.minimum(NM_NEAR[name], NM_C[name] / dist))


def eps_df(name, v):
    """The bound on the error of the device's f'(v), written through the stored output: 1e-6 for the sixteen classes whose
    derivative is a closed form in the output, the emulation's envelope for the four inverted ones."""
    v = np.asarray(v, dtype=np.float64)
    return eps_nm(name, v) if name in NM else np.full(v.shape, 1e-6)


def ratio_tol(name, s, x, u, expected):
    """|s| L (eps(x) + eps(s f(x))) + 1e-5 |expected|: the bound of one layer's derivative, propagated through f'(u) s f'(x) with
    |f'| <= L, plus the output-layer product that feeds the upstream gradient."""
    return abs(s) * SUP_DF[name] * (eps_df(name, x) + eps_df(name, u)) + 1e-5 * np.abs(expected)


# ---- the probes' fixed parts (tests/test_act_sweep_gpu.py; tests/test_act_sweep_cpu.py runs the bf16 reference below against the
# oracle on the same model) --------------------------------------------------------------------------------------------------
N_ITEMS = 2048      # the output layer: logits = h2 . u / N stay within +-1 for every class (asserted on the reference)


@functools.lru_cache(maxsize=None)
def out_layer(H):
    """dec.lin3: all positive, entries in [0.5, 1.5] / N."""
    w = (np.random.default_rng(7).uniform(0.5, 1.5, size=(N_ITEMS, H)) / N_ITEMS).astype(f32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def enc_upstream(rows, H):
    rng = np.random.default_rng(11)
    g = (rng.uniform(0.5, 1.5, size=(rows, H)) * rng.choice([-1.0, 1.0], size=(rows, H))).astype(f32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def forward_tolerance(name, rows, H, s):
    """max(2e-6, 4 x the oracle's own error of the composite against float64 on this sweep), relative to max(1, |y|)."""
    from oracle import aae_oracle as O
    c = composite(name, rows, H, s)
    y = O.act_fwd(name, (f32(s) * O.act_fwd(name, c["x"])).astype(f32))
    keep = ~excluded(name, c["x"], c["u"])
    own = (np.abs(y - c["h2"]) / np.maximum(1.0, np.abs(c["h2"])))[keep].max()
    return max(2e-6, 4.0 * float(own))


# ---- bf16 mode (dtype = 'bf16'): the same composite with bf16_round where the mode applies it ---------------------------------
# The rounding points are OracleAAE._linear's and _mlp_bwd's (oracle/aae_oracle.py): a Linear layer's forward product and its dX
# product take both operands rounded, the sparse first encoder layer takes none.  On the probes' model ([identity, s I] stacks,
# zero biases; 1 and s = 1, -2 are bf16 values, so a product has one non-zero term and is exact):
#   decoder probe   dec.lin1 = I rounds its input: h1 = f(R(X));  dec.lin2 = s I rounds h1: h2 = f(s R(h1)) = AAE_T_ACT_DH2;  the
#                   output layer rounds h2 and G = dL/dlogits: g2 = R(G) V (V itself made of bf16 values for this test);  dX of
#                   dec.lin2 rounds ga2 = g2 f'(u), dX of dec.lin1 rounds ga1 = s R(ga2) f'(R(X)):  dzc = R(ga1)
#   encoder probe   the first layer is not rounded: AAE_T_ACT_A1 = X bit for bit, h1 = f(X);  enc.lin2 rounds h1: h2 = f(s R(h1));
#                   enc.lin3 = I rounds h2: z = R(h2);  backward from dz = G: dX of enc.lin3 rounds G, dX of enc.lin2 rounds
#                   ga2 = R(G) f'(u):  AAE_T_ACT_GA1 = s R(ga2) f'(X)
# So the expected ratio to the upstream gradient is the plain f'(u) s f'(x) at the rounded points, and the gradient passes two
# roundings on its way down.  bf16 keeps 8 significant bits: a rounding moves a value by up to half a unit in its last place,
# 2^-8 relative just above a power of two (2^-9 just below the next) - so 2 x 2^-8 = 2^-7 |expected| on top of the fp32 sweep's
# ratio_tol (derived, not measured; test_act_sweep_cpu.py holds the oracle's own run of the probes to it, and finds single
# roundings of 0.96 x 2^-8).  Where an output is itself rounded (z = R(h2)) it is compared with R of the reference: bf16_z.
# A device h1 that differs from the reference by fp32 units can land on the other side of a bf16 rounding boundary: a point is
# AMBIGUOUS when its reference h1 lies within the fp32 error of h1 of the midpoint of two bf16 values, and may then match either
# neighbour's continuation.  That error is the fp32 sweep's forward tolerance RELATIVE to |h1| - not to max(1, |h1|), the form
# it takes where errors of both layers add up: below 1 the bf16 spacing shrinks with |h1|, and an absolute 2e-6 would call a
# third of the grid ambiguous for every class that decays towards 0 (Sigmoid, Softplus, SiLU ..) - plus what a class computes
# with an ABSOLUTE error: GELU's 1 + erf cancels on the left (0.5 |x| times erff's 4 units at 1), Hardsigmoid's x / 6 + 0.5 is
# rounded at 0.5, and results below the smallest normal float32 may be flushed.
AMBIGUITY_FLOOR = {"GELU": lambda x: 0.5 * np.abs(x) * LIB_ULPS * 2.0 ** -24, "Hardsigmoid": lambda x: 2.0 ** -24 + 0.0 * x}
BF16_EPS = 2.0 ** -8


def bf16_values(h):
    """(R(h), the bf16 neighbour of R(h) on h's side, their midpoint) of float64 h, as float64"""
    from oracle.aae_oracle import bf16_round
    h32 = np.ascontiguousarray(h, dtype=f32)
    r = bf16_round(h32)
    bits = r.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    up = np.abs(np.asarray(h, dtype=np.float64)) > np.abs(r.astype(np.float64))
    step = np.where(up, np.uint32(0x10000), np.where(mag >= np.uint32(0x10000), np.uint32(0xFFFF0000), np.uint32(0)))       # (+1 / -1 bf16 unit of magnitude)
    with np.errstate(over="ignore"):
        other = (bits + step).view(f32)
    r64, o64 = r.astype(np.float64), other.astype(np.float64)
    return r64, o64, 0.5 * (r64 + o64)


def _f_df(name, v):
    t = torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True)
    y = module(name)(t)
    y.sum().backward()
    return y.detach().numpy(), t.grad.numpy()


@functools.lru_cache(maxsize=None)
def composite_bf16(name, rows, width, s, probe):
    """The probe's element-wise composite in bf16 mode, float64 between the roundings: xin (what the first activation sees:
    R(x) in the decoder probe, x in the encoder probe), h1 = f(xin), the ambiguity mask `amb`, and for both continuations k = 0
    (the nearest bf16 value of h1) and 1 (its neighbour across the midpoint): u[k] = s R_k(h1), h2[k] = f(u[k]),
    d[k] = f'(u[k]) s f'(xin).  Read-only arrays."""
    from oracle.aae_oracle import bf16_round
    x = sweep(name, rows, width)
    xin = (bf16_round(x) if probe == "decoder" else x).astype(np.float64)
    h1, d1 = _f_df(name, xin)
    r, other, mid = bf16_values(h1)
    tol1 = forward_tolerance(name, rows, width, s) * np.abs(h1) + 2.0 ** -126 + AMBIGUITY_FLOOR.get(name, lambda v: 0.0 * v)(xin)
    amb = (np.abs(h1 - mid) <= tol1) & (other != r)
    out = dict(x=x, xin=xin, h1=h1, amb=amb, u=[], h2=[], d=[])
    for rk in (r, other):
        u = s * rk
        h2, d2 = _f_df(name, u)
        out["u"].append(u), out["h2"].append(h2), out["d"].append(d2 * s * d1)
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return out


def excluded_bf16(name, c):
    """Left out of a bf16 case: within 1e-4 of a kink, not on it, in either layer - for an ambiguous point in either continuation."""
    return near_kink(name, c["xin"], 1e-4) | near_kink(name, c["u"][0], 1e-4) | (c["amb"] & near_kink(name, c["u"][1], 1e-4))


@functools.lru_cache(maxsize=None)
def out_layer_bf16(H):
    from oracle.aae_oracle import bf16_round
    w = bf16_round(out_layer(H))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def upstream_bf16(name, rows, H, s):
    """g2 = dL/d(h2) of the decoder probe in bf16 mode: mean BCE of sigmoid(R(h2) V^T) against the one item every document holds,
    G = dL/dlogits rounded, g2 = R(G) V - float64 between the roundings."""
    from oracle.aae_oracle import bf16_round
    c = composite_bf16(name, rows, H, s, "decoder")
    V = out_layer_bf16(H).astype(np.float64)
    h2 = bf16_round(c["h2"][0].astype(f32)).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-(h2 @ V.T)))
    p[:, 0] -= 1.0
    G = bf16_round((p / (rows * N_ITEMS)).astype(f32)).astype(np.float64)
    g2 = G @ V
    g2.setflags(write=False)
    return g2


def bf16_errors(c, keep, got, want_key, tol_fn):
    """|got - want| / tolerance per point: against continuation 0, and for an ambiguous point the better of the two."""
    e = [np.abs(got - c[want_key][k]) / tol_fn(k) for k in (0, 1)]
    return np.where(keep, np.where(c["amb"], np.minimum(e[0], e[1]), e[0]), 0.0)


def bf16_forward_tol(name, rows, H, s, c, k):
    """The fp32 sweep's forward tolerance after the last rounding the output has seen (AAE_T_ACT_DH2 = h2, not rounded itself)."""
    return forward_tolerance(name, rows, H, s) * np.maximum(1.0, np.abs(c["h2"][k]))


def bf16_z(name, rows, H, s, c, k):
    """(R(h2), its tolerance) where the output is itself rounded, z = R(h2): a device h2 within the forward tolerance of the
    reference rounds to the same bf16 value - unless the reference h2 lies that close to the midpoint of two, and then to either:
    the forward tolerance, plus the distance of those two neighbours at such points alone."""
    r, other, mid = bf16_values(c["h2"][k])
    t = bf16_forward_tol(name, rows, H, s, c, k)
    return r, t + np.where(np.abs(c["h2"][k] - mid) <= t, np.abs(other - r), 0.0)


def weakened(name, rows, H, s, c):
    """The ambiguous points at which matching either continuation is a weaker check than matching one: where the two differ by
    more than the tolerances.  (GELU's tail from x = -4 down lies below 1.3e-4 with an absolute error of |x| 1.2e-7 from
    1 + erf: more than the bf16 spacing there, so 8 % of its grid is ambiguous - between neighbours 1e-6 apart.)"""
    return c["amb"] & ((np.abs(c["h2"][0] - c["h2"][1]) > bf16_forward_tol(name, rows, H, s, c, 0)) |
                       (np.abs(c["d"][0] - c["d"][1]) > bf16_ratio_tol(name, s, c, 0)))


def bf16_ratio_tol(name, s, c, k):
    return ratio_tol(name, s, c["xin"], c["u"][k], c["d"][k]) + 2 * BF16_EPS * np.abs(c["d"][k])
