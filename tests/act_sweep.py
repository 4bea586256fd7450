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
