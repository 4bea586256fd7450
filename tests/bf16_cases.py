"""The cases of the bf16 fuzz (tests/test_bf16_fuzz_cpu.py, tests/test_bf16_fuzz_gpu.py) and the twin of the rounded oracle that
shows, without a device, how much of each tolerance the reference itself uses.

A case is a configuration of tests/fuzz_cases.py (the fp32 fuzz's generator and step loop, the same implementation) run as
HipAAE(.., dtype='bf16'), possibly on a forced path, against OracleAAE(.., bf16=True): three steps, the last one shorter, the
cut at the output layer and predict where the configuration draws them.  The tolerances are those of tests/test_bf16_gpu.py.

The twin (TwinAAE / TwinDecoder) rounds the same operands at the same points and differs from the oracle the way a device may:
every dense product it shares with the oracle accumulates in float64 (another summation order, at its limit), and every hidden
activation's output is moved by 4 units in the last place, up or down by a hash of its argument (act_sweep.Intrinsics: the
error bound of the device's erff / tanhf / log1pf / expm1f, as a function of x alone).  tests/test_bf16_fuzz_cpu.py asserts for
every case below that oracle and twin disagree by at most a QUARTER of each cap: three quarters are the device's."""
import numpy as np

import act_sweep as A
import fuzz_cases as F

f32 = np.float32

# ---- the groups ----------------------------------------------------------------------------------------------------------------
PATH_CYCLE = ["default", "kslices", "chain16", "no_chain", "x16", "split_any", "blocked_any"]
# regular: 28 consecutive seeds of F.config, the path cycling over them (four seeds each).  The first seed is the smallest from
# 100 on (the fp32 fuzz holds 0 .. 27 and 500 .. 527; it is 443) whose 28 configurations give every path a dropout case and an SGD case
# and BLOCKED_ANY a batch above 112 rows (test_bf16_fuzz_cpu.py asserts what the lists hold).
REGULAR_FIRST = 443
REGULAR = [(REGULAR_FIRST + i, PATH_CYCLE[i % len(PATH_CYCLE)]) for i in range(28)]
# tiny: F.config(seed, tiny=True) - one hidden unit, two items, one document - on the default path and layer by layer
TINY = [(100 + i, ["default", "no_chain"][i % 2]) for i in range(12)]
# r6: each of the fourteen further classes on the default path (chain_kernel<true, true>) and layer by layer (kGemmBf16's
# epilogues), every (class, path) with a configuration of its own
R6 = [(600 + 2 * k + j, name, path) for k, name in enumerate(F.ACTS_R6) for j, path in enumerate(["default", "no_chain"])]
# wide conditions: F.WIDE, whole step and cut form, predict.  The seed of a case names its batches and its initial parameters
WIDE_SEED = {case: 7000 + case for case in range(len(F.WIDE))}
WIDE = [(case, cut) for case in range(len(F.WIDE)) for cut in (False, True)]
# decoder-only: aae_decoder_step against OracleDecoder(bf16=True); seeds of F.decoder_config
DECODER = [100 + 2 * i for i in range(8)]

# Seeds replaced because oracle and twin alone disagree by more than a quarter of a cap: (group, case) -> (seed generated, its
# replacement, the reason).  One of 92.
# WIDE[1] (SELU under AlphaDropout, 200 hidden units, 120 items, 100 documents, a 198-column condition) is the one shape of the
# lists where the pair disagrees like this whatever the seed: the share of enc.lin1.weight beyond 2e-4, as a fraction of the 1 %
# allowed, over the seeds 7001, 7009, .. (steps of 8 keep a case's seeds apart from the other cases'): 0.283 0.495 0.327 0.313 0.452
# 0.308 0.659 0.560 0.250 0.188 (losses at 0.226 of theirs) 1.322 0.716 0.168.  7065 sits on the quarter exactly (60 of 240
# elements), which another BLAS' summation order can tip; 7097 is the next with room to spare.  Seed 7081 shows the reference
# alone BEYOND the whole cap: at this shape the 1 % share is not a bound that separates a wrong kernel from a right one, and a
# device failure here on another seed would not by itself be a finding.
REPLACED = {("wide", 1): (7001, 7097, "enc.lin1.weight: 68 elements beyond 2e-4 between oracle and twin, a quarter of the allowed 240 is 60")}
WIDE_SEED[1] = REPLACED[("wide", 1)][1]

# SGD cases keep the fp32 fuzz's bound, close_enough(.., F.SGD_TOL = 5e-5, 3 max(lr)).  Measured over the SGD cases of the lists:
# leaving out a quarter of the elements close_enough sets aside, oracle and twin differ by at most 9.7e-6 (r6 ReLU6 layer by layer;
# next 6.9e-6, regular 469) - under a quarter of 5e-5, so the bound stays.
SGD_PAIR_MAX = 9.7e-6

# Bounds tests/test_bf16_gpu.py has no counterpart for, each 4 x what oracle and twin alone differ by over the eight decoder-only cases:
#   dL/d(input) of aae_decoder_step on the FIRST step (both sides hold the same parameters; from the second on Adam's sign flips
#   of near-zero gradients - up to ~lr per step, the cap on the parameters - move these entries, sums of ~1e-5 with cancellation,
#   by per cents): measured 1.39e-3 of max |dz| (seed 114; 1.13e-3 seed 112; 2e-7 without a rounding boundary crossed)
DZ_PAIR_MAX = 1.4e-3
DZ_TOL = 4 * DZ_PAIR_MAX
#   decode() with the trained weights: measured 5.0e-4 (seed 112; 3.3e-4 seed 104), taken as 5.5e-4 for another BLAS.  The step
#   cases' predict keeps 5e-3 / 10: there the pair differs by at most 0.36 of it (WIDE[4]; 0.33 - 0.49 over five seeds of that shape,
#   so no seed brings it under a quarter, and the device keeps the other 64 %), by under 0.01 of it in the other cases
DECODE_PAIR_MAX = 5.5e-4
DECODE_TOL = 4 * DECODE_PAIR_MAX
PREDICT_TOL = 5e-4


def regular_config(seed):
    return F.config(seed)


def tiny_config(seed):
    return F.config(seed, tiny=True)


def r6_config(seed, name):
    cfg, r = F.config(seed)
    cfg["act"] = name
    return cfg, r


def all_step_cases():
    """(group, id, cfg factory, seed for init_params, path) of every case that runs whole steps"""
    out = []
    for seed, path in REGULAR:
        out.append(("regular", f"{seed}-{path}", lambda seed=seed: regular_config(seed), seed, path))
    for seed, path in TINY:
        out.append(("tiny", f"{seed}-{path}", lambda seed=seed: tiny_config(seed), seed, path))
    for seed, name, path in R6:
        out.append(("r6", f"{name}-{path}", lambda seed=seed, name=name: r6_config(seed, name), seed, path))
    for case, cut in WIDE:
        out.append(("wide", f"{case}-{'cut' if cut else 'step'}", lambda case=case, cut=cut: F.wide_config(case, cut, WIDE_SEED[case]), WIDE_SEED[case], "default"))
    return out


# ---- the twin ------------------------------------------------------------------------------------------------------------------
TWIN_ULPS = 4.0
# Where a class evaluates a library function (erff, tanhf, log1pf, expm1f, __expf): everywhere, or on its curved side alone.
# The other classes - ReLU, LeakyReLU, Hardtanh, ReLU6, Softsign, Hardsigmoid, the two shrinks, Identity, Hardswish - are a
# comparison and at most two correctly rounded operations, the same on the device and in the oracle: nothing to move.
CURVED = {"SELU": "neg", "ELU": "neg", "CELU": "neg", "Tanh": "all", "Sigmoid": "all", "Softplus": "all", "LogSigmoid": "all",
          "GELU": "all", "SiLU": "all", "Mish": "all"}


class _Twin:
    """OracleAAE._mlp_fwd / _mlp_bwd with the same roundings, float64 accumulation and moved activations."""
    model = A.Intrinsics(0)

    def _R(self, x):
        from oracle.aae_oracle import bf16_round
        if not self.bf16:                            # (the fp32 fuzz's twin, tests/fuzz_path_cases.py: no rounding, the float64 cast alone)
            return np.asarray(x).astype(np.float64)
        return bf16_round(x).astype(np.float64)      # (the same bf16 value; a product of two of these accumulates in float64)

    def _act(self, u):
        from oracle.aae_oracle import act_fwd
        y = act_fwd(self.act, u)
        where = CURVED.get(self.act)
        if where is None:
            return y
        m = self.model.move(y, u, TWIN_ULPS, 5)
        if self.act in ("Tanh", "Sigmoid"):          # (never beyond +-1, and exactly +-1 where the function rounds to it)
            m = np.where(np.abs(y) == 1, y, np.clip(m, f32(-1), f32(1))).astype(f32)
        return m if where == "all" else np.where(u > 0, y, m).astype(f32)

    def _mlp_fwd(self, net, x0, masks, first_pre=None):
        from oracle.aae_oracle import Drop
        P, f64 = self.p, np.float64
        k1, k2 = masks if masks is not None else (None, None)
        d1, d2 = Drop(self.dropout[0], k1, self.alpha_mode), Drop(self.dropout[1], k2, self.alpha_mode)
        a1 = first_pre if first_pre is not None else self._linear(x0, P[net + ".lin1.weight"], P[net + ".lin1.bias"])
        u1 = d1.fwd(a1)
        h1 = self._act(u1)
        a2 = self._linear(h1, P[net + ".lin2.weight"], P[net + ".lin2.bias"])
        u2 = d2.fwd(a2)
        h2 = self._act(u2)
        if net == "disc":
            a3 = (h2.astype(f64) @ P[net + ".lin3.weight"].astype(f64).T + P[net + ".lin3.bias"]).astype(f32)
        else:
            a3 = self._linear(h2, P[net + ".lin3.weight"], P[net + ".lin3.bias"])
        return a3, dict(x0=x0, d1=d1, d2=d2, u1=u1, h1=h1, u2=u2, h2=h2)

    def _mlp_bwd(self, net, g3, cache, need_dx=True):
        from oracle.aae_oracle import act_bwd
        P, R, f64 = self.p, self._R, np.float64
        if net == "dec":
            G = {net + ".lin3.weight": (R(g3).T @ R(cache["h2"])).astype(f32), net + ".lin3.bias": R(g3).sum(0).astype(f32)}
        else:
            G = {net + ".lin3.weight": (g3.astype(f64).T @ cache["h2"].astype(f64)).astype(f32), net + ".lin3.bias": g3.astype(f64).sum(0).astype(f32)}
        gh2 = (g3.astype(f64) @ P[net + ".lin3.weight"].astype(f64)).astype(f32) if net == "disc" else (R(g3) @ R(P[net + ".lin3.weight"])).astype(f32)
        ga2 = cache["d2"].bwd(act_bwd(self.act, cache["u2"], cache["h2"], gh2))
        G[net + ".lin2.weight"] = (ga2.astype(f64).T @ cache["h1"].astype(f64)).astype(f32)
        G[net + ".lin2.bias"] = ga2.astype(f64).sum(0).astype(f32)
        gh1 = (R(ga2) @ R(P[net + ".lin2.weight"])).astype(f32)
        ga1 = cache["d1"].bwd(act_bwd(self.act, cache["u1"], cache["h1"], gh1))
        G[net + ".lin1.bias"] = ga1.astype(f64).sum(0).astype(f32)
        gx = (R(ga1) @ R(P[net + ".lin1.weight"])).astype(f32) if need_dx else None
        return G, ga1, gx


def make_pair(params, salt, decoder=False, bf16=True, **kw):
    """(the rounded oracle, its twin) on copies of the same parameters; bf16=False: the fp32 oracle and its twin"""
    from oracle import aae_oracle as O
    base = O.OracleDecoder if decoder else O.OracleAAE
    twin_cls = type("Twin" + base.__name__, (_Twin, base), {})
    ora, twin = base(params, bf16=bf16, **kw), twin_cls(params, bf16=bf16, **kw)
    twin.model = A.Intrinsics(salt)
    return ora, twin


def run_pair(cfg, r, seed, bf16=True):
    """A step case through oracle and twin: per-step losses of both, the two models, and predict of both where asked."""
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    inc = cfg["inc"]
    kw, p, lr = F.model_kwargs(cfg)
    params = init_params(cfg["N"], cfg["h"], cfg["c"], cond_inc=inc, seed=seed)
    ora, twin = make_pair(params, seed, bf16=bf16, conditions=[O.ConcatConst(inc)] if inc else [], **kw)
    twin.conditions = [O.ConcatConst(inc)] if inc else []
    la, lb = [], []
    for st in F.steps(cfg, r):
        args = (st["ip"], st["idx"], st["val"], st["zr"], st["masks"], [st["cond"]] if inc else None)
        la.append(ora.partial_fit(*args))
        lb.append(twin.partial_fit(*args))
    pred = None
    if cfg.get("predict") and st["pick"] is None:
        args = (st["ip"], st["idx"], st["val"], [st["cond"]] if inc else None)
        pred = (ora.predict(*args), twin.predict(*args))
    return np.asarray(la), np.asarray(lb), ora, twin, pred


def run_decoder_pair(seed, bf16=True):
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    r, N, h, B, act = F.decoder_config(seed)
    it = F.decoder_steps(r, N, h, B, seed)
    c, p = next(it)
    params = init_params(N, h, c, seed=seed)
    ora, twin = make_pair(params, seed, decoder=True, bf16=bf16, lr=2e-3, dropout=p, activation=act, conditions=[O.ConcatConst(c)])
    twin.conditions = [O.ConcatConst(c)]
    la, lb, dz = [], [], []
    for s in range(3):
        ip, idx, val, zin, masks = next(it)
        la.append(ora.partial_fit([zin], ip, idx, val, masks))
        lb.append(twin.partial_fit([zin], ip, idx, val, masks))
        dz.append((ora.last_dzin, twin.last_dzin))
    zp = next(it)
    return np.asarray(la), np.asarray(lb), ora, twin, dz, (ora.predict([zp]), twin.predict([zp])), dict(N=N, h=h, c=c, B=B, act=act, drop=bool(p[0]))
