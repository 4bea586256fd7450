"""Groundwork for the Tanhshrink and PReLU activation classes, which the library does not carry yet (HipAAE raises for both
names).  Float32 NumPy emulations of what the backward pass would need - it keeps a layer's output alone (csrc/device_common.h):
an output-only derivative for Tanhshrink, the branch bit and the recovery x = y / a for PReLU - each with the error bound
derived from it; a dense PyTorch restatement of the training step with the real torch.nn module (per-module trainable weights
for PReLU, the roundings of bf16 mode on request, a twin that differs the way a device may); and the cases of a fuzz against
that restatement.  tests/test_act_more_cpu.py holds the emulations to float64 and the restatement to the runs of the real
reference in tests/golden/ (step_act_tanhshrink, step_act_prelu, step_act_prelu_sgd, step_vae_prelu).  Plain NumPy / torch on the
CPU: nothing here touches the library, and tests/act_sweep.py is imported as it stands."""
import numpy as np
import torch
import torch.nn.functional as TF

import act_sweep as A
import fuzz_cases as F
from oracle.dense_torch_port import DenseTorchAAE

f32 = np.float32
NAME = "Tanhshrink"
FIXTURE = "step_act_tanhshrink"

# ---- an output-only derivative, emulated in float32 ----------------------------------------------------------------------------
# y = x - tanh(x) is odd and strictly increasing: the stored output needs no branch bit (as GELU / SiLU / Mish / Hardswish do,
# device_common.h nm_mark) and keeps all its bits; but f' = tanh(x)^2 is no closed form in y, so the backward pass has to invert
# f.  On |y| (f is odd, f' even): Newton steps inside a bracket, from c = cbrt(3 |y|) in [0.999 c, 1.5 c] below |y| = 1
# (y = x^3 / 3 - 2 x^5 / 15 .., x / c grows from 1 to 1.36 at y = 1) and from |y| + 1 in [|y|, |y| + 1] beyond (0 < tanh < 1).
# f is convex on x > 0, so the steps fall monotonically from the first overshoot on: four reach the neighbourhood the residual's
# own rounding allows, six are run.
# Near 0 the forward difference x - tanhf(x) and the residual both cancel: eta, the error of tanhf at x (units in the last
# place of x), stands against a y of x^3 / 3.  That moves the recovered x by eta / x^2 and tanh(x)^2 by 2 eta / x - a CONSTANT in
# x, since eta is proportional to x - and where eta exceeds y altogether (|x| < 1e-3) the bracket keeps the result below
# 2.25 c^2 = 2.25 (3 eta)^(2/3).  So the bound needs no near / c terms as act_sweep.eps_nm has them.
# The ALGORITHM in float32, as act_sweep.nm_grad_from_y32 is for the four non-monotone classes: with model = None tanhf is
# NumPy's, an act_sweep.Intrinsics model moves each result by tanhf's error bound (LIB_ULPS = 4 units in the last place), up or
# down by a hash of the argument.
TS_STEPS = 6
# The bound on the absolute error of f'(x) over the whole domain: 1.5 x the emulation's maximum over act_sweep.MODELS (2.28e-6;
# 2.6e-7 with a correctly rounded tanhf), the margin the r6 classes got for the device's own tanhf.
TS_EPS = 3.5e-6


def _tanh32(x, model):
    return A._lib32(np.tanh, x, model, 4, saturates=True)


def ts_fwd32(x, model=None):
    """The forward pass: x - tanhf(x), ATen's form, cancellation near 0 included."""
    x = np.asarray(x, dtype=f32)
    return (x - _tanh32(x, model)).astype(f32)


def ts_grad_from_y32(y, model=None, steps=TS_STEPS):
    """tanh(x)^2 from the stored output alone."""
    ay = np.abs(np.asarray(y, dtype=f32))
    with np.errstate(all="ignore"):
        c = np.cbrt(f32(3) * ay).astype(f32)
        small = ay < 1
        lo = np.where(small, f32(0.999) * c, ay).astype(f32)
        hi = np.where(small, f32(1.5) * c, ay + f32(1)).astype(f32)
        x = np.where(small, c, hi).astype(f32)
        for _ in range(steps):
            t = _tanh32(x, model)
            r = ((x - t) - ay).astype(f32)
            neg = r < 0
            lo, hi = np.where(neg, x, lo), np.where(neg, hi, x)
            xn = (x - r / (t * t)).astype(f32)
            x = np.where((xn >= lo) & (xn <= hi), xn, f32(0.5) * (lo + hi)).astype(f32)      # (also the NaN of t == 0)
        t = _tanh32(x, model)
        out = (t * t).astype(f32)
    return np.where(ay > 0, out, f32(0)).astype(f32)


def whole_domain():
    """|x| from 1e-30 to 1e4 log-spaced, a dense grid on [-8, 8], +-0 and the sweeps of tests/act_sweep.py."""
    mag = np.logspace(-30, 4, 40000)
    parts = [mag, -mag, np.linspace(-8.0, 8.0, 200001), [0.0, -0.0]] + [A.sweep(NAME, r, w).ravel() for r, w in A.SHAPES]
    return np.concatenate(parts).astype(f32)


# ---- PReLU: what the stored output has to carry, emulated in float32 ------------------------------------------------------------
# y = x > 0 ? x : a x with one trainable scalar a per module (0.25 at first).  a can turn negative in training, and then y > 0 on
# both branches: the branch !(x > 0) has to ride in the stored output's lowest mantissa bit (as nm_mark's does).  The backward
# pass needs dx = x > 0 ? g : a g - exact, from the bit alone - and da = sum over the branch of g x, for which x = y / a is
# recovered.  The quotient's relative error: the product a x is rounded (2^-24), the bit costs up to a unit in the last place
# (2^-23), the division rounds again (2^-24): 2^-22 = 2.4e-7 at most; PRELU_REL is 1.5 x the emulation's maximum (1.83e-7: the
# three roundings seldom line up), and it holds down to where a x leaves the normal range: below |a x| = 2^-126 the product
# is flushed (or denormal) and the term g x of that cell is lost, |x| < 2^-126 / |a| of it - 1.2e-18 at |a| = 1e-20.
# a == 0 is decided explicitly: y = +-0 on the whole branch, nothing can be recovered, x is taken as 0 and the weight's gradient
# of that step is 0 where the reference's is sum g x - a departure from the reference - while the forward pass and dx are exact
# and equal ReLU's.
PRELU_A = [0.25, 1.0, -0.5, 1e-3, -1e-3, 1e-20, 0.0]
PRELU_REL = 2.8e-7
PRELU_FLUSH = 2.0 ** -126


def prelu_fwd32(x, a):
    """The stored output: x or a x in float32, the branch !(x > 0) in its last bit."""
    x, a = np.asarray(x, dtype=f32), f32(a)
    with np.errstate(under="ignore"):
        y = np.where(x > 0, x, a * x).astype(f32)
    return ((y.view(np.uint32) & np.uint32(0xFFFFFFFE)) | (~(x > 0)).astype(np.uint32)).view(f32)


def prelu_bwd32(ym, a):
    """(slope dy/dx, the recovered x on the branch that feeds da - 0 elsewhere) from the stored output alone."""
    ym, a = np.ascontiguousarray(ym, dtype=f32), f32(a)
    neg = (ym.view(np.uint32) & np.uint32(1)) != 0
    y = (ym.view(np.uint32) & np.uint32(0xFFFFFFFE)).view(f32)
    with np.errstate(all="ignore"):
        x = np.where(neg & (a != 0), y / a, f32(0)).astype(f32)
    return np.where(neg, a, f32(1)).astype(f32), x


# ---- the dense PyTorch restatement ---------------------------------------------------------------------------------------------
# oracle/dense_torch_port.py's DenseTorchAAE (the reference's own dense formulation: three nets, the injected masks and z_real,
# four torch.optim optimisers) with the real torch.nn module as the activation.  bf16 = True rounds both operands of every product
# the kernels round in bf16 mode (csrc/chain.h's BF description; OracleAAE._linear / _mlp_bwd are the model): a Linear layer's
# forward product, bias included, and its dX product - all three products of the decoder's output layer - but not the first
# encoder layer, not the discriminator's one-unit output layer, not the hidden layers' weight gradients.
# twin = True is the port as a device may differ from it (tests/bf16_cases.py's _Twin): the same roundings, every product it
# shares with the port accumulated in float64, every activation output moved by 4 units in the last place, up or down by a hash
# of its argument.
def _R(t):
    return t.to(torch.bfloat16).to(torch.float32)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, mode, wide):
        """mode 0: fp32 on every product; 1: forward and dX on rounded operands; 2: the weight gradient too (dec.lin3)"""
        ctx.save_for_backward(x, W)
        ctx.mode, ctx.wide = mode, wide
        acc = torch.float64 if wide else torch.float32
        rx, rW, rb = (_R(x), _R(W), _R(b)) if mode else (x, W, b)
        return (rx.to(acc) @ rW.to(acc).t() + rb.to(acc)).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        acc = torch.float64 if ctx.wide else torch.float32
        rg = _R(g) if ctx.mode else g
        dx = (rg.to(acc) @ (_R(W) if ctx.mode else W).to(acc)).to(torch.float32)
        gw, xw = (rg, _R(x)) if ctx.mode == 2 else (g, x)
        dW = (gw.to(acc).t() @ xw.to(acc)).to(torch.float32)
        return dx, dW, gw.to(acc).sum(0).to(torch.float32), None, None


class Port(DenseTorchAAE):
    def __init__(self, params, activation=NAME, bf16=False, twin=False, salt=0, **kw):
        if activation == "SELU":
            raise ValueError("SELU takes AlphaDropout: use DenseTorchAAE itself")
        # (the base class builds the optimisers over every tensor of `params` by its net: with PReLU these hold the six weights
        #  enc.act1.weight .. disc.act2.weight of shape [1] - enc.act* in enc_optim and gen_optim, as enc.parameters() is in the
        #  reference)
        super().__init__(params, activation="ReLU", **kw)
        self.module = getattr(torch.nn, activation)()
        self.per_module = any(True for _ in self.module.parameters())
        assert not self.per_module or all(f"{n}.act{i}.weight" in self.p for n in ("enc", "dec", "disc") for i in (1, 2))
        self.bf16, self.twin = bool(bf16), bool(twin)
        self.model = A.Intrinsics(salt)

    def _act(self, net, i, u):
        if self.per_module:      # the real module's forward on this instance's weight
            y = torch.func.functional_call(self.module, {"weight": self.p[f"{net}.act{i}.weight"]}, (u,))
        else:
            y = self.module(u)
        if not self.twin or self.per_module:      # (PReLU calls no library function: nothing to move, as bf16_cases.CURVED has it)
            return y
        moved = self.model.move(y.detach().numpy(), u.detach().numpy(), 4.0, 5)
        return y * torch.from_numpy(moved / np.where(y.detach().numpy() == 0, f32(1), y.detach().numpy())).to(torch.float32)

    def _lin(self, net, i, x):
        W, b = self.p[f"{net}.lin{i}.weight"], self.p[f"{net}.lin{i}.bias"]
        plain = not self.bf16 or (net == "enc" and i == 1) or (net == "disc" and i == 3)
        if plain and not self.twin:
            return TF.linear(x, W, b)
        return _Linear.apply(x, W, b, 0 if plain else 2 if (net == "dec" and i == 3) else 1, self.twin)

    def _stack(self, net, x, train, keeps):
        k1, k2 = keeps if keeps is not None else (None, None)
        x = self._act(net, 1, self._drop(self._lin(net, 1, x), self.dropout[0], train, k1))
        x = self._act(net, 2, self._drop(self._lin(net, 2, x), self.dropout[1], train, k2))
        return self._lin(net, 3, x)


class PortVAE:
    """The reference's VAE step (OracleVAE is the model): L1-normalise -> fc1 -> act -> (fc21, fc22) -> z = mu + eps exp(logvar / 2)
    -> [condition] -> fc3 -> act -> fc4 -> sigmoid; mean BCE + KL sum; one Adam over the five Linears.  ONE shared activation
    module, built after the optimiser (vae.py:94-96): a weight of it (PReLU's) is in no optimiser and never moves."""

    def __init__(self, params, lr=2e-3, activation=NAME):
        self.p = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=True) for k, v in params.items()}
        self.act = getattr(torch.nn, activation)()
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)

    def forward(self, X, eps, cond):
        P = self.p
        h1 = self.act(TF.linear(TF.normalize(X, 1), P["fc1.weight"], P["fc1.bias"]))
        mu, lv = TF.linear(h1, P["fc21.weight"], P["fc21.bias"]), TF.linear(h1, P["fc22.weight"], P["fc22.bias"])
        z = torch.as_tensor(eps, dtype=torch.float32) * torch.exp(0.5 * lv) + mu
        if cond is not None:
            z = torch.cat([z, torch.as_tensor(cond, dtype=torch.float32)], 1)
        h3 = self.act(TF.linear(z, P["fc3.weight"], P["fc3.bias"]))
        return torch.sigmoid(TF.linear(h3, P["fc4.weight"], P["fc4.bias"])), mu, lv

    def partial_fit(self, X_dense, eps, cond=None):
        X = torch.FloatTensor(X_dense)
        xh, mu, lv = self.forward(X, eps, cond)
        loss = TF.binary_cross_entropy(xh, X) + -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp())
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.item() / X.shape[0]

    def predict(self, X_dense, eps, cond=None):
        with torch.no_grad():
            return self.forward(torch.FloatTensor(X_dense), eps, cond)[0].numpy()


# ---- the cases of the fuzz -----------------------------------------------------------------------------------------------------
# 120 items; every (rows, n_hidden) pair - a 16-row block is the general chain kernel's unit, 207 the widest hidden layer a slot
# holds - with n_code and dropout cycling so that each meets every rows and every n_hidden; then a decoder input of 209 columns
# (code + condition + bias: the narrowest two-part input), and the sibling models.  A case's seed names its initial parameters
# and its batches.
N_ITEMS = 120
ROWS, HIDDEN, CODES = [1, 15, 16, 17, 33], [1, 7, 61, 207], [1, 10]
# (rows, n_hidden, inc) -> the seed of the bf16 case where it is not the fp32 case's: the port and its twin alone (test_act_more_cpu.py)
# disagree on the losses by 0.474 of the cap at seed 110 and by 0.436 at 115; seeds + 100, + 200 .. in turn gave 0.043 at 210, and
# 0.340, 0.202, 0.001 at 215, 315, 415
# PReLU at 33 rows x 207 hidden units under dropout is bimodal in the seed: losses at 0.346 0.592 2.686 0.491 1.431 0.582 2.252 0.000
# 0.001 0.001 3.081 3.930 1.182 of their cap over 119, 219 .. 1319 - the pair alone is BEYOND the cap on five of thirteen, so at this
# shape a device failure on another seed would not by itself be a finding (as bf16_cases.REPLACED says of its WIDE[1]); 819 is taken
BF16_SEED = {("Tanhshrink", 16, 61, 0): 210, ("Tanhshrink", 17, 207, 0): 415, ("PReLU", 33, 207, 0): 819}


def bf16_seed(activation, c):
    return BF16_SEED.get((activation, c["B"], c["h"], c["inc"]), c["seed"])


def aae_cases():
    out = []
    for i, B in enumerate(ROWS):
        for j, h in enumerate(HIDDEN):
            out.append(dict(N=N_ITEMS, B=B, h=h, c=CODES[(i + j) % 2], inc=0, drop=bool((i + j // 2) % 2), seed=100 + 4 * i + j))
    out.append(dict(N=N_ITEMS, B=17, h=61, c=10, inc=198, drop=True, seed=130))          # 10 + 198 + 1 = 209 columns
    return out


def case_id(c):
    return f"B{c['B']}-h{c['h']}-c{c['c']}-inc{c['inc']}-{'drop' if c['drop'] else 'nodrop'}"


def case_cfg(c):
    """the case as a configuration of fuzz_cases.steps / model_kwargs"""
    return dict(N=c["N"], h=c["h"], c=c["c"], B=c["B"], inc=c["inc"], act=NAME, prior="gauss", opt="adam", drop=c["drop"], norm=True,
                scale=0.0, cut=False, long_rows=False, window=False)


def case_steps(c, seed):
    """Three batches, the last one shorter by a third of the rows (17 -> 12 and 33 -> 22 lose a 16-row block, 16 -> 11): per step the
    keys of fuzz_cases.steps - the batch (documents of 0 .. 11 items, empty ones included from three rows on), the twelve dropout
    keep-masks, the prior's draw, the condition block - every array with exactly `Bs` rows (asserted: the device is told Bs)."""
    N, h, B, inc = c["N"], c["h"], c["B"], c["inc"]
    r = np.random.default_rng(40000 + seed)
    p = (0.2, 0.3)
    out = []
    for s in range(3):
        Bs = B if s < 2 else max(1, B - max(1, B // 3)) if B > 1 else 1
        ip, idx, val = F.batch(r, N, Bs, B)
        masks = [(r.random((Bs, h)) > p[j % 2]).astype(np.uint8) for j in range(12)] if c["drop"] else None
        zr = r.standard_normal((Bs, c["c"])).astype(f32)
        cond = (r.standard_normal((Bs, inc)) * 0.4).astype(f32) if inc else None
        assert len(ip) == Bs + 1 and zr.shape[0] == Bs and (masks is None or all(m.shape == (Bs, h) for m in masks))
        assert cond is None or cond.shape == (Bs, inc)
        out.append(dict(s=s, Bs=Bs, corpus=(ip, idx, val), pick=None, ip=ip, idx=idx, val=val, masks=masks, zr=zr, cond=cond))
    return out


HIDDEN_SCALE = 3.0


def case_params(N, h, c, inc, seed, activation=NAME):
    """nn.Linear's default initialisation with the two hidden layers of every net 3 times larger: Tanhshrink maps a pre-activation
    of 0.1 - what the default gives behind L1-normalised rows - to 3e-4 with a derivative of 1e-2, and a step at that scale
    would hardly notice a wrong activation; with these the hidden pre-activations reach +-1.5 (6 times larger, and the bf16
    port and its twin disagree on the losses by up to 10 times the cap at 207 hidden units)."""
    from oracle.dense_torch_port import init_params
    p = init_params(N, h, c, cond_inc=inc, seed=seed)
    for k in p:
        if ".lin1." in k or ".lin2." in k:
            p[k] = (p[k] * f32(HIDDEN_SCALE)).astype(f32)
    if activation == "PReLU":          # nn.PReLU's initial weight, one per module
        for n in ("enc", "dec", "disc"):
            p[n + ".act1.weight"], p[n + ".act2.weight"] = np.full(1, 0.25, dtype=f32), np.full(1, 0.25, dtype=f32)
    return p


def dense(st, N):
    import scipy.sparse as sp
    return sp.csr_matrix((st["val"], st["idx"], st["ip"]), shape=(len(st["ip"]) - 1, N)).toarray().astype(f32)


def run_port(c, seed, bf16=False, twin=False, activation=NAME):
    """The AAE case through the port: (losses per step, parameters after them)."""
    cfg = case_cfg(c)
    kw, p, lr = F.model_kwargs(cfg)
    kw.pop("activation")
    m = Port(case_params(c["N"], c["h"], c["c"], c["inc"], seed, activation), activation=activation, bf16=bf16, twin=twin, salt=seed, **kw)
    losses = [m.partial_fit(dense(st, c["N"]), z_real=st["zr"], masks=st["masks"], cond=st["cond"]) for st in case_steps(c, seed)]
    return np.asarray(losses), m.state_dict()

