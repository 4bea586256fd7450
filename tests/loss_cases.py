"""Shared by tests/test_eval_loss_cpu.py and tests/test_eval_loss_gpu.py: the shapes and target sets of the held-out loss
(csrc/loss_eval.h), the oracles' LOGITS, and the host restatement of a row's loss that the device is held to.

Shapes - the smallest at which the kernels can go wrong: N = 1007 items (a ragged last tile of 32), 130 rows (two 128-row
blocks of the rank kernel, the second with 2 rows), hidden widths 24 and 200 (two NB families of the rank kernel), n_code 8,
no condition or a constant block of 12 columns.  A target set holds an empty row, a row of 90 entries (more than one chunk of
64 of loss_targets_kernel), fractional values in (0, 1), and differs from the inputs.

row_bce restates the two cell functions (csrc/rank_x3.h loss_cell_t0 / loss_cell_target) in float64:
  a cell without a target entry    softplus(l); 100 from the fp32 logit >= 24 ln 2 on (there fl(sigmoid) = 1 and the reference's
                                   log1p(-1) = -inf is clamped to -100)
  a target entry of value v        -(t log x + (1 - t) log(1 - s)), x = s + 1e-12, t = v + 1e-12, s = sigmoid(l), log x clamped
                                   at -100, and log(1 - s) = -softplus(l) below the cut-off, -100 from it on
tiny = 0 gives the VAE's reference, nn.BCELoss without the 1e-12 (vae.py:133-136); the kernels charge a VAE handle's target
cells with the 1e-12 form as its training step does - the two differ by < 1e-9 per cell while sigmoid(l) > 1e-3."""
import numpy as np

N, ROWS, CODE, MAX_BATCH = 1007, 130, 8, 64
EMPTY_ROW, LONG_ROW, LONG_LEN = 3, 5, 90
TINY = 1e-12
ZONE = 4e-3                         # tests/test_bce_saturation_gpu.py: no oracle logit this close to the cut-off
TOL_LOSS = 2e-6                     # tests/test_oracle_golden.py: "fp32 summation order only"
CUT32 = np.float32(16.635532)       # csrc/device_common.h kBceSatLogit = fl(24 ln 2)
BCE_CUT = 24.0 * np.log(2.0)
SAT_ITEMS_HI, SAT_ITEMS_LO = np.arange(40, 50), np.arange(500, 510)      # the saturated case: bias + 30 / - 30


def corpus(seed, rows=ROWS, n_items=N, max_len=30):
    r = np.random.default_rng(500 + seed)
    docs = [np.sort(r.choice(n_items, size=int(r.integers(1, max_len)), replace=False)) for _ in range(rows)]
    ip = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return ip, np.concatenate(docs).astype(np.int32), np.ones(int(ip[-1]), dtype=np.float32), docs


def targets(seed, docs, n_items=N, saturated=False):
    """(indptr, indices, values) of a target CSR over the rows of `docs`: most of a row's input items and a few held-out ones,
    half of the values fractional in (0, 1); row EMPTY_ROW without entries, row LONG_ROW with LONG_LEN.  saturated: every
    non-empty row also names one item of SAT_ITEMS_HI and one of SAT_ITEMS_LO (saturated cells ON non-zero targets)."""
    r = np.random.default_rng(900 + seed)
    rows, vals = [], []
    for b, d in enumerate(docs):
        if b == EMPTY_ROW:
            t = np.zeros(0, dtype=np.int64)
        elif b == LONG_ROW:
            t = r.choice(n_items, size=LONG_LEN, replace=False)
        else:
            keep = d[r.random(len(d)) < 0.7]
            free = np.setdiff1d(np.arange(n_items), d)
            t = np.concatenate([keep, r.choice(free, size=3, replace=False)])
        if saturated and b != EMPTY_ROW:
            t = np.union1d(t, [r.choice(SAT_ITEMS_HI), r.choice(SAT_ITEMS_LO)])
        t = np.unique(t)
        v = np.where(r.random(len(t)) < 0.5, 1.0, r.uniform(0.05, 0.95, len(t))).astype(np.float32)
        rows.append(t)
        vals.append(v)
    ip = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.float32)


def aae_params(h, inc, seed, saturated=False, spread=8.0):
    """tools.synth.init_params with the output layer spread (tests/test_rank_gpu.py::_rank_case); saturated: the bias of ten
    items at + 30 and of ten at - 30."""
    from tools.synth import init_params
    p = init_params(N, h, CODE, cond_inc=inc, seed=seed)
    p["dec.lin3.weight"] = (p["dec.lin3.weight"] * np.float32(spread)).astype(np.float32)
    if saturated:
        p["dec.lin3.bias"] = p["dec.lin3.bias"].copy()
        p["dec.lin3.bias"][SAT_ITEMS_HI] = 30.0
        p["dec.lin3.bias"][SAT_ITEMS_LO] = -30.0
    return p


def vae_params(h, inc, seed, spread=8.0):
    r = np.random.default_rng(seed)

    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return r.uniform(-b, b, (o, i)).astype(np.float32), r.uniform(-b, b, o).astype(np.float32)
    p = {}
    for name, (o, i) in (("fc1", (h, N)), ("fc21", (CODE, h)), ("fc22", (CODE, h)), ("fc3", (h, CODE + inc)), ("fc4", (N, h))):
        p[name + ".weight"], p[name + ".bias"] = lin(o, i)
    p["fc4.weight"] *= np.float32(spread)
    return p


def vae_to_hip(p):
    return {"enc.lin1.weight": p["fc1.weight"], "enc.lin1.bias": p["fc1.bias"],
            "enc.lin3.weight": np.vstack([p["fc21.weight"], p["fc22.weight"]]),
            "enc.lin3.bias": np.concatenate([p["fc21.bias"], p["fc22.bias"]]),
            "dec.lin1.weight": p["fc3.weight"], "dec.lin1.bias": p["fc3.bias"],
            "dec.lin3.weight": p["fc4.weight"], "dec.lin3.bias": p["fc4.bias"]}


# ---- the oracles' logits (oracle.aae_oracle; eval mode) ---------------------------------------------------------------
def aae_logits(ora, ip, idx, val, cond=None):
    z, _ = ora.encode(ip, idx, val, None)
    for c, inp in zip(ora.conditions, [cond] if cond is not None else []):
        z = c.fwd(z, inp, train=False)
    return ora._mlp_fwd("dec", z, None)[0]


def decoder_logits(ora, zin):
    return ora._mlp_fwd("dec", np.asarray(zin, dtype=np.float32), None)[0]


def vae_logits(ora, ip, idx, val, eps, cond=None):
    """(logits, mu, logvar) of OracleVAE.forward in eval mode."""
    from oracle.aae_oracle import _lin
    _, c = ora.forward(ip, idx, val, eps, [cond] if cond is not None else None, train=False)
    return _lin(c["h3"], ora.p["fc4.weight"], ora.p["fc4.bias"]), c["mu"], c["lv"]


# ---- the restatement -----------------------------------------------------------------------------------------------
def row_bce(logits, indptr, indices, values, tiny=TINY):
    """float64 [rows]: per row the sum over the items of the cell loss (module docstring)."""
    L32 = np.asarray(logits, dtype=np.float32)
    L = L32.astype(np.float64)
    sat = L32 >= CUT32
    softplus = np.maximum(L, 0.0) + np.log1p(np.exp(-np.abs(L)))
    cell = np.where(sat, 100.0, softplus)
    rows = np.repeat(np.arange(L.shape[0]), np.diff(indptr))
    l = L[rows, indices]
    t = np.asarray(values, dtype=np.float64) + tiny
    x = 1.0 / (1.0 + np.exp(-l)) + tiny
    with np.errstate(divide="ignore"):
        lx = np.maximum(np.log(x), -100.0)
    l1x = np.where(sat[rows, indices], -100.0, -softplus[rows, indices])
    cell[rows, indices] = -(t * lx + (1.0 - t) * l1x)
    return cell.sum(1)


def row_kl(mu, logvar):
    """float64 [rows]: -0.5 sum_c (1 + logvar - mu^2 - exp(logvar))."""
    mu, lv = np.asarray(mu, dtype=np.float64), np.asarray(logvar, dtype=np.float64)
    return -0.5 * (1.0 + lv - mu ** 2 - np.exp(lv)).sum(1)


def row_bound(logits, indptr, indices, values):
    """The per-row form of golden_util.bce_quantisation_bound: that function on a one-row slice, times N."""
    from golden_util import bce_quantisation_bound
    L = np.asarray(logits)
    out = np.empty(L.shape[0])
    for b in range(L.shape[0]):
        lo, hi = indptr[b], indptr[b + 1]
        out[b] = bce_quantisation_bound(L[b:b + 1], np.array([0, hi - lo]), indices[lo:hi], values[lo:hi]) * L.shape[1]
    return out


def zone_clear(logits):
    """The condition every case states on its oracle's logits: none within ZONE of 24 ln 2."""
    return float(np.abs(np.asarray(logits, dtype=np.float64) - BCE_CUT).min()) > ZONE


def dense_targets(indptr, indices, values, n_items=N):
    T = np.zeros((len(indptr) - 1, n_items), dtype=np.float32)
    T[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = values
    return T


# ---- the cases: (name, hidden width, condition columns, seed, saturated) - the seeds are ones for which the ORACLE's logits
# keep clear of the cut-off (checked on the CPU, tests/test_eval_loss_cpu.py) -----------------------------------------
AAE_CASES = [("h24", 24, 0, 1, False), ("h200-cond12", 200, 12, 2, False), ("h200-saturated", 200, 0, 3, True)]
VAE_CASES = [("h24", 24, 0, 11), ("h200-cond12", 200, 12, 12)]


class AaeCase:
    """Parameters, input rows, target rows, the condition block, the oracle and its logits of one AAE case; device(): a handle
    with the same parameters and the two CSRs in HBM."""

    def __init__(self, name, h, inc, seed, saturated, bf16=False):
        from oracle import aae_oracle as O
        self.name, self.h, self.inc, self.bf16 = name, h, inc, bf16
        self.params = aae_params(h, inc, seed, saturated)
        self.ip, self.idx, self.val, self.docs = corpus(seed)
        self.tip, self.tidx, self.tval = targets(seed, self.docs, saturated=saturated)
        r = np.random.default_rng(70 + seed)
        self.cond = (r.standard_normal((ROWS, inc)) * 0.4).astype(np.float32) if inc else None
        self.kw = dict(dropout=(0.0, 0.0), gen_lr=1e-3, reg_lr=1e-3)
        self.ora = O.OracleAAE(self.params, conditions=[O.ConcatConst(inc)] if inc else None, bf16=bf16, **self.kw)
        self.logits = aae_logits(self.ora, self.ip, self.idx, self.val, self.cond)

    def device(self, **kw):
        import torch
        from aaerec._hip import HipAAE, DeviceCSR
        dev = HipAAE(N, self.h, CODE, cond_inc=self.inc, max_batch=MAX_BATCH, max_nnz=MAX_BATCH * N, rng_mode="inject",
                     **({"dtype": "bf16"} if self.bf16 else {}), **self.kw, **kw)
        dev.load_params(self.params)
        self.csr = DeviceCSR.from_arrays(self.ip, self.idx, self.val, N, dev.device)
        self.tcsr = DeviceCSR.from_arrays(self.tip, self.tidx, self.tval, N, dev.device)
        self.cond_t = torch.as_tensor(self.cond, device=dev.device) if self.inc else None
        return dev


class VaeCase:
    def __init__(self, name, h, inc, seed):
        from oracle import aae_oracle as O
        self.name, self.h, self.inc = name, h, inc
        self.params = vae_params(h, inc, seed)
        self.ip, self.idx, self.val, self.docs = corpus(seed)
        self.tip, self.tidx, self.tval = targets(seed, self.docs)
        r = np.random.default_rng(70 + seed)
        self.eps = r.standard_normal((ROWS, CODE)).astype(np.float32)
        self.cond = (r.standard_normal((ROWS, inc)) * 0.4).astype(np.float32) if inc else None
        self.ora = O.OracleVAE(self.params, lr=1e-3, conditions=[O.ConcatConst(inc)] if inc else None)
        self.logits, self.mu, self.lv = vae_logits(self.ora, self.ip, self.idx, self.val, self.eps, self.cond)

    def device(self, rng_mode="inject", **kw):
        import torch
        from aaerec._hip import HipAAE, DeviceCSR
        dev = HipAAE(N, self.h, CODE, cond_inc=self.inc, max_batch=MAX_BATCH, max_nnz=MAX_BATCH * N, rng_mode=rng_mode, seed=7,
                     dropout=(0.0, 0.0), gen_lr=1e-3, reg_lr=1e-3, vae=True, **kw)
        dev.load_params(vae_to_hip(self.params))
        self.csr = DeviceCSR.from_arrays(self.ip, self.idx, self.val, N, dev.device)
        self.tcsr = DeviceCSR.from_arrays(self.tip, self.tidx, self.tval, N, dev.device)
        self.eps_t = torch.as_tensor(self.eps, device=dev.device)
        self.cond_t = torch.as_tensor(self.cond, device=dev.device) if self.inc else None
        return dev


def reference_test_loss(bce_rows, kl_rows, n_items, batch_size):
    """vae.py:243-263: sum over the batches of batch_size rows of (mean BCE of the batch + its KL), over the rows."""
    total = 0.0
    for s in range(0, len(bce_rows), batch_size):
        b = bce_rows[s:s + batch_size]
        total += b.sum() / (len(b) * n_items) + kl_rows[s:s + batch_size].sum()
    return total / len(bce_rows)
