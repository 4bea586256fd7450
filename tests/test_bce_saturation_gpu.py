"""The decoder's output layer ALONE on designed logits, around the point where the reference's fp32 sigmoid becomes exactly
1.0 (24 ln 2 = 16.6355: F.binary_cross_entropy(sigmoid(l) + 1e-12, .) then charges a zero target the clamped 100 and
back-propagates 0; aae.py:176-177, 693-695) - every form of the layer (single launch, critical + deferred launches,
row-blocked, three GEMMs, bf16) through HipAAE.output_layer_step, against a plain restatement of
sigmoid -> BCE(+1e-12) -> backward -> Adam in the reference's fp32 arithmetic.

The logits are exact by construction: every row of dh2 is one-hot (plus the bias column), so logit[b, n] = w[n, j(b)] +
b3[n] with no rounding in any product form (the three-term bf16 emulation of the fp32 product included), and b3 = 0 at
the first call.  w is a sweep: dense between 8 and 18 on both sides of 24 ln 2 and of 25 ln 2, the float neighbours of
+-87, +-100, +-104, 0, -0.0, +-500; targets 0, 1 and strictly inside (0, 1) at every kind of logit; empty rows; a ragged
last item tile.  Column 0 of w holds saturated logits only and is the one-hot column of rows without targets: their
dL/d(dh2) must be EXACTLY 0 and column 0 of dec.lin3.weight must not move by a bit.

No logit of the first call lies within ZONE of 24 ln 2, and Adam moves a logit by at most 2 lr per call, so none of the
second call's lies within ZONE - 2 lr of it (asserted on the restatement's logits): no cell can fall on the other side of the
cut-off for a difference in the last bits."""
import numpy as np
import pytest
import torch

from golden_util import BCE_CUT, bce_quantisation_bound

CUT25 = 25.0 * np.log(2.0)
ZONE = 4e-3          # no designed logit this close to 24 ln 2 (lr = 1e-3: the second call's stay 2e-3 away)
LR, GRAD_SCALE = 1e-3, 0.5
K_DEC_BCE_FWD, K_DEC_FUSED, K_DEC_CRIT = 1, 5, 7        # aaerec._hip kernel ids of the profile


def _neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-1e30), dtype=np.float32), x, np.nextafter(x, np.float32(1e30), dtype=np.float32)]


def sweep_values(bf16):
    """(all values, the saturated ones) as float32; bf16: rounded to bf16-representable values first."""
    from oracle.aae_oracle import bf16_round
    dense = np.arange(8.0, 18.0, 0.0125)
    near = [BCE_CUT + k * ZONE for k in (-3, -2, -1.25, 1.25, 2, 3)] + [CUT25 + k * 2e-3 for k in (-2, -1, 1, 2)]
    special = [0.0, -0.0, 500.0, -500.0, 30.0, -30.0, 1.0, -1.0, 4.0, -4.0, -12.0, -17.0]
    for x in (87.0, -87.0, 100.0, -100.0, 104.0, -104.0):
        special += _neighbours(x)
    v = np.concatenate([dense, near, special]).astype(np.float32)
    if bf16:
        v = np.unique(bf16_round(v))
    v = v[np.abs(v.astype(np.float64) - BCE_CUT) >= ZONE]
    sat = v[v.astype(np.float64) > BCE_CUT]
    assert ((sat < CUT25) & (sat > BCE_CUT)).sum() >= 4 and (v < BCE_CUT).sum() >= 20
    return v, sat


class Restatement:
    """aae_output_layer_step restated: logits = dh2 V3^T + b3; F.binary_cross_entropy(sigmoid + 1e-12, T + 1e-12) and its
    gradient as autograd forms it, in fp32 (oracle.aae_oracle.sigmoid: 1 / (1 + exp(-l)), pinned to torch's saturation by
    tests/test_oracle_golden.py); dA2 = G V3; dV3 = G^T dh2, db3 = sum_b G; torch.optim.Adam.  bf16: the matrix products'
    operands rounded to bf16 as the bf16 build defines them (tests/test_bf16_gpu.py _SliceEmu).  moments (m_w, v_w, m_b, v_b)
    and step: Adam's state as aae_load_adam sets it before the first call; optimizer 'sgd': torch.optim.SGD
    (tests/outlayer_cases.py)."""

    def __init__(self, w, b, lr, scale, bf16, moments=None, step=0, optimizer="adam"):
        from oracle.aae_oracle import SGD, Adam, bf16_round
        self.p = {"w": w.copy(), "b": b.copy()}
        self.opt, self.scale = (Adam(lr) if optimizer == "adam" else SGD(lr)), scale
        if moments is not None and optimizer == "adam":
            for k in ("w", "b"):
                self.opt.m[k], self.opt.v[k], self.opt.t[k] = moments["m_" + k].copy(), moments["v_" + k].copy(), int(step)
        self.R = bf16_round if bf16 else (lambda x: x)

    def forward(self, dh2):
        h2 = self.R(dh2[:, :-1])
        return h2, (h2 @ self.R(self.p["w"]).T + self.R(self.p["b"])).astype(np.float32)

    def step(self, dh2, T):
        from oracle.aae_oracle import TINY, f32, sigmoid
        B, N = T.shape
        h2, logits = self.forward(dh2)
        xhat = sigmoid(logits)
        x, t = xhat + TINY, T + TINY
        with np.errstate(divide="ignore"):
            lx, l1x = np.maximum(np.log(x), f32(-100)), np.maximum(np.log1p(-x), f32(-100))
        cells = -(t * lx + (f32(1) - t) * l1x)
        gx = (x - t) / np.maximum((f32(1) - x) * x, f32(1e-12)) * f32(self.scale / (B * N))
        G = (gx * xhat * (f32(1) - xhat)).astype(f32)
        Gr = self.R(G)
        da2 = (Gr @ self.R(self.p["w"])).astype(f32)
        self.opt.step(self.p, {"w": (Gr.T @ h2).astype(f32), "b": Gr.sum(0).astype(f32)})
        return float(cells.mean(dtype=np.float64)), da2, logits, G, cells


def design(N, h, B, bf16, seed):
    """(w [N, h], X csr [2 B, N] of targets, dh2 of both calls [2][B, h + 1], rows without targets on column 0 [2][...])"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    v, sat = sweep_values(bf16)
    w = rng.choice(v, size=(N, h)).astype(np.float32)
    w[:, 0] = rng.choice(sat, size=N)                       # column 0: every logit beyond the cut-off
    w[: len(v), 1] = v                                      # column 1: every value of the sweep at least once
    w[: len(sat), 0] = sat
    kinds = [(-1e9, -20.0), (-20.0, 0.0), (0.0, 10.0), (10.0, BCE_CUT), (BCE_CUT, CUT25), (CUT25, 1e9)]
    rows, cols, vals, dh2s, zero_rows = [], [], [], [], []
    for call in range(2):
        dh2 = np.zeros((B, h + 1), dtype=np.float32)
        dh2[:, h] = 1.0
        zr = []
        for b in range(B):
            if b % 5 == 2 or b == B - 1:                    # a row without targets on the saturated column
                j = 0
                zr.append(b)
            else:
                j = 1 if b % 7 == 0 else 1 + (b * 3 + call) % (h - 1)
                if b % 11 != 5:                             # (else: a row without targets on an ordinary column)
                    items = []
                    for lo, hi in kinds:                    # targets at every kind of logit: 0/1 and strictly inside
                        cand = np.flatnonzero((w[:, j] >= lo) & (w[:, j] < hi))
                        if len(cand):
                            items += list(rng.choice(cand, size=min(2, len(cand)), replace=False))
                    items += [N - 1] if b % 3 == 0 else []  # the ragged last tile's last item
                    for n in sorted(set(int(i) for i in items)):
                        rows.append(call * B + b)
                        cols.append(n)
                        vals.append([1.0, 1.0, 0.25, 0.5, 0.75][len(vals) % 5])
            dh2[b, j] = 1.0
        dh2s.append(dh2)
        zero_rows.append(np.asarray(zr))
    X = sp.csr_matrix((np.asarray(vals, dtype=np.float32), (rows, cols)), shape=(2 * B, N))
    X.sort_indices()
    return w, X, dh2s, zero_rows


def kernel_rule(logits, T, scale, cut):
    """What the kernels do with a cell, restated in fp64 (csrc/gemm_f32.h bce_elem): softplus for log(1 - x) below `cut`, the
    clamped 100 and no gradient from `cut` on.  -> (mean loss, dL/dlogits).  Used WITHOUT a GPU, to show that this file's
    comparison holds for the rule with cut = 24 ln 2 and cannot hold with 25 ln 2."""
    l = logits.astype(np.float64)
    B, N = l.shape
    s = np.where(l >= 0, 1.0 / (1.0 + np.exp(-np.abs(l))), np.exp(-np.abs(l)) / (1.0 + np.exp(-np.abs(l))))
    satd = l >= cut
    x, t = s + 1e-12, T + 1e-12                 # (the reference's TINY on both: a target far below zero has no gradient)
    l1x = np.where(satd, -100.0, -np.logaddexp(0.0, l))
    loss = -(t * np.maximum(np.log(x), -100.0) + (1.0 - t) * l1x)
    one_minus_s = np.where(l >= 0, np.exp(-np.abs(l)) / (1.0 + np.exp(-np.abs(l))), 1.0 / (1.0 + np.exp(-np.abs(l))))
    G = (x - t) / np.maximum((one_minus_s - 1e-12) * x, 1e-12) * s * one_minus_s
    G = np.where(satd, 0.0, G) * scale / (B * N)
    return float(loss.mean()), G


def test_restatement_agrees_with_torch_autograd_and_tells_the_two_cut_offs_apart():
    """Without a GPU: (1) the restatement's loss cells and dL/dlogits are torch's own (CPU autograd on the same logits) - and
    fp64's away from the quantised band; (2) the kernels' rule in fp64 with the cut-off at 24 ln 2 meets the restatement
    within this file's bounds (loss: the derived quantisation bound; gradient: 2e-4 of the largest), with 25 ln 2 it misses
    both by orders of magnitude - the GPU tests below can fail."""
    import torch.nn.functional as F
    N, h, B = 1003, 50, 37
    w, X, dh2s, zero_rows = design(N, h, B, False, 1)
    T = np.asarray(X[:B].todense(), dtype=np.float32)
    emu = Restatement(w, np.zeros(N, dtype=np.float32), LR, GRAD_SCALE, False)
    loss, da2, logits, G, cells = emu.step(dh2s[0], T)
    assert np.array_equal(logits, w[:, np.argmax(dh2s[0][:, :h], 1)].T)              # exact by construction
    x = torch.from_numpy(logits).requires_grad_(True)
    ref = F.binary_cross_entropy(torch.sigmoid(x) + 1e-12, torch.from_numpy(T) + 1e-12, reduction="none")
    (ref.mean() * GRAD_SCALE).backward()
    np.testing.assert_allclose(cells, ref.detach().numpy(), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(G, x.grad.numpy(), rtol=1e-5, atol=1e-7 * GRAD_SCALE / (B * N))
    sat0 = (logits >= BCE_CUT) & (T == 0)
    assert sat0.sum() > 500 and np.all(G[sat0] == 0) and np.all(cells[sat0] == 100.0)
    band0 = sat0 & (logits <= CUT25)
    assert band0.sum() > 100
    calm = np.abs(logits) < 8.0
    l64, g64 = kernel_rule(logits, T.astype(np.float64), GRAD_SCALE, BCE_CUT)
    np.testing.assert_allclose(G[calm], g64[calm], rtol=2e-6, atol=1e-13)
    bound = bce_quantisation_bound(logits, X[:B].indptr, X[:B].indices, X[:B].data)
    assert abs(l64 - loss) <= bound + 1e-5 * loss, (l64, loss, bound)
    assert np.abs(g64 - G).max() <= 2e-4 * np.abs(G).max()
    l25, g25 = kernel_rule(logits, T.astype(np.float64), GRAD_SCALE, CUT25)
    print(f"loss: restatement {loss:.5f}, rule at 24 ln 2 {l64:.5f}, at 25 ln 2 {l25:.5f}; bound {bound:.5f}; cells in the band {band0.sum()}")
    assert abs(l25 - loss) > 20 * (bound + 1e-5 * loss)
    assert np.abs(g25 - G).max() > 0.9 * GRAD_SCALE / (B * N)


FORMS = [  # id, N, h, B, constructor keywords, AAE_SPLIT_ANY, (kernel ids that must have run), (kernel ids that must not)
    ("single-h50", 1003, 50, 37, {}, False, (K_DEC_FUSED,), (K_DEC_CRIT, K_DEC_BCE_FWD)),
    ("single-h100", 2021, 100, 100, {}, False, (K_DEC_FUSED,), (K_DEC_CRIT, K_DEC_BCE_FWD)),
    ("single-h200", 1517, 200, 104, {}, False, (K_DEC_FUSED,), (K_DEC_CRIT, K_DEC_BCE_FWD)),
    ("split-h50", 1003, 50, 37, {}, True, (K_DEC_CRIT,), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    ("split-h100", 2021, 100, 100, {}, True, (K_DEC_CRIT,), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    ("split-h200", 1517, 200, 104, {}, True, (K_DEC_CRIT,), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    ("blocked-h100", 2021, 100, 300, dict(blocked_output=True), False, (K_DEC_CRIT,), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    ("blocked-h200", 1517, 200, 230, dict(blocked_output=True), False, (K_DEC_CRIT,), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    ("three-gemm-h50", 1003, 50, 128, {}, False, (K_DEC_BCE_FWD,), (K_DEC_FUSED, K_DEC_CRIT)),
    ("three-gemm-h200", 1517, 200, 128, {}, False, (K_DEC_BCE_FWD,), (K_DEC_FUSED, K_DEC_CRIT)),
    ("bf16-h50", 1003, 50, 37, dict(dtype="bf16"), False, (), (K_DEC_BCE_FWD,)),
    ("bf16-h100", 2021, 100, 100, dict(dtype="bf16"), False, (), (K_DEC_BCE_FWD,)),
    ("bf16-h200", 1517, 200, 104, dict(dtype="bf16"), False, (), (K_DEC_BCE_FWD,)),
    ("bf16-blocked-h200", 1517, 200, 230, dict(dtype="bf16", blocked_output=True), False, (), (K_DEC_BCE_FWD,)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_output_layer_on_designed_logits_matches_the_restatement(form, monkeypatch):
    from aaerec._hip import HipAAE, DeviceCSR
    name, N, h, B, kw, split_any, ran, not_ran = form
    bf16 = kw.get("dtype") == "bf16"
    if split_any:
        monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    w, X, dh2s, zero_rows = design(N, h, B, bf16, N + h + B)
    b3 = np.zeros(N, dtype=np.float32)
    sl = HipAAE(N, h, 10, max_batch=B, rng_mode="inject", gen_lr=LR, **kw)
    sl.load_params({"dec.lin3.weight": w, "dec.lin3.bias": b3})
    sl.set_grad_scale(GRAD_SCALE)
    sl.profile_enable()
    emu = Restatement(w, b3, LR, GRAD_SCALE, bf16)
    csr = DeviceCSR(X, sl.device)
    for s in range(2):
        Xs = X[s * B:(s + 1) * B]
        T = np.asarray(Xs.todense(), dtype=np.float32)
        sl.dh2_rows(B)[:, :h + 1].copy_(torch.from_numpy(dh2s[s]))
        sl.output_layer_step(csr, s * B, B)
        loss, da2, logits, G, _ = emu.step(dh2s[s], T)
        dist = np.abs(logits.astype(np.float64) - BCE_CUT)
        assert dist.min() >= ZONE - 2 * LR - 1e-4 * s, (s, dist.min())      # no cell of this call near the cut-off
        zero_sat = (T == 0) & (logits >= BCE_CUT)
        assert zero_sat.sum() >= B and (zero_sat & (logits <= CUT25)).sum() >= 20 and np.all(G[zero_sat] == 0)
        bound = bce_quantisation_bound(logits, Xs.indptr, Xs.indices, Xs.data)
        got_loss = sl.losses()[0]
        got = sl.da2_rows(B)[:, :h].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - da2).max())
        print(f"{name} call {s}: loss {got_loss:.6f}, restatement {loss:.6f} (derived bound {bound:.6f}); max |da2 - restatement| "
              f"{err:.3e} of {np.abs(da2).max():.3e}; zero-target cells beyond the cut-off {zero_sat.sum()}, "
              f"of them up to 25 ln 2 {(zero_sat & (logits <= CUT25)).sum()}")
        sd = sl.state_dict()
        zmax = float(np.abs(got[zero_rows[s]]).max())
        moved = float(np.abs(sd["dec.lin3.weight"][:, 0].astype(np.float64) - w[:, 0]).max())
        werr = float(np.abs(sd["dec.lin3.weight"].astype(np.float64) - emu.p["w"]).max())
        berr = float(np.abs(sd["dec.lin3.bias"].astype(np.float64) - emu.p["b"]).max())
        # (every check of the call is evaluated before the first one fails the test: the message names all that miss)
        checks = {
            f"loss {got_loss} against {loss} within {bound} + 1e-5 relative": abs(got_loss - loss) <= bound + 1e-5 * abs(loss),
            f"dL/d(dh2) of the rows whose every cell is saturated is exactly 0 (largest {zmax:.3e})": zmax == 0.0,
            f"dL/d(dh2) within 2e-4 of its largest ({err:.3e} of {float(np.abs(da2).max()):.3e})":
                err <= 2e-4 * float(np.abs(da2).max()) + 1e-12,
            f"column 0 of dec.lin3.weight has not moved by a bit (moved {moved:.3e})":
                np.array_equal(sd["dec.lin3.weight"][:, 0], w[:, 0]),
            f"dec.lin3.weight within 1e-5 ({werr:.3e})": werr <= 1e-5,
            f"dec.lin3.bias within 1e-5 ({berr:.3e})": berr <= 1e-5,
        }
        assert all(checks.values()), (name, "call", s, [k for k, ok in checks.items() if not ok])
    torch.cuda.synchronize()
    counts = {k: sl.profile_read(k)[1] for k in set(ran) | set(not_ran)}
    assert all(counts[k] > 0 for k in ran) and all(counts[k] == 0 for k in not_ran), (name, counts)
