"""Groundwork for the Tanhshrink and PReLU activation classes (tests/act_more.py), without a GPU: the float32 emulations of
Tanhshrink's output-only derivative and of PReLU's branch bit and y / a recovery against float64 over the whole domain, with the
bounds derived from them; the dense PyTorch restatement against the four fixtures of the real reference, and its bf16 switch
against the rounded oracle; and, for the cases of the bf16 fuzz, how much of each tolerance the restatement and its twin use
between themselves."""
import numpy as np
import pytest

import act_more as M
import act_sweep as A
import fuzz_cases as F
from golden_util import Fixture

f32 = np.float32


def test_emulated_inverse_keeps_its_bound_over_the_whole_domain():
    """tanh(x)^2 recovered from y = x - tanhf(x) in float32 NumPy (Newton steps inside a bracket on |y|), against float64: |x| from
    1e-30 to 1e4, a dense grid on [-8, 8], +-0 and the activation sweeps, for every model of tanhf's error in act_sweep.MODELS
    (correctly rounded, and twelve sign patterns of 4 units in the last place).  act_more.TS_EPS is at least 1.5 x the maximum
    and not loose by more than 2 x; two Newton steps fewer or more stay inside the maximum's room as well (four reach the
    neighbourhood the residual's own rounding allows: the error is the forward difference's, not the iteration's)."""
    x = M.whole_domain()
    want = np.tanh(x.astype(np.float64)) ** 2
    worst, worst_plain = 0.0, 0.0
    for k, model in enumerate(A.MODELS):
        y = M.ts_fwd32(x, model)
        got = M.ts_grad_from_y32(y, model)
        assert got.dtype == f32 and np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
        err = np.abs(got - want)
        i = int(err.argmax())
        print(f"Tanhshrink model {k}: worst {err[i]:.3e} at x = {x[i]!r} (got {got[i]!r}, want {want[i]!r})")
        worst = max(worst, float(err[i]))
        if model is None:
            worst_plain = float(err[i])
        for steps in (M.TS_STEPS - 2, M.TS_STEPS + 2):
            assert np.abs(M.ts_grad_from_y32(y, model, steps=steps) - want).max() <= M.TS_EPS / 1.5, (k, steps)
    print(f"Tanhshrink: worst over the models {worst:.3e} (correctly rounded tanhf alone {worst_plain:.3e}); bound {M.TS_EPS:.1e}")
    assert 1.5 * worst <= M.TS_EPS <= 3.0 * worst, (worst, M.TS_EPS)
    # the function is odd, its derivative even; and the bound is a real check: LeakyReLU's derivative (what the kernels that
    # carry six classes return for any other id) or Tanh's 1 - y^2 is off by a hundred times more on 99 % of 0.05 < |x| < 3
    y = M.ts_fwd32(x)
    assert np.array_equal(M.ts_grad_from_y32(y), M.ts_grad_from_y32(-y))
    mid = (np.abs(x) > 0.05) & (np.abs(x) < 3)
    assert (np.abs(np.where(y > 0, 1.0, 0.01) - want)[mid] > 100 * M.TS_EPS).mean() > 0.99
    assert (np.abs(1.0 - y.astype(np.float64) ** 2 - want)[mid] > 100 * M.TS_EPS).mean() > 0.99


def test_port_reproduces_the_reference_fixture():
    """The dense PyTorch restatement with the real nn.Tanhshrink against tests/golden/step_act_tanhshrink.npz, a run of the real
    reference (tools/gen_golden.py acts_more; the case shape of the other step_act_* fixtures), at test_oracle_golden.py's
    tolerances: losses 2e-6 relative, parameters 5e-6, reconstructions 2e-6."""
    import scipy.sparse as sp
    fx = Fixture(M.FIXTURE)
    assert fx.cfg["activation"] == M.NAME and tuple(fx.cfg["dropout"]) == (0.2, 0.2)
    kw = fx.model_kwargs()
    assert kw.pop("activation") == M.NAME
    m = M.Port(fx.init_params(), **kw)
    checked = 0
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"])).toarray()
        losses = m.partial_fit(X, z_real=fx.z[f"step{s}.z_real"], masks=fx.masks(s))
        np.testing.assert_allclose(losses, fx.z[f"step{s}.losses"], rtol=2e-6, atol=1e-7)
        if fx.has_state(s):
            got = m.state_dict()
            for k, w in fx.expected_params(s).items():
                np.testing.assert_allclose(got[k], w, atol=5e-6, rtol=0, err_msg=f"step {s} {k}")
                checked += 1
    assert checked == 18
    ip, idx, val = fx.batch(0, "predict")
    X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"])).toarray()
    np.testing.assert_allclose(m.predict(X), fx.z["predict.out"], atol=2e-6)


def test_bf16_port_rounds_where_the_oracle_rounds():
    """The port's bf16 switch on a class the oracle carries too: Port(activation='Tanh', bf16=True) against OracleAAE(bf16=True),
    three steps with dropout, a condition block and a shorter last batch - the same operands rounded at the same points give the
    same steps (losses 2e-6 relative, parameters 5e-6; a rounding put elsewhere moves them by 1e-3 relative)."""
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    N, B, h, c, inc = 120, 17, 23, 10, 5
    cfg = dict(N=N, h=h, c=c, B=B, inc=inc, act="Tanh", prior="gauss", opt="adam", drop=True, norm=True, scale=0.0, cut=False,
               long_rows=False, window=False)
    kw, p, lr = F.model_kwargs(cfg)
    params = init_params(N, h, c, cond_inc=inc, seed=3)
    ora = O.OracleAAE(params, conditions=[O.ConcatConst(inc)], bf16=True, **kw)
    kw.pop("activation")
    port = M.Port(params, activation="Tanh", bf16=True, **kw)
    import scipy.sparse as sp
    for st in F.steps(cfg, np.random.default_rng(3)):
        want = ora.partial_fit(st["ip"], st["idx"], st["val"], st["zr"], st["masks"], [st["cond"]])
        X = sp.csr_matrix((st["val"], st["idx"], st["ip"]), shape=(st["Bs"], N)).toarray().astype(f32)
        got = port.partial_fit(X, z_real=st["zr"], masks=st["masks"], cond=st["cond"])
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7)
    got = port.state_dict()
    for k, w in ora.p.items():
        F.close_enough(got[k], w, 5e-6, 3 * max(lr), k)


@pytest.mark.parametrize("a", M.PRELU_A)
def test_emulated_prelu_recovery_keeps_its_bound(a):
    """The stored output x or a x with the branch !(x > 0) in its last bit, and what the backward pass takes from it alone: the
    slope (1 or a, exact - at x = 0 it is a, as in ATen) and x = y / a for the weight's gradient.  Over the whole domain: the
    unmarked output is within a unit in the last place of the real module's, the recovered x within PRELU_REL |x| + 2^-126 / |a|
    (the product's flush), PRELU_REL at least 1.5 x the worst relative error; a == 0 recovers 0 everywhere, as decided."""
    import torch
    x = M.whole_domain()
    ym = M.prelu_fwd32(x, a)
    with torch.no_grad():
        want_y = torch.nn.functional.prelu(torch.from_numpy(x), torch.tensor([a], dtype=torch.float32)).numpy()
    y = (ym.view(np.uint32) & np.uint32(0xFFFFFFFE)).view(f32)
    assert (np.abs(y.astype(np.float64) - want_y) <= np.abs(np.spacing(want_y))).all()
    slope, xr = M.prelu_bwd32(ym, a)
    neg = ~(x > 0)
    assert np.array_equal(slope, np.where(neg, f32(a), f32(1))) and (xr[~neg] == 0).all()
    if a == 0:
        assert (xr == 0).all() and (y[neg] == 0).all()
        return
    x64, a64 = x.astype(np.float64), float(f32(a))
    err = np.abs(xr - x64)[neg]
    assert (err <= M.PRELU_REL * np.abs(x64[neg]) + M.PRELU_FLUSH / abs(a64)).all()
    normal = neg & (np.abs(a64 * x64) >= M.PRELU_FLUSH)
    worst = float((np.abs(xr - x64)[normal] / np.abs(x64[normal])).max())
    print(f"PReLU a = {a:g}: worst relative error of y / a {worst:.3e} (bound {M.PRELU_REL:.1e})")
    assert 1.5 * worst <= M.PRELU_REL <= 3.0 * 1.84e-7


def _prelu_port(fx):
    kw = fx.model_kwargs()
    assert kw.pop("activation") == "PReLU"
    return M.Port(fx.init_params(), activation="PReLU", **kw)


@pytest.mark.parametrize("name", ["step_act_prelu", "step_act_prelu_sgd"])
def test_port_reproduces_the_prelu_fixtures(name):
    """The restatement with the real nn.PReLU's forward on six per-module weights against the runs of the real reference (Adam,
    and SGD at lr 0.05 / 0.02): losses at 2e-6, every parameter - the six weights among them - at 5e-6, and the weights' Adam
    moments in all four optimisers (enc.act* in enc_optim and in gen_optim) at test_parity_abi_gpu.py's tolerances."""
    import scipy.sparse as sp
    fx = Fixture(name)
    m = _prelu_port(fx)
    acts = [f"{n}.act{i}.weight" for n in ("enc", "dec", "disc") for i in (1, 2)]
    assert all(fx.init_params()[k].shape == (1,) and fx.init_params()[k][0] == 0.25 for k in acts)
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"])).toarray()
        losses = m.partial_fit(X, z_real=fx.z[f"step{s}.z_real"], masks=fx.masks(s))
        np.testing.assert_allclose(losses, fx.z[f"step{s}.losses"], rtol=2e-6, atol=1e-7)
    s = fx.steps - 1
    got = m.state_dict()
    for k, w in dict(fx.expected_params(s), **{k: fx.z[f"step{s}.{k}"] for k in acts}).items():
        np.testing.assert_allclose(got[k], w, atol=5e-6, rtol=0, err_msg=f"{name} {k}")
    assert all(fx.z[f"step{s}.{k}"][0] != 0.25 for k in acts)          # (they are trained)
    if fx.cfg.get("optimizer", "adam") == "adam":
        order = fx.cfg["param_order"]
        for tag, net, opt in (("A_enc", "enc", m.opt_enc), ("A_dec", "dec", m.opt_dec), ("A_gen", "enc", m.opt_gen), ("A_disc", "disc", m.opt_disc)):
            for i, k in enumerate(order[net]):
                st = opt.state[m.p[f"{net}.{k}"]]
                np.testing.assert_allclose(st["exp_avg"].numpy(), fx.z[f"step{s}.{tag}.{i}.m"], atol=2e-9, rtol=1e-4, err_msg=f"{tag} m {k}")
                np.testing.assert_allclose(st["exp_avg_sq"].numpy(), fx.z[f"step{s}.{tag}.{i}.v"], atol=1e-12, rtol=2e-4, err_msg=f"{tag} v {k}")
                assert float(st["step"]) == float(fx.z[f"step{s}.{tag}.{i}.t"])


def test_vae_port_reproduces_the_prelu_fixture_and_its_weight_never_moves():
    """The VAE builds its one shared activation after its optimiser (vae.py:94-96): the reference's own run leaves act.weight at
    0.25 to the bit after every step, and the restatement - whose optimiser owns the five Linears alone - matches its losses and
    parameters at test_oracle_golden.py's VAE tolerances (5e-6)."""
    import scipy.sparse as sp
    fx = Fixture("step_vae_prelu")
    assert fx.cfg["activation"] == "PReLU"
    names = ("fc1", "fc21", "fc22", "fc3", "fc4")
    m = M.PortVAE({f"{n}.{t}": fx.z[f"init.{n}.{t}"] for n in names for t in ("weight", "bias")}, lr=fx.cfg["gen_lr"], activation="PReLU")
    for s in range(fx.steps):
        assert fx.z[f"step{s}.act.weight"].view(np.uint32) == fx.z["init.act.weight"].view(np.uint32) == f32(0.25).view(np.uint32)
        ip, idx, val = fx.batch(s)
        X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"])).toarray()
        loss = m.partial_fit(X, fx.z[f"step{s}.eps"])
        np.testing.assert_allclose(loss, fx.z[f"step{s}.losses"][0], rtol=5e-6)
        for n in names:
            for t in ("weight", "bias"):
                np.testing.assert_allclose(m.p[f"{n}.{t}"].detach().numpy(), fx.z[f"step{s}.{n}.{t}"], atol=5e-6, rtol=0, err_msg=f"step {s} {n}.{t}")
    assert float(m.act.weight.detach()) == 0.25
    ip, idx, val = fx.batch(0, "predict")
    X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"])).toarray()
    np.testing.assert_allclose(m.predict(X, fx.z["predict.eps"]), fx.z["predict.out"], atol=2e-6)


def test_port_refuses_selu():
    from oracle.dense_torch_port import init_params
    with pytest.raises(ValueError, match="AlphaDropout"):
        M.Port(init_params(20, 4, 2), activation="SELU")


# ---- the bf16 fuzz's cases: what the reference side alone uses of each tolerance -----------------------------------------------
@pytest.mark.parametrize("activation", ["Tanhshrink", "PReLU"])
@pytest.mark.parametrize("case", M.aae_cases(), ids=M.case_id)
def test_port_and_twin_use_at_most_a_quarter_of_each_bf16_tolerance(case, activation):
    """As tests/test_bf16_fuzz_cpu.py does for the oracle: the bf16 port and its twin (float64 accumulation, Tanhshrink's outputs
    moved by 4 units in the last place) disagree by at most a QUARTER of each cap of tests/test_bf16_gpu.py - losses 2e-4
    relative + 2e-6, per tensor the share of elements beyond 1e-4 max(1, lr / 1e-3) and the largest difference - on the seed
    chosen for the case (act_more.BF16_SEED has the replaced ones and why).  Three quarters are the device's."""
    seed = M.bf16_seed(activation, case)
    la, pa = M.run_port(case, seed, bf16=True, activation=activation)
    lb, pb = M.run_port(case, seed, bf16=True, twin=True, activation=activation)
    assert np.isfinite(la).all() and np.isfinite(lb).all()
    loss_use = float((np.abs(la - lb) / (2e-4 * np.abs(la) + 2e-6)).max())
    stats = F.bf16_param_stats(pb, pa, 2e-3, 3)
    share_use = max(frac / allowed for frac, allowed, mx, bound in stats.values())
    max_use = max(mx / bound for frac, allowed, mx, bound in stats.values())
    print(f"BF16PAIR {activation} {M.case_id(case)} seed {seed}: losses {loss_use:.3f}, share {share_use:.3f}, maximum {max_use:.3f} of the caps")
    assert loss_use <= 0.25 and share_use <= 0.25 and max_use <= 0.25, (loss_use, share_use, max_use)
