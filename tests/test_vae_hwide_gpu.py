"""A VAE wider than one chain slot on the device (cfg.vae_wide; csrc/vae_layers.h and the per-layer route of every aae_vae_*
entry point, csrc/abi_output_layer.h): n_hidden up to 1024, n_code up to 512.

Tolerances are the project's own, unchanged: the reference fixtures at test_vae_wide_gpu.py's (loss rtol 2e-5, parameters 1e-5,
Adam m 2e-8 / 2e-4, v 1e-12 / 2e-4, predict 1e-5, the embedding table 1e-5); the boundary sweep at test_fuzz_gpu.py's VAE rule
(losses rtol 5e-5, parameters close_enough(.., 5e-5, 6e-3)) and 1e-5 for aae_vae_predict - but for the case at the bound, whose
predict tolerance is 4 x the ceiling stated for the float32 oracle's own distance from the float64 oracle (vae_hwide_cases.py:
4 x 1.5e-5 over a measured 1.28e-5; the device measured 8.0e-6 from the float32 oracle there); the
rank calls at test_rank_gpu.py's 2e-6 against the host ranker over aae_vae_predict's own scores; the held-out loss at
test_eval_loss_gpu.py's."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import device_rng as R
import loss_cases as LC
import vae_hwide_cases as H
from golden_util import Fixture
from vae_wide_cases import corpus, to_hip, vae_params

pytestmark = pytest.mark.gpu

TOL_PARAM, TOL_RECON = 1e-5, 1e-5
NAMES = ("fc1", "fc21", "fc22", "fc3", "fc4")


@contextlib.contextmanager
def _no_chain():
    """Handles created inside run their hidden layers one launch per layer (option NO_CHAIN)."""
    from aaerec import _hip
    _hip.set_option("NO_CHAIN", "1")
    try:
        yield
    finally:
        _hip.set_option("NO_CHAIN", None)


def _handle(N, h, c, inc, B, wide=True, no_chain=False, **kw):
    from aaerec._hip import HipAAE
    kw = dict(dict(rng_mode="inject", gen_lr=H.LR, reg_lr=H.LR, dropout=(0.0, 0.0)), **kw)
    with (_no_chain() if no_chain else contextlib.nullcontext()):
        return HipAAE(N, h, c, cond_inc=inc, max_batch=B, vae=True, **({"vae_wide": True} if wide else {}), **kw)


def _csr(dev, ip, idx, val, N):
    from aaerec._hip import DeviceCSR
    return DeviceCSR.from_arrays(ip, idx, val, N, dev.device)


def _t(dev, a):
    return None if a is None else torch.as_tensor(a, device=dev.device)


def _launches(dev):
    from aaerec._hip import K_CHAIN, K_VAE_REPARAM
    return dev.profile_read(K_CHAIN)[1], dev.profile_read(K_VAE_REPARAM)[1]


def _fx_params(fx, prefix):
    return to_hip({f"{n}.{t}": fx.z[f"{prefix}.{n}.{t}"] for n in NAMES for t in ("weight", "bias")})


# ---- 5. reference parity, ABI level --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.HWIDE_FIXTURES)
def test_hwide_vae_step_matches_reference(name):
    """aae_vae_step / aae_vae_predict on the reference's recorded steps at (209, 105) and, behind ConditionList([30-column
    constant block, CategoricalCondition(8, sum, SparseAdam)]), at (300, 40): every step's loss (and the table, trained by
    aae_cat_update from AAE_T_ACT_DZC's columns), after the last step every parameter and the Adam moments of fc3 and fc21,
    then a predict.  The handle must have run the per-layer route: two reparametrisation launches a step, no chain launch.
    (The fixtures' initial parameters are the reference's nn.Linear initialisation rounded to multiples of 2^-12, so that a
    file stays below 1 MiB: every step is the reference's own from there - tools/gen_golden.py gen_vae.)"""
    from aaerec import _hip
    fx = Fixture(name)
    c = fx.cfg
    cat = "cat" in c
    W, dim = (c["concat"], c["cat"]["dim"]) if cat else (0, 0)
    m = _handle(c["N"], c["h"], c["c"], c["cond_inc"], c["B"], gen_lr=c["gen_lr"], reg_lr=c["gen_lr"])
    m.load_params(_fx_params(fx, "init"))
    m.profile_enable(True, kernels=(_hip.K_CHAIN, _hip.K_VAE_REPARAM))
    if cat:
        table = torch.as_tensor(fx.z["init.cond.embedding"], device=m.device).contiguous()
        t_m, t_v = torch.zeros_like(table), torch.zeros_like(table)

    def block(prefix):
        if not cat:
            return None, None
        idx = torch.as_tensor(fx.z[prefix + ".cond1"].astype(np.int32), device=m.device).contiguous()
        b = torch.empty(idx.shape[0], W + dim, dtype=torch.float32, device=m.device)
        b[:, :W] = torch.as_tensor(fx.z[prefix + ".cond0"], device=m.device)
        _hip.cat_encode(table, idx, b[:, W:])
        return b, idx
    for s in range(fx.steps):
        csr = _csr(m, *fx.batch(s), c["N"])
        B = csr.shape[0]
        cond, idx = block(f"step{s}")
        m.vae_step(csr, 0, B, cond=cond, eps=fx.z[f"step{s}.eps"])
        if cat:
            _hip.cat_update(table, t_m, t_v, idx, m.cond_grad(B)[:, W:W + dim], c["cat"]["lr"], s + 1)
            np.testing.assert_allclose(table.cpu().numpy(), fx.z[f"step{s}.cond.embedding"], atol=1e-5, err_msg=f"{name} table {s}")
        l = m.losses()
        print(f"{name} step {s}: loss {(l[0] + l[1]) / B:.8f} reference {float(fx.z[f'step{s}.losses'][0]):.8f}")
        np.testing.assert_allclose((l[0] + l[1]) / B, fx.z[f"step{s}.losses"][0], rtol=2e-5)
    assert _launches(m) == (0, 2 * fx.steps)
    s = fx.steps - 1
    got, want = m.state_dict(), _fx_params(fx, f"step{s}")
    for k, w in want.items():
        print(f"   {k}: max |diff| {float(np.abs(got[k] - w).max()):.3g}")
        np.testing.assert_allclose(got[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} {k}")
    enc, dec = m.adam_state("enc"), m.adam_state("dec")
    half = c["c"]
    for st, key, n, rows in ((enc, "lin3", "fc21", slice(0, half)), (dec, "lin1", "fc3", slice(None))):
        for t in ("weight", "bias"):
            gm, gv = st[f"{key}.{t}"]
            np.testing.assert_allclose(gm[rows], fx.z[f"step{s}.A.{n}.{t}.m"], atol=2e-8, rtol=2e-4, err_msg=f"{name} m {n}.{t}")
            np.testing.assert_allclose(gv[rows], fx.z[f"step{s}.A.{n}.{t}.v"], atol=1e-12, rtol=2e-4, err_msg=f"{name} v {n}.{t}")
        assert st["step"] == float(fx.z[f"step{s}.A.{n}.weight.t"])
    pcsr = _csr(m, *fx.batch(0, prefix="predict"), c["N"])
    out = m.vae_predict(pcsr, 0, pcsr.shape[0], cond=block("predict")[0], eps=fx.z["predict.eps"]).cpu().numpy()
    print(f"{name} predict: max |diff| {float(np.abs(out - fx.z['predict.out']).max()):.3g}")
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)


# ---- 6. reference parity, Python level -----------------------------------------------------------------------------------
def _const_block(C, width):
    class ConstConcat(C.ConcatenationBasedConditioning):
        constant_concat = True

        def size_increment(self):
            return width

        def encode(self, inputs):
            return torch.as_tensor(np.asarray(inputs), dtype=torch.float32, device="cuda")
    return ConstConcat()


def test_hwide_vae_tracks_reference():
    """aaerec.vae.VAE(n_hidden=300, n_code=40) with the fixture's ConditionList - a constant block, then a CategoricalCondition
    whose table lives on the GPU - through partial_fit / predict with the recorded eps."""
    from aaerec.vae import VAE
    from aaerec import condition as C
    fx = Fixture("step_vae_hwide_cond")
    cfg, kind = fx.cfg, fx.cfg["cat"]
    cat = C.CategoricalCondition(kind["dim"], sparse=kind["sparse"], use_cuda=True, reduce=kind["reduce"], lr=kind["lr"])
    V = fx.z["init.cond.embedding"].shape[0]
    cat.vocab = {"a%d" % i: i for i in range(1, V)}               # indices are given pre-transformed
    cat.embedding = torch.nn.Embedding(V, kind["dim"], padding_idx=0, sparse=kind["sparse"]).cuda()
    with torch.no_grad():
        cat.embedding.weight.copy_(torch.from_numpy(fx.z["init.cond.embedding"]))
    cat.optimizer = torch.optim.SparseAdam(cat.embedding.parameters(), lr=kind["lr"])
    conds = C.ConditionList([("title", _const_block(C, cfg["concat"])), ("authors", cat)])

    def cin(prefix):       # the fixture stores the batch-padded index lists: strip the padding again
        return [fx.z[prefix + ".cond0"], [[int(j) for j in row if j != 0] or [0] for row in fx.z[prefix + ".cond1"]]]
    m = VAE(cfg["N"], cfg["N"], n_hidden=cfg["h"], n_code=cfg["c"], lr=cfg["gen_lr"], batch_size=cfg["B"], conditions=conds,
            verbose=True, rng_mode="reference")
    assert m.hip.cfg.vae_wide == 1 and m._cond_native and m.hip.cond_inc == cfg["cond_inc"]
    m.hip.load_params(_fx_params(fx, "init"))
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        X = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, cfg["N"]))
        eps = fx.z[f"step{s}.eps"]
        m._eps = lambda B, eps=eps: torch.from_numpy(eps)
        m.partial_fit(X, condition_data=cin(f"step{s}"))
        np.testing.assert_allclose(cat.embedding.weight.detach().cpu().numpy(), fx.z[f"step{s}.cond.embedding"], atol=1e-5,
                                   err_msg=f"step {s} embedding")
        np.testing.assert_allclose(m.last_loss, fx.z[f"step{s}.losses"][0], rtol=2e-5)
    sd = m.state_dict()
    for n in NAMES:
        for t in ("weight", "bias"):
            np.testing.assert_allclose(sd[f"{n}.{t}"].numpy(), fx.z[f"step{fx.steps - 1}.{n}.{t}"], atol=1e-5, rtol=0, err_msg=f"{n}.{t}")
    ip, idx, val = fx.batch(0, prefix="predict")
    Xp = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, cfg["N"]))
    m._eps = lambda B: torch.from_numpy(fx.z["predict.eps"])
    np.testing.assert_allclose(m.predict(Xp, condition_data=cin("predict")), fx.z["predict.out"], atol=1e-5)


# ---- 7. boundary sweep against OracleVAE ---------------------------------------------------------------------------------
def _run_steps(dev, N, steps):
    losses = []
    for Bs, ip, idx, val, eps, cond in steps:
        dev.vae_step(_csr(dev, ip, idx, val, N), 0, Bs, cond=_t(dev, cond), eps=eps)
        l = dev.losses()
        losses.append((float(l[0]), float(l[1]), (l[0] + l[1]) / Bs))
    return losses


def _predict(dev, N, pred):
    Bs, ip, idx, val, eps, cond = pred
    return dev.vae_predict(_csr(dev, ip, idx, val, N), 0, Bs, cond=_t(dev, cond), eps=eps).cpu().numpy()


def _against_oracle(dev, case, p, steps, pred, tag):
    h, c, inc, B, act, opt, N, _ = case
    ora = H.sweep_oracle(p, inc, act, opt)
    want_l, want_p = H.run_oracle(ora, steps, pred)
    got_l = _run_steps(dev, N, steps)
    for s, (g, w) in enumerate(zip(got_l, want_l)):
        np.testing.assert_allclose(g[2], w, rtol=5e-5, err_msg=f"{tag} step {s}")
    got = dev.state_dict()
    for k, w in to_hip({k: ora.p[k] for k in p}).items():
        off, allowed, worst = H.close_enough_counts(got[k], w, 5e-5)
        print(f"{tag} {k}: {off} beyond 5e-5 (allowed {allowed:.0f}), max {worst:.3g}")
        H.close_enough(got[k], w, 5e-5, 6e-3, f"{tag} {k}")
    out = _predict(dev, N, pred)
    print(f"{tag}: predict max |diff| {float(np.abs(out - want_p).max()):.3g} (tolerance {H.predict_tol(case):g})")
    np.testing.assert_allclose(out, want_p, atol=H.predict_tol(case), rtol=0)
    return got_l


@pytest.mark.parametrize("case", H.SWEEP, ids=H.SWEEP_IDS)
def test_boundary_sweep_against_the_oracle(case):
    """Three aae_vae_step with injected eps - the last batch ragged - and an aae_vae_predict on a cfg.vae_wide handle, against
    OracleVAE.  The case at the bound (1024, 512): aae_vae_predict at 6e-5 = 4 x 1.5e-5, the ceiling vae_hwide_cases.py states for
    the float32 oracle's own distance from the float64 oracle on these inputs (1.28e-5 measured on the CPU, asserted by
    test_vae_hwide_cpu.py); measured on an MI355X: 8.0e-6.  Every other figure as everywhere."""
    h, c, inc, B, act, opt, N, _ = case
    p, steps, pred = H.sweep_inputs(*case)
    dev = _handle(N, h, c, inc, B, activation=act, optimizer=opt)
    dev.load_params(to_hip(p))
    _against_oracle(dev, case, p, steps, pred, H.SWEEP_IDS[H.SWEEP.index(case)])


# ---- 8. the two routes agree -----------------------------------------------------------------------------------------------
def test_the_chain_route_and_the_layer_route_agree_and_the_flag_alone_changes_no_bit():
    from aaerec import _hip
    case = H.ROUTES_CASE
    h, c, inc, B, act, opt, N, _ = case
    p, steps, pred = H.sweep_inputs(*case)
    chain, layer, flag = _handle(N, h, c, inc, B, wide=False), _handle(N, h, c, inc, B, no_chain=True), _handle(N, h, c, inc, B)
    for d in (chain, layer, flag):
        d.load_params(to_hip(p))
        d.profile_enable(True, kernels=(_hip.K_CHAIN, _hip.K_VAE_REPARAM))
    l_chain = _against_oracle(chain, case, p, steps, pred, "chain route")
    l_layer = _against_oracle(layer, case, p, steps, pred, "layer route")
    n_chain, n_layer = _launches(chain), _launches(layer)
    print("launches (chain programs, reparametrisation kernels): chain route", n_chain, "layer route", n_layer)
    assert n_chain[0] > 0 and n_chain[1] == 0
    assert n_layer == (0, 2 * len(steps) + 1)               # forward + backward a step, the predict's forward: no silent fallback
    Bs = steps[-1][0]
    dzc_c, dzc_l = chain.cond_grad(Bs).cpu().numpy(), layer.cond_grad(Bs).cpu().numpy()
    print(f"AAE_T_ACT_DZC: max |diff| between the routes {float(np.abs(dzc_c - dzc_l).max()):.3g}, largest entry {float(np.abs(dzc_c).max()):.3g}")
    assert np.abs(dzc_c).max() > 0
    np.testing.assert_allclose(dzc_l, dzc_c, atol=1e-6, rtol=0)
    # the flag without NO_CHAIN at this size: the handle of before - every parameter and both losses, bit for bit
    l_flag = _run_steps(flag, N, steps)
    assert _launches(flag)[1] == 0
    a, b = chain.state_dict(), flag.state_dict()
    for k in a:
        np.testing.assert_array_equal(b[k], a[k], err_msg=k)
    for (b0, k0, _), (b1, k1, _) in zip(l_chain, l_flag):
        assert b0 == b1
        np.testing.assert_allclose(k1, k0, rtol=1e-6)        # (the chain op's KL sum: one float atomic per row, any order)
    assert len(l_layer) == len(l_chain)
    # without the flag the refusal of before
    with _no_chain():
        old = _handle(N, h, c, inc, B, wide=False)
    Bs, ip, idx, val, eps, cond = steps[0]
    with pytest.raises(_hip.AaeHipError, match=r"error -4: VAE mode needs the layer-chain kernels"):
        old.vae_step(_csr(old, ip, idx, val, N), 0, Bs, cond=_t(old, cond), eps=eps)


# ---- 9. one generator definition -------------------------------------------------------------------------------------------
def test_device_draws_on_the_layer_route_are_the_generators_and_the_kl_sum_has_one_order():
    """rng_mode='device' on a layer-route handle.  The kernels' draws are read off the device - aae_vae_encode(train) on a twin
    whose [fc21; fc22] is zero returns z = 0 + eps * exp(0), the draws' own bits - and held to the host restatement
    device_rng.vae_eps at its stated accuracy (5e-6: the restatement evaluates the Gaussian in float64, the kernels in fp32, so
    its values are not the kernels' bits); a handle fed those draws as injected eps then equals the drawing handle bit for bit,
    parameters and both losses.  aae_vae_predict_loss over 40 rows in one call equals two calls of 20 rows with row0 = 0, 20
    bit for bit, and a second run of everything gives the same bits (the fixed-order KL sum)."""
    N, h, c, inc, B, seed = 257, 300, 100, 30, 40, 4242
    p = vae_params(N, h, c, inc, seed=9)
    r = np.random.default_rng(9)
    batches = [corpus(r, N, B, 9)[:3] + ((r.standard_normal((B, inc)) * 0.4).astype(np.float32),) for _ in range(3)]
    probe_p = {k: (np.zeros_like(v) if k.startswith(("fc21", "fc22")) else v) for k, v in p.items()}

    def run(inject):
        dev = _handle(N, h, c, inc, B, rng_mode="device", seed=seed)
        dev.load_params(to_hip(p))
        losses = []
        for s, (ip, idx, val, cond) in enumerate(batches):
            dev.vae_step(_csr(dev, ip, idx, val, N), 0, B, cond=_t(dev, cond), eps=None if inject is None else inject[s])
            losses.append(tuple(float(x) for x in dev.losses()[:2]))
        ip, idx, val, cond = batches[0]
        csr = _csr(dev, ip, idx, val, N)
        one = dev.vae_predict_loss(csr, 0, B, cond=_t(dev, cond), eps=None, row0=0)
        two = [dev.vae_predict_loss(csr, lo, 20, cond=_t(dev, cond[lo:lo + 20]), eps=None, row0=lo) for lo in (0, 20)]
        rows = [torch.cat([t[i] for t in two]).cpu().numpy() for i in (0, 1)]
        return dev.state_dict(), losses, [one[0].cpu().numpy(), one[1].cpu().numpy()], rows
    probe = _handle(N, h, c, inc, B, rng_mode="device", seed=seed)
    probe.load_params(to_hip(probe_p))
    draws = []
    for s, (ip, idx, val, _) in enumerate(batches):
        e = probe.vae_encode(_csr(probe, ip, idx, val, N), 0, B, eps=None, train=True).cpu().numpy()
        want = R.vae_eps(seed, R.step_value(s + 1), R.EPS_STREAM, B, c)
        print(f"step {s + 1}: the device's draws against the host restatement, max |diff| {float(np.abs(e - want).max()):.3g}")
        np.testing.assert_allclose(e, want, atol=5e-6, rtol=0)
        assert abs(float(e.std()) - 1.0) < 0.05
        draws.append(e)
    sd_dev, l_dev, one, two = run(None)
    sd_inj, l_inj, _, _ = run(draws)
    for k in sd_dev:
        np.testing.assert_array_equal(sd_inj[k], sd_dev[k], err_msg=k)
    assert l_inj == l_dev, (l_inj, l_dev)
    for a, b in zip(one, two):
        np.testing.assert_array_equal(a, b)                  # row0 reaches the generator row on this route
    sd2, l2, one2, _ = run(None)
    assert l2 == l_dev and all(np.array_equal(a, b) for a, b in zip(one, one2))
    for k in sd_dev:
        np.testing.assert_array_equal(sd2[k], sd_dev[k], err_msg=k)


# ---- 10. the cut route -----------------------------------------------------------------------------------------------------
def test_cut_step_equals_the_whole_step_bit_for_bit_on_the_layer_route():
    """aae_vae_encode(train) -> the caller concatenates the block -> aae_vae_decode_backward -> aae_vae_encoder_backward(dzc[:, :c])
    on a (300, 100, cond_inc 30) handle: the launches of aae_vae_step in the same order, so the same bits."""
    N, h, c, inc, B = 257, 300, 100, 30, 21
    p = vae_params(N, h, c, inc, seed=5)
    r = np.random.default_rng(5)
    whole, cut = _handle(N, h, c, inc, B), _handle(N, h, c, inc, B)
    for m in (whole, cut):
        m.load_params(to_hip(p))
    for s in range(2):
        ip, idx, val, _ = corpus(r, N, B, 9)
        eps = r.standard_normal((B, c)).astype(np.float32)
        cond = torch.as_tensor((r.standard_normal((B, inc)) * 0.4).astype(np.float32), device=cut.device)
        whole.vae_step(_csr(whole, ip, idx, val, N), 0, B, cond=cond, eps=eps)
        z = cut.vae_encode(_csr(cut, ip, idx, val, N), 0, B, eps=eps, train=True)
        dzc = cut.vae_decode_backward(torch.cat([z, cond], 1))
        assert dzc.shape == (B, c + inc)
        np.testing.assert_array_equal(dzc[:, c:].cpu().numpy(), whole.cond_grad(B).cpu().numpy())
        cut.vae_encoder_backward(dzc[:, :c].contiguous())
        assert tuple(cut.losses()[:2]) == tuple(whole.losses()[:2])
    a, b = whole.state_dict(), cut.state_dict()
    for k in a:
        np.testing.assert_array_equal(b[k], a[k], err_msg=k)
    assert not np.array_equal(a["enc.lin3.weight"], to_hip(p)["enc.lin3.weight"])


# ---- 11. ranking and loss --------------------------------------------------------------------------------------------------
def _scaled(full):
    lo, hi = full.min(1), full.max(1)
    return (full - lo[:, None]) / np.where(hi > lo, hi - lo, 1.0)[:, None]


def _check_lists(ids, vals, want_ids, want_vals, scaled, k, tol, what):
    """test_rank_vae_gpu.py's rule: scaled scores within tol; ids differ only where the two items' scores lie within tol."""
    np.testing.assert_allclose(vals, want_vals, atol=tol, err_msg=what)
    b, j = np.nonzero(ids != want_ids)
    assert not ((ids[b, j] < 0) | (want_ids[b, j] < 0)).any(), (what, "a padded position differs")
    gap = np.abs(scaled[b, np.maximum(ids[b, j], 0)] - scaled[b, np.maximum(want_ids[b, j], 0)])
    print(f"{what}: k={k} positions that differ={len(b)} their largest score gap={float(gap.max()) if len(b) else 0.0:.3g}")
    assert np.all(gap <= tol), (what, len(b), float(gap.max()))


def test_rank_and_loss_calls_take_their_dense_forms_at_any_width():
    """(300, 100), 40 rows, 257 items: aae_vae_predict_topk (k = 10, 40) and aae_vae_predict_ranks against the host ranker over
    aae_vae_predict's own scores; aae_vae_predict_loss and VAE.eval_loss against OracleVAE (loss_cases.py's restatement); the
    *_max_rows calls answer max_batch."""
    from aaerec import ranking
    from aaerec._hip import DeviceCSR
    from aaerec.vae import VAE
    from oracle import aae_oracle as O
    N, h, c, R_, rows = 257, 300, 100, 64, 40
    r = np.random.default_rng(300)
    p = vae_params(N, h, c, 0, seed=300, spread=8.0)
    m = VAE(N, N, n_hidden=h, n_code=c, lr=1e-3, batch_size=R_, verbose=False, rng_mode="reference")
    dev = m.hip
    assert dev.cfg.vae_wide == 1
    dev.load_params(to_hip(p))
    tip, tidx, tval, _ = corpus(r, N, R_, 30)            # one training step first: the handle has run
    teps = r.standard_normal((R_, c)).astype(np.float32)
    dev.vae_step(_csr(dev, tip, tidx, tval, N), 0, R_, eps=teps)
    ora = O.OracleVAE(p, lr=1e-3)
    ora.partial_fit(tip, tidx, tval, teps)
    ip, idx, val, docs = corpus(r, N, rows, 30)
    X = sp.csr_matrix((val, idx, ip), shape=(rows, N))
    csr = _csr(dev, ip, idx, val, N)
    eps_np = r.standard_normal((rows, c)).astype(np.float32)
    eps = torch.as_tensor(eps_np, device=dev.device)
    full = dev.vae_predict(csr, 0, rows, eps=eps).cpu().numpy()
    scaled = _scaled(full.astype(np.float64))
    assert dev.vae_rank_max_rows(10) == R_ and dev.vae_rank_max_rows(40) == R_ and dev.vae_rank_full_max_rows() == R_
    assert dev.loss_max_rows() == R_

    def scale32(s, best):      # min-max over ALL the row's scores, in float32 as the device scales
        row = s.astype(np.float32)
        lo, hi = row.min(), row.max()
        return (row[best] - lo) * (np.float32(1.0) / (hi - lo) if hi > lo else np.float32(1.0))
    for k in (10, 40):
        want_ids, want_vals = ranking.host_topk(ranking.host_rows(X, lambda a, b: full[a:b]), rows, k, scale32)
        ids, vals = dev.vae_predict_topk(csr, 0, rows, k, eps=eps, exclude_known=True)
        _check_lists(ids.cpu().numpy(), vals.cpu().numpy(), want_ids, want_vals, scaled, k, 2e-6, "predict_topk")
    trows = [np.sort(r.choice(np.setdiff1d(np.arange(N), d), size=3, replace=False)) for d in docs]
    Y = sp.csr_matrix((np.ones(3 * rows, dtype=np.float32), np.concatenate(trows), np.arange(0, 3 * rows + 1, 3)), shape=(rows, N))
    Ys = ranking.canonical_truth(Y, X.shape)
    want = ranking.host_ranks(ranking.host_rows(X, lambda a, b: full[a:b]), Ys).data
    near = np.array([np.sort(np.abs(scaled[b] - scaled[b, t]))[1] <= 2e-6 for b in range(rows) for t in Ys.indices[Ys.indptr[b]:Ys.indptr[b + 1]]])
    assert near.mean() <= 0.02, near.mean()
    got = dev.vae_predict_ranks(csr, 0, rows, DeviceCSR(Ys, dev.device), eps=eps, exclude_known=True).cpu().numpy()
    np.testing.assert_array_equal(got[~near], want[~near])
    # the held-out loss: rows against the restatement of the oracle's logits (test_eval_loss_gpu.py's rule and figures)
    logits, mu, lv = LC.vae_logits(ora, ip, idx, val, eps_np)
    assert LC.zone_clear(logits)
    want_b, want_k = LC.row_bce(logits, ip, idx, val), LC.row_kl(mu, lv)
    bce, kl = (t.cpu().numpy() for t in dev.vae_predict_loss(csr, 0, rows, eps=eps, row0=0))
    tol = LC.row_bound(logits, ip, idx, val) + LC.TOL_LOSS * np.abs(want_b)
    print(f"loss rows: largest share of a row's tolerance {float((np.abs(bce - want_b) / tol).max()):.3g}; KL max relative diff {float(np.abs(kl / want_k - 1).max()):.3g}")
    assert np.all(np.abs(bce - want_b) <= tol)
    np.testing.assert_allclose(kl, want_k, rtol=2e-5, atol=c * 2.0 ** -23)
    m._eps = lambda n: torch.from_numpy(eps_np[:n])
    np.testing.assert_allclose(m.eval_loss(X), LC.reference_test_loss(want_b, want_k, N, R_), rtol=2e-5)


def _bags():
    from aaerec.datasets import Bags
    rng = np.random.RandomState(0)
    protos = [rng.choice(300, size=8, replace=False) for _ in range(30)]
    data, owners, years = [], [], {}
    for i in range(600):
        k = rng.randint(30)
        data.append(["i%d" % t for t in rng.choice(protos[k], size=rng.randint(4, 8), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // 600
    return Bags(data, owners, {"year": years})


def test_the_reference_grid_point_runs_through_evaluation():
    """VAERecommender(n_hidden=300, n_code=100) - the reference's own grid point - trained and ranked by Evaluation on the small
    corpus of test_rank_recommenders_gpu.py; metrics_on="device" gives the host's numbers (test_metrics_gpu.py's bound)."""
    import metric_cases as MC
    from aaerec.evaluation import Evaluation
    from aaerec.vae import VAERecommender
    names = ["mrr@10", "map@10", "p@5", "ndcg@10"]
    np.random.seed(3)
    torch.manual_seed(3)
    ev = Evaluation(_bags(), 2009, metrics=names, logfile=None, topk=True).setup(min_elements=2, drop=1)
    n = ev.y_test.shape[0]
    rec = VAERecommender(n_hidden=300, n_code=100, n_epochs=2, batch_size=50, lr=0.01, verbose=False, seed=11)
    host = ev([rec])[0]
    assert rec.model.hip.cfg.vae_wide == 1
    rec.train = lambda training_set: None                     # (the same trained model answers the second run)
    ev.metrics_on = "device"
    dev = ev([rec])[0]
    row_eps = 2 * (2 + 2) * MC.U
    for name, (m_h, s_h), (m_d, s_d) in zip(names, host, dev):
        print(name, "host", repr(float(m_h)), repr(float(s_h)), "device", repr(float(m_d)), repr(float(s_d)))
        assert abs(m_d - m_h) <= (row_eps + 2 * (n + 1) * MC.U) * abs(m_h), name
        assert abs(s_d * s_d - s_h * s_h) <= 2 * ((n + 8) * 2.0 ** -52 + 4 * row_eps), name
    assert all(np.isfinite(v) for pair in dev for v in pair)
    out = rec.predict(ev.test_set.clone())
    assert out.shape[0] == n and np.all(np.isfinite(out))


# ---- 12. checkpoint --------------------------------------------------------------------------------------------------------
def test_hwide_vae_saved_and_restored_continues_bit_for_bit():
    """aaerec.vae.VAE(n_hidden=300, n_code=100): 2 steps, the checkpoint through the C ABI (test_checkpoint_gpu.py's helpers),
    2 more; a new VAE loaded from the checkpoint runs the same 2 - every parameter, moment, step count and, on this route, the
    logged loss with its fixed-order KL sum: equal bits."""
    from aaerec.vae import VAE
    from test_checkpoint_gpu import abi_load, abi_store, assert_same_checkpoint
    N, h, c, B = 257, 300, 100, 9
    r = np.random.default_rng(12)
    p = to_hip(vae_params(N, h, c, 0, seed=12))
    steps = []
    for _ in range(4):
        ip, idx, val, _ = corpus(r, N, B, 7)
        steps.append((sp.csr_matrix((val, idx, ip), shape=(B, N)), r.standard_normal((B, c)).astype(np.float32)))

    def make():
        return VAE(N, N, n_hidden=h, n_code=c, lr=2e-3, batch_size=B, verbose=True, rng_mode="reference")

    def run(m, lo, hi):
        out = []
        for X, eps in steps[lo:hi]:
            m._eps = lambda n, eps=eps: torch.from_numpy(eps)
            m.partial_fit(X)
            out.append(m.last_loss)
        return out
    a = make()
    a.hip.load_params(p)
    run(a, 0, 2)
    ck = abi_store(a.hip)
    assert ck["params"]["dec.lin1.weight"].shape == (h, c) and ck["params"]["enc.lin3.weight"].shape == (2 * c, h)
    la = run(a, 2, 4)
    b = make()
    abi_load(b.hip, ck)
    lb = run(b, 2, 4)
    assert la == lb, (la, lb)
    end_a, end_b = abi_store(a.hip), abi_store(b.hip)
    assert_same_checkpoint(end_a, end_b, "resumed (300, 100)")
    assert not np.array_equal(end_a["params"]["dec.lin1.weight"], ck["params"]["dec.lin1.weight"])
