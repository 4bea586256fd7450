"""rng_mode='device' (what fit() and the benchmark run) against rng_mode='inject' fed the draws of tests/device_rng.py, the
NumPy restatement of the counter generator: two handles with the same parameters, one drawing its dropout masks, prior
sample and eps in the kernels, the other handed them - the three losses after every step and the whole state_dict() at the
end must agree.  The injected path is the one every fixture, fuzzer and sweep of the suite already pins to the reference, so
this holds every copy of the keep rule (drop_keep, chain_keep, the GEMM epilogues), every caller of the one Box-Muller /
categorical draw (draw_gauss / draw_class through prior_cell, device_common.h: prior_kernel and the COP_PRIOR op of chain.h,
chain4.h, chain16x3.h; the reparametrisation draw of COP_REPARAM in chain.h and chain4.h) - the key, row and column each of
them hands it -, the step value of the forward and of the recomputed backward masks, the stream ids and the row offsets to
ONE definition.

Shape: N = 700, h = 48, c = 12, B = 37 (no multiple of the 4- or 16-row blocks), B = 1, and B = 40 (a multiple of 4: the
discriminator program then carries the encoder's evaluation pass as a prefix of its upper rows).  Three steps per case: the
counter advances, and the first step's in-launch advance (enc_gather_kernel_t's step_val) is part of it.

Tolerance: atol 2e-5, what the suite holds a step to against its oracle (test_parity_abi_gpu.py::test_tiny_shapes_match_oracle).
The two handles run the same kernels on the same numbers but for the Gaussian draws, where the restatement's float64
sqrt(-2 ln f1) cos(2 pi f2) differs from the kernels' fp32 logf / cosf by less than 5e-6 (device_rng.py); one wrong keep
bit moves an activation by O(0.1) and a weight by O(lr), a hundred times the tolerance (test_the_comparison_is_sensitive).
The VAE cases use the tolerances of test_parity_abi_gpu.py::test_vae_step_matches_reference."""
import functools

import numpy as np
import pytest
import torch

import device_rng as R

pytestmark = pytest.mark.gpu

N, H, C = 700, 48, 12
ATOL = 2e-5                     # test_tiny_shapes_match_oracle
VAE_LOSS_RTOL, VAE_PARAM_ATOL, VAE_RECON_ATOL = 2e-5, 1e-5, 1e-5      # test_vae_step_matches_reference (TOL_PARAM, TOL_RECON)
LRS = dict(gen_lr=2e-3, reg_lr=1e-3)      # test_device_rng_draws_by_global_row_so_ranks_reproduce_the_single_process_run
DROP = (0.2, 0.3)
STEPS = 3
PATHS = {"default": None, "x16": ("X16_ROWS", 1), "chain16": ("CHAIN16", 1), "no_chain": ("NO_CHAIN", 1)}


@functools.lru_cache(maxsize=None)
def corpus(rows, seed=0):
    """`rows` documents of 1-9 items (ones), as CSR arrays."""
    r = np.random.default_rng(100 + seed)
    docs = [np.sort(r.choice(N, size=int(r.integers(1, 10)), replace=False)) for _ in range(rows)]
    ip = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    idx = np.concatenate(docs).astype(np.int32)
    return ip, idx, np.ones(len(idx), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def aae_params():
    from oracle.dense_torch_port import init_params
    return init_params(N, H, C, seed=9)


@functools.lru_cache(maxsize=None)
def vae_params():
    """The VAE's five Linears under the handle's names: enc.lin3 holds [fc21; fc22] (2c rows)."""
    from oracle.dense_torch_port import init_params
    p, wide = init_params(N, H, C, seed=9), init_params(N, H, 2 * C, seed=10)
    return {"enc.lin1.weight": p["enc.lin1.weight"], "enc.lin1.bias": p["enc.lin1.bias"],
            "enc.lin3.weight": wide["enc.lin3.weight"], "enc.lin3.bias": wide["enc.lin3.bias"],
            "dec.lin1.weight": p["dec.lin1.weight"], "dec.lin1.bias": p["dec.lin1.bias"],
            "dec.lin3.weight": p["dec.lin3.weight"], "dec.lin3.bias": p["dec.lin3.bias"]}


def make(path, rng_mode, B, seed=0, params=None, **kw):
    """A handle on the asked kernel path (a handle reads its switches once, at creation).  The handle cannot report which
    chain kernel a program ran on (its profile has one id for all of them), so the tests take the switch on trust.  A kernel
    trace of two steps at B = 37 (default also at 40) showed, once: default 10 launches of chain4_kernel and none of the others for the
    AAE step; X16_ROWS=1 the same 10 on chain16x3_kernel, none on chain4_kernel; CHAIN16 all on chain_kernel; NO_CHAIN no
    chain kernel, prior_kernel and the gemm_f32_kernel epilogues.  The VAE's training and predict programs ran on
    chain_kernel on every path, its rank call on chain4_kernel's VAE member (default and X16_ROWS alone have it)."""
    from aaerec import _hip
    opt = PATHS[path]
    if opt:
        _hip.set_option(opt[0], opt[1])
    try:
        m = _hip.HipAAE(N, H, C, max_batch=B, rng_mode=rng_mode, seed=seed, **LRS, **kw)
    finally:
        if opt:
            _hip.set_option(opt[0], None)
    m.load_params(aae_params() if params is None else params)
    return m


def pair(path, B, seed, **kw):
    return make(path, "device", B, seed=seed, **kw), make(path, "inject", B, **kw)


def csr_for(m, B):
    from aaerec._hip import DeviceCSR
    ip, idx, val = corpus(STEPS * B)
    return DeviceCSR.from_arrays(ip, idx, val, N, m.device)


def restated(seed, n, B, prior, dropout, row0=0, global_rows=0):
    """What the n-th step of a handle draws: (masks, z_real before prior_scale)."""
    step = R.step_value(n)
    return (R.dropout_masks(seed, step, dropout[0], dropout[1], B, H, row0=row0, global_rows=global_rows),
            R.prior(seed, step, prior, B, C, scale=1.0, row0=row0))


def state_deviation(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    worst = max(sa, key=lambda k: float(np.abs(sa[k] - sb[k]).max()))
    return float(np.abs(sa[worst] - sb[worst]).max()), worst


def run_aae(path, B, seed, prior="gauss", dropout=DROP, rows=None, tweak=None, **kw):
    """Three steps of both handles -> (largest loss deviation, largest parameter deviation, its name)."""
    dev, inj = pair(path, B, seed, prior=prior, dropout=dropout, **kw)
    row0, global_rows = rows if rows else (0, 0)
    if rows:
        dev.set_rng_rows(row0, global_rows)
    cd, ci = csr_for(dev, B), csr_for(inj, B)
    dl = 0.0
    for n in range(1, STEPS + 1):
        masks, z = restated(seed, n, B, prior, dropout, row0, global_rows)
        if tweak:
            masks = tweak(masks, n)
        dev.step(cd, (n - 1) * B, B)
        inj.step(ci, (n - 1) * B, B, masks=masks, z_real=z)
        ld, li = np.asarray(dev.losses(), dtype=np.float64), np.asarray(inj.losses(), dtype=np.float64)
        assert np.isfinite(ld).all() and np.isfinite(li).all(), (n, ld, li)
        dl = max(dl, float(np.abs(ld - li).max()))
    dp, worst = state_deviation(dev, inj)
    return dl, dp, worst


def check_aae(what, *a, **kw):
    dl, dp, worst = run_aae(*a, **kw)
    print(f"{what}: losses differ by {dl:.3g}, parameters by {dp:.3g} ({worst})")
    assert dl <= ATOL and dp <= ATOL, (what, dl, dp, worst)


# ---- 1. kernel path x dropout kind x prior ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["gauss", "categorical", "bernoulli"])
@pytest.mark.parametrize("activation", ["ReLU", "SELU"])            # nn.Dropout | nn.AlphaDropout
@pytest.mark.parametrize("path", list(PATHS))
def test_device_mode_equals_injected_restatement(path, activation, prior):
    check_aae(f"{path} {activation} {prior}", path, 37, 1234, prior=prior, activation=activation)


@pytest.mark.parametrize("path,B", [(p, 1) for p in PATHS] + [("default", 40), ("x16", 40), ("chain16", 40), ("no_chain", 40)])
def test_device_mode_equals_injected_restatement_one_row_and_merged_discriminator_program(path, B):
    check_aae(f"{path} B={B}", path, B, 7, prior="gauss", activation="ReLU")


@pytest.mark.parametrize("path", ["default", "no_chain"])
def test_device_mode_equals_injected_restatement_non_monotone_activation(path):
    """GELU: every layer program on chain_kernel<.., true>; the per-layer epilogues carry it too."""
    check_aae(f"{path} GELU", path, 37, 99, prior="gauss", activation="GELU")


@pytest.mark.parametrize("prior", ["gauss", "categorical"])
@pytest.mark.parametrize("path", list(PATHS))
def test_device_mode_equals_injected_restatement_with_a_prior_scale(path, prior):
    check_aae(f"{path} {prior} x 2.5", path, 37, 2 ** 63 + 5, prior=prior, activation="ReLU", prior_scale=2.5)


# ---- 2. the comparison is sensitive ----------------------------------------------------------------------------------------
def test_the_comparison_is_sensitive():
    """The restatement deliberately off in one place must miss by more than 100 x the tolerance: (a) streams 4 and 5
    swapped (the discriminator's two layers on [z_real; z_fake]); (b) step + 1 on streams 10 and 11, the discriminator's
    dropout of the generator phase: D is not updated there, so these masks reach the parameters through the backward pass
    alone (dL/dz into the encoder) - injected masks serve both passes of a layer, so a slip of the backward pass alone
    cannot be injected; this is the nearest one.  The untouched restatement of the same case is held to ATOL first."""
    B, seed = 37, 1234
    check_aae("untouched", "default", B, seed)

    def swap_4_5(masks, n):
        step, fake0 = R.step_value(n), B
        masks = list(masks)
        masks[4], masks[6] = R.keep(R.words(seed, step, 5, B, H, 0), DROP[0]), R.keep(R.words(seed, step, 5, B, H, fake0), DROP[0])
        masks[5], masks[7] = R.keep(R.words(seed, step, 4, B, H, 0), DROP[1]), R.keep(R.words(seed, step, 4, B, H, fake0), DROP[1])
        return masks

    def late_10_11(masks, n):
        late = R.dropout_masks(seed, R.step_value(n) + 1, DROP[0], DROP[1], B, H)
        return list(masks[:10]) + late[10:]

    for what, tweak in (("streams 4 and 5 swapped", swap_4_5), ("step + 1 on streams 10 and 11", late_10_11)):
        dl, dp, worst = run_aae("default", B, seed, tweak=tweak)
        print(f"{what}: losses differ by {dl:.3g}, parameters by {dp:.3g} ({worst})")
        assert max(dl, dp) > 100 * ATOL, (what, dl, dp)


# ---- 3. row offsets --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["gauss", "categorical"])
@pytest.mark.parametrize("path", list(PATHS))
def test_row_offsets_of_a_global_batch(path, prior):
    """aae_set_rng_rows(o, Bg), o != 0, Bg > B: masks and prior at global rows o + r, the discriminator's z_fake half at
    Bg + o + r (make_drop's goff_b)."""
    check_aae(f"{path} {prior} rows [5, 42) of 64", path, 37, 1, prior=prior, rows=(5, 64))


# ---- 4. the other models ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_plain_autoencoder(path):
    B, seed = 37, 7
    dev, inj = pair(path, B, seed, dropout=DROP, ae_only=True)
    cd, ci = csr_for(dev, B), csr_for(inj, B)
    for n in range(1, STEPS + 1):
        masks, _ = restated(seed, n, B, "gauss", DROP)
        dev.step(cd, (n - 1) * B, B)
        inj.step(ci, (n - 1) * B, B, masks=masks[:4] + [None] * 8)
        d = abs(float(dev.losses()[0]) - float(inj.losses()[0]))
        print(f"ae_only {path} step {n}: reconstruction losses differ by {d:.3g}")
        assert d <= ATOL
    dp, worst = state_deviation(dev, inj)
    print(f"ae_only {path}: parameters differ by {dp:.3g} ({worst})")
    assert dp <= ATOL


@pytest.mark.parametrize("path", list(PATHS))
def test_decoder_only_step(path):
    """aae_decoder_step: dec.drop1 / dec.drop2 are streams 2 and 3 of the step the call opens."""
    B, seed = 37, 99
    dev, inj = pair(path, B, seed, dropout=DROP)
    cd, ci = csr_for(dev, B), csr_for(inj, B)
    zin = np.random.default_rng(3).standard_normal((STEPS, B, C)).astype(np.float32)
    for n in range(1, STEPS + 1):
        masks, _ = restated(seed, n, B, "gauss", DROP)
        z = torch.as_tensor(zin[n - 1], device=dev.device)
        gd = dev.decoder_step(cd, (n - 1) * B, B, z)
        gi = inj.decoder_step(ci, (n - 1) * B, B, z, masks=(masks[2], masks[3]))
        d = abs(float(dev.losses()[0]) - float(inj.losses()[0]))
        dg = float((gd - gi).abs().max())
        print(f"decoder step {path} step {n}: losses differ by {d:.3g}, dL/dzin by {dg:.3g}")
        assert d <= ATOL and dg <= ATOL
    dp, worst = state_deviation(dev, inj)
    print(f"decoder step {path}: parameters differ by {dp:.3g} ({worst})")
    assert dp <= ATOL


def vae_pair(path, B, seed):
    kw = dict(dropout=(0.0, 0.0), vae=True, params=vae_params())
    return make(path, "device", B, seed=seed, **kw), make(path, "inject", B, **kw)


def vae_steps(dev, inj, B, seed, steps):
    cd, ci = csr_for(dev, B), csr_for(inj, B)
    for n in range(1, steps + 1):
        dev.vae_step(cd, (n - 1) * B, B)
        inj.vae_step(ci, (n - 1) * B, B, eps=R.vae_eps(seed, R.step_value(n), R.EPS_STREAM, B, C))
        ld, li = dev.losses(), inj.losses()
        print(f"vae step {n}: (BCE + KL) / B {(ld[0] + ld[1]) / B:.7g} device, {(li[0] + li[1]) / B:.7g} injected")
        np.testing.assert_allclose((ld[0] + ld[1]) / B, (li[0] + li[1]) / B, rtol=VAE_LOSS_RTOL)
    sa, sb = dev.state_dict(), inj.state_dict()
    assert sa.keys() == sb.keys() and set(vae_params()) <= set(sa)
    for k in sa:                                # (every tensor of the handle, the layers a VAE leaves alone included)
        d = float(np.abs(sa[k] - sb[k]).max())
        if k in vae_params():
            print(f"vae {k}: differs by {d:.3g}")
        assert d <= VAE_PARAM_ATOL, k


@pytest.mark.parametrize("path,B", [("default", 37), ("chain16", 37), ("default", 1)])
def test_vae_step(path, B):
    """eps of reparametrize(): stream 12, the row within the call; the training programs run on chain.h's kernel on both
    paths (COP_REPARAM_BWD lives there alone), with the step's first layer on either gather form."""
    dev, inj = vae_pair(path, B, 1234)
    vae_steps(dev, inj, B, 1234, STEPS)


# ---- 5. the VAE's predict calls over more rows than max_batch --------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "chain16"])
def test_vae_predict_over_more_rows_than_max_batch(path):
    """include/aaerec_hip.h: a VAE call draws eps for (seed, step, ROW OF THE CALL, column).  Rows beyond max_batch reach the
    generator in two ways: aae_vae_predict called once per max_batch rows (chain.h's COP_REPARAM, which has no row offset:
    every call counts its rows from 0 - what VAE.predict does), and ONE rank call of more rows than max_batch
    (aae_vae_predict_topk on the 4-row kernel's COP_REPARAM member, rows 0 .. n - 1 of the call; its row offset serves the
    re-ranked spans of that call alone).  Both against inject mode with eps restated for those rows, after one training
    step (step value 1).  On the CHAIN16 path the rank call has no fused form and takes max_batch rows like aae_vae_predict."""
    from aaerec._hip import DeviceCSR
    B, seed, rows = 37, 99, 2 * 37 + 5
    dev, inj = vae_pair(path, B, seed)
    vae_steps(dev, inj, B, seed, 1)
    ip, idx, val = corpus(rows, seed=1)
    cd, ci = DeviceCSR.from_arrays(ip, idx, val, N, dev.device), DeviceCSR.from_arrays(ip, idx, val, N, inj.device)
    step = 1                                  # a predict call opens no step: the count of the steps opened so far
    for lo in range(0, rows, B):
        n = min(B, rows - lo)
        got = dev.vae_predict(cd, lo, n).cpu().numpy()
        want = inj.vae_predict(ci, lo, n, eps=R.vae_eps(seed, step, R.EPS_STREAM, n, C)).cpu().numpy()
        zero = inj.vae_predict(ci, lo, n, eps=np.zeros((n, C), dtype=np.float32)).cpu().numpy()
        d = float(np.abs(got - want).max())
        print(f"{path} aae_vae_predict rows [{lo}, {lo + n}): differs by {d:.3g} (eps = 0 would differ by {np.abs(got - zero).max():.3g})")
        assert np.abs(got - zero).max() > 100 * VAE_RECON_ATOL          # (the draw matters: a wrong one cannot hide)
        assert d <= VAE_RECON_ATOL
    k = 10
    cap = dev.vae_rank_max_rows(k)
    assert cap == inj.vae_rank_max_rows(k)
    if path == "default":
        assert cap >= rows > B, cap           # one fused call over all rows: chain4.h's COP_REPARAM member
    else:
        assert cap == B, cap
    n = min(cap, rows)
    ids, vals = dev.vae_predict_topk(cd, 0, n, k)
    ids_i, vals_i = inj.vae_predict_topk(ci, 0, n, k, eps=R.vae_eps(seed, step, R.EPS_STREAM, n, C))
    ids, vals, ids_i, vals_i = ids.cpu().numpy(), vals.cpu().numpy(), ids_i.cpu().numpy(), vals_i.cpu().numpy()
    d = float(np.abs(vals - vals_i).max())
    print(f"{path} aae_vae_predict_topk of {n} rows: scaled scores differ by {d:.3g}, {int((ids != ids_i).sum())} of {ids.size} ids")
    assert d <= VAE_RECON_ATOL
    # an id may differ only where the list holds a near tie: a neighbour's score within the two lists' tolerance of its own
    gap = np.full(vals.shape, np.inf)
    gap[:, 1:] = np.minimum(gap[:, 1:], np.abs(np.diff(vals_i, axis=1)))
    gap[:, :-1] = np.minimum(gap[:, :-1], np.abs(np.diff(vals_i, axis=1)))
    assert np.all((ids == ids_i) | (gap <= 2 * VAE_RECON_ATOL))


# ---- 6. one seed, one run --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", ["gauss", "categorical"])
def test_one_seed_gives_one_run_on_the_per_layer_path_and_the_chain_path(prior):
    """rng_mode='device' on both sides: the per-layer path (NO_CHAIN; any model with h + 1 > 208 takes it) draws z_real in
    prior_kernel, the chain path in its COP_PRIOR op - one generator, so one run."""
    B, seed = 37, 1234
    a = make("default", "device", B, seed=seed, prior=prior, dropout=DROP)
    b = make("no_chain", "device", B, seed=seed, prior=prior, dropout=DROP)
    ca, cb = csr_for(a, B), csr_for(b, B)
    for n in range(1, STEPS + 1):
        a.step(ca, (n - 1) * B, B)
        b.step(cb, (n - 1) * B, B)
        la, lb = np.asarray(a.losses(), dtype=np.float64), np.asarray(b.losses(), dtype=np.float64)
        print(f"{prior} step {n}: losses {la} chain, {lb} per layer, differ by {np.abs(la - lb).max():.3g}")
        assert np.abs(la - lb).max() <= ATOL
    dp, worst = state_deviation(a, b)
    print(f"{prior}: parameters differ by {dp:.3g} ({worst})")
    assert dp <= ATOL
