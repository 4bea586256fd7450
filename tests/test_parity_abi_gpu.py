"""GPU parity, through the C ABI: replay every golden fixture (generated from the real
reference by tools/gen_golden.py) on libaaerec_hip.so with the recorded randomness injected,
and compare losses, parameters and Adam states after every step.

Tolerances (fp32): losses 1e-5 relative; parameters 1e-5 absolute (Adam turns an fp32
summation-order difference of a ~1e-8 gradient into a few 1e-6 of parameter, see
tests/test_oracle_golden.py); reconstructions 1e-5 absolute (north star: 1e-4).

step_saturated (dec.lin3 x 400: a thousand zero-target logits beyond 24 ln 2, where the reference's fp32 sigmoid is exactly
1.0 - loss 100, gradient 0 - and thousands just below, where its 1 - sigmoid is quantised in steps of 2^-24) is replayed at
the same tolerances on every quantity but the reconstruction loss, whose bound is DERIVED from the reference-side logits
(golden_util.bce_quantisation_bound) - the kernels' softplus is exact where the reference's logarithm is not."""
import functools

import numpy as np
import pytest
import torch

from golden_util import ACT_CASES, STEP_CASES, Fixture, bce_quantisation_bound

pytestmark = pytest.mark.gpu

TOL_LOSS, TOL_PARAM, TOL_RECON = 1e-5, 1e-5, 1e-5
FUSED_CASES = [c for c in STEP_CASES if c not in ("step_cond_categorical", "step_cond_concat_bias")]


def make_model(fx, **over):
    from aaerec._hip import HipAAE
    c = fx.cfg
    kw = fx.model_kwargs()
    kw.update(over)
    inc = c["cond_inc"]
    m = HipAAE(c["N"], c["h"], c["c"], cond_inc=inc, max_batch=c["B"], rng_mode="inject", **kw)
    m.load_params(fx.init_params())
    return m


def csr_of(fx, m, s, prefix=None):
    from aaerec._hip import DeviceCSR
    ip, idx, val = fx.batch(s, prefix)
    return DeviceCSR.from_arrays(ip, idx, val, fx.cfg["N"], m.device)


def check_state(fx, m, s, name):
    got = m.state_dict()
    for k, w in fx.expected_params(s).items():
        np.testing.assert_allclose(got[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k}")
    exp = fx.expected_adam(s)
    if not exp:
        return
    states = {"A_enc": m.adam_state("enc"), "A_dec": m.adam_state("dec")}
    if any(t in ("A_gen", "A_disc") for t, _ in exp):
        states.update({"A_gen": m.adam_state("gen"), "A_disc": m.adam_state("disc")})
    for (tag, k), (em, ev, et) in exp.items():
        st = states[tag]
        gm, gv = st[k.split(".", 1)[1]]
        assert st["step"] == et
        np.testing.assert_allclose(gm, em, atol=2e-9, rtol=1e-4, err_msg=f"{name} {tag} m {k}")
        np.testing.assert_allclose(gv, ev, atol=1e-12, rtol=2e-4, err_msg=f"{name} {tag} v {k}")


@functools.lru_cache(maxsize=None)
def recon_loss_bounds(name):
    """Per step of a fixture in the saturated regime: the derived bound on |kernels' reconstruction loss - reference's| from
    the REFERENCE-side logits - the CPU oracle's replay of the fixture (pinned to the reference by tests/test_oracle_golden.py),
    never the device's."""
    from test_oracle_golden import build_oracle
    fx = Fixture(name)
    ora = build_oracle(fx)
    out = []
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        ora.partial_fit(ip, idx, val, fx.z[f"step{s}.z_real"], fx.masks(s), fx.cond_inputs(s))
        out.append(bce_quantisation_bound(ora.last["logits"], ip, idx))
    return tuple(out)


def check_losses(fx, s, got, name):
    want = fx.z[f"step{s}.losses"]
    if "saturation" not in fx.cfg:
        np.testing.assert_allclose(got, want, rtol=TOL_LOSS, atol=1e-6, err_msg=f"{name} step {s} losses")
        return
    np.testing.assert_allclose(got[1:], want[1:], rtol=TOL_LOSS, atol=1e-6, err_msg=f"{name} step {s} adversarial losses")
    bound = recon_loss_bounds(name)[s]
    tol = bound + TOL_LOSS * abs(want[0])
    print(f"{name} step {s}: reconstruction loss {got[0]:.6f}, reference {want[0]:.6f}, difference {got[0] - want[0]:+.6f}, "
          f"derived bound {bound:.6f} + {TOL_LOSS:g} relative")
    assert abs(got[0] - want[0]) <= tol, (name, s, got[0], want[0], tol)


@pytest.mark.parametrize("name", FUSED_CASES + ACT_CASES)
def test_step_matches_reference(name):
    fx = Fixture(name)
    m = make_model(fx)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = fx.cond_inputs(s)
        cond_t = torch.as_tensor(cond[0], device=m.device) if cond else None
        m.step(csr, 0, B, cond=cond_t, masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
        check_losses(fx, s, m.losses(), name)
        if fx.has_state(s):
            check_state(fx, m, s, name)
    # predict with the trained weights (ragged last predict batch is the host's job: one call here)
    pcsr = csr_of(fx, m, 0, prefix="predict")
    pc = fx.cond_inputs(0, prefix="predict")
    pc_t = torch.as_tensor(pc[0], device=m.device) if pc else None
    out = m.predict(pcsr, 0, pcsr.shape[0], cond=pc_t).cpu().numpy()
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)


@pytest.mark.parametrize("name", ["step_headline", "step_masks", "step_wide", "step_ragged", "step_cond_concat", "step_sgd",
                                  "step_lrs", "step_selu", "step_nonorm", "step_saturated"])
def test_step_matches_reference_through_the_split_output_layer(name, monkeypatch):
    """The same replay with the output layer in the form the benchmark's shapes take (AAE_SPLIT_ANY lifts the size rule
    that keeps small layers on the single launch): the CRITICAL launch with its fp32 products emulated on the bf16 matrix
    cores (csrc/dec_crit_x3.h: three bf16 terms per operand, six cross products, fp32 accumulation - 16, 7-block and
    13-block widths, ragged / empty rows, a condition block, SGD) and the DEFERRED optimiser launch on the side stream -
    against the reference's recorded losses, parameters and Adam moments at the SAME tolerances as the fp32 kernels."""
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    test_step_matches_reference(name)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_step_matches_reference_on_the_wide_batch_chain_kernel(name, monkeypatch):
    """The same replay with every layer-chain program on the wide-batch kernel (r5, csrc/chain16x3.h; AAE_X16_ROWS=1 lifts
    the 256-row rule): 16 rows per workgroup, activations as three bf16 planes in LDS, the hidden layers' fp32 products
    emulated by six bf16 products against the split weight copies the optimiser epilogues keep (device_common.h FX / DX),
    slots renamed by live range - every option of the path (dropout, conditions incl. the two-part decoder input,
    SELU / Tanh, priors with a softmax / sigmoid code, SGD, ragged / empty / short batches, the merged discriminator
    program's prefix on workgroups that straddle the z_real / z_fake boundary) against the reference's recorded losses,
    parameters and Adam moments at the SAME tolerances as the fp32 kernels."""
    monkeypatch.setenv("AAE_X16_ROWS", "1")
    test_step_matches_reference(name)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_step_matches_reference_on_the_k_split_weight_gradient_tiles(name, monkeypatch):
    """The same replay with every weight-gradient tile in the wide batches' form (r5, csrc/chain.h grouped_dw_kernel;
    AAE_DW_KSPLIT_ROWS=1 lifts the 256-row rule): each wave multiplies the whole 32 x 32 tile over a quarter of the rows,
    operands straight from memory into the matrix instructions' registers (tile rows 2 i / 2 i + 1 on lane i of the two
    16-row blocks), the four partial tiles added in wave order - against the reference's recorded losses, parameters and
    Adam moments at the SAME tolerances, incl. batches of fewer rows than waves have k-steps."""
    monkeypatch.setenv("AAE_DW_KSPLIT_ROWS", "1")
    test_step_matches_reference(name)


def test_saturated_logits_cost_the_same_on_both_forms_of_the_output_layer(monkeypatch):
    """F.binary_cross_entropy clamps its logarithms at -100, and the fp32 sigmoid rounds to exactly 1.0f from a logit of
    24 ln 2 = 16.64 on: such a cell of a zero target costs 100 and its s (1 - s) factor zeroes its gradient (aae.py:176-177,
    693-695) - the output-layer kernels keep both (csrc/gemm_f32.h bce_elem_t0, device_common.h kBceSatLogit).  Since r6 the
    CRITICAL launch takes the loss of a cell in parts - one logarithm per thread and tile, of the product of its cells' 1 + e
    (bce_elem_t0_parts) -, where a saturated cell, a target's exact form and the series for small e each leave the product
    alone.  dec.lin3 scaled until hundreds of logits saturate (and as many lie far below zero): the reconstruction loss of
    the first step - a function of the initial parameters alone - on the single launch (the per-cell form) and on the
    critical + deferred launches (the form in parts), to 1e-6; the saturated cells' 100s are in it.  Both are also held to
    the CPU oracle's loss of the same step (the reference's arithmetic, cut-off included) within the derived bound of the
    quantisation of its 1 - sigmoid(l) below the cut-off (golden_util.bce_quantisation_bound on the oracle's logits) plus
    TOL_LOSS relative: two forms that are wrong the same way do not pass."""
    from test_oracle_golden import build_oracle
    fx = Fixture("step_headline")
    params = fx.init_params()
    params["dec.lin3.weight"] = (params["dec.lin3.weight"] * np.float32(400.0)).astype(np.float32)
    ora = build_oracle(fx)
    ora.p.update({k: v.copy() for k, v in params.items()})
    ip, idx, val = fx.batch(0)
    want = ora.partial_fit(ip, idx, val, fx.z["step0.z_real"], fx.masks(0), None)[0]
    bound = bce_quantisation_bound(ora.last["logits"], ip, idx)
    losses, nsat = [], 0
    for split in (False, True):
        if split:
            monkeypatch.setenv("AAE_SPLIT_ANY", "1")
        m = make_model(fx)
        m.load_params(params)
        csr = csr_of(fx, m, 0)
        full = m.predict(csr, 0, csr.shape[0]).cpu().numpy()
        nsat = int((full == 1.0).sum())
        m.step(csr, 0, csr.shape[0], masks=fx.masks(0), z_real=fx.z["step0.z_real"])
        losses.append(np.asarray(m.losses(), dtype=np.float64))
    print("saturated scores of the batch:", nsat, "of", full.size, "| reconstruction loss, single launch | critical launch | oracle:",
          losses[0][0], losses[1][0], want, "| derived bound", bound)
    assert nsat >= 200, ("the case is meant to saturate", nsat)
    assert losses[0][0] > 100.0 * nsat / full.size, ("the saturated cells' 100s are missing from the loss", losses[0], nsat, full.size)
    np.testing.assert_allclose(losses[1][0], losses[0][0], rtol=1e-6)
    for got in (losses[0][0], losses[1][0]):
        assert abs(got - want) <= bound + TOL_LOSS * want, (got, want, bound)


def test_plain_autoencoder_matches_reference():
    """cfg.reserved[2] = 1: the reference's non-adversarial AutoEncoder (aae.py:221-458) - only the
    reconstruction step runs; fixture generated from the reference's AutoEncoder class."""
    fx = Fixture("step_ae_only")
    m = make_model(fx, ae_only=True)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        m.step(csr, 0, csr.shape[0], masks=fx.masks(s) + [None] * 8)
        got = m.losses()
        np.testing.assert_allclose(got[0], fx.z[f"step{s}.losses"][0], rtol=TOL_LOSS)
        check_state(fx, m, s, "ae_only")
    pcsr = csr_of(fx, m, 0, prefix="predict")
    np.testing.assert_allclose(m.predict(pcsr, 0, pcsr.shape[0]).cpu().numpy(), fx.z["predict.out"], atol=TOL_RECON)
    from aaerec._hip import AaeHipError
    with pytest.raises(AaeHipError):
        m.disc_step()


def test_first_layer_and_code_match_reference():
    fx = Fixture("step_nodrop_gauss")
    m = make_model(fx)
    csr = csr_of(fx, m, 0)
    z = m.ae_encode(csr, 0, csr.shape[0]).cpu().numpy()
    from aaerec import _hip
    a1 = m.tensor(_hip.T_ACT_A1)[:csr.shape[0]].cpu().numpy()
    np.testing.assert_allclose(a1, fx.z["step0.act.enc_a1_ae"], atol=1e-6)
    np.testing.assert_allclose(z, fx.z["step0.act.enc_z_ae"], atol=1e-6)


def test_split_phase_equals_fused_step():
    """aae_ae_encode / decode_backward / encoder_backward / disc_gen with the concatenation done
    by the caller must give the same result as aae_step."""
    fx = Fixture("step_cond_concat")
    m = make_model(fx)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = torch.as_tensor(fx.cond_inputs(s)[0], device=m.device)
        z = m.ae_encode(csr, 0, B, masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
        dzc = m.ae_decode_backward(torch.cat([z, cond], 1))
        m.ae_encoder_backward(dzc[:, :fx.cfg["c"]])
        m.disc_gen()
        np.testing.assert_allclose(m.losses(), fx.z[f"step{s}.losses"], rtol=TOL_LOSS, atol=1e-6)
        check_state(fx, m, s, "split")


# ---- calls out of order: each is refused by a host-side check, with its text, and the handle carries on ----------------
# A sequence below is one step through its phase calls; at(point) runs between them.  The handle under test gets a refused
# call at the case's points, its twin none.
def _seq_whole(fx, m, s, at):
    csr = csr_of(fx, m, s)
    at("open")
    m.step(csr, 0, csr.shape[0], masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])


def _seq_split(fx, m, s, at):
    csr = csr_of(fx, m, s)
    cond = fx.cond_inputs(s)
    at("open")
    z = m.ae_encode(csr, 0, csr.shape[0], masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
    at("encoded")
    dzc = m.ae_decode_backward(torch.cat([z, torch.as_tensor(cond[0], device=m.device)], 1) if cond else z)
    at("decoded")
    m.ae_encoder_backward(dzc[:, :fx.cfg["c"]])
    at("encoder_done")
    m.disc_step()
    m.gen_step()


def _seq_cut(fx, m, s, at):
    csr = csr_of(fx, m, s)
    at("open")
    m.ae_forward(csr, 0, csr.shape[0], masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
    m.output_layer_step()
    at("output_done")
    m.ae_backward()
    at("backward_done")
    m.disc_gen()


def _seq_vae(fx, m, s, at):
    csr = csr_of(fx, m, s)
    at("open")
    z = m.vae_encode(csr, 0, csr.shape[0], eps=fx.z[f"step{s}.eps"], train=True)
    at("encoded")
    dzc = m.vae_decode_backward(z)
    at("decoded")
    m.vae_encoder_backward(dzc[:, :fx.cfg["c"]])


def _zeros(m, cols):
    return torch.zeros(m.max_batch, cols, device=m.device)


def _step_on_an_external_first_layer(fx, m, s):
    m.set_first_layer_external(True)
    try:
        m.step(csr_of(fx, m, s), 0, fx.cfg["B"])
    finally:
        m.set_first_layer_external(False)


# name: (fixture, sequence, the points of a step at which the call is made, the call (fx, m, s), the text it is refused with
#        [, the steps it is made in: both of the two unless given])
BAD_CALLS = {
    "disc_step_before_the_ae_phases": ("step_nodrop_gauss", _seq_split, ("open", "encoded", "decoded"),
                                       lambda fx, m, s: m.disc_gen(), "aae_disc_step before the ae phases of the step"),
    "gen_step_before_disc_step": ("step_nodrop_gauss", _seq_split, ("open", "encoder_done"),
                                  lambda fx, m, s: m.gen_step(), "aae_gen_step before aae_disc_step"),
    "ae_decode_backward_without_ae_encode": ("step_cond_concat", _seq_split, ("open", "decoded"),
                                             lambda fx, m, s: m.ae_decode_backward(_zeros(m, fx.cfg["c"] + fx.cfg["cond_inc"])),
                                             "aae_ae_decode_backward without aae_ae_encode"),
    "ae_encoder_backward_without_ae_decode_backward": ("step_cond_concat", _seq_split, ("open", "encoded"),
                                                       lambda fx, m, s: m.ae_encoder_backward(_zeros(m, fx.cfg["c"])),
                                                       "aae_ae_encoder_backward without aae_ae_decode_backward"),
    "output_layer_step_without_ae_forward": ("step_nodrop_gauss", _seq_cut, ("open", "output_done"),
                                             lambda fx, m, s: m.output_layer_step(),
                                             "aae_output_layer_step(batch = NULL) without aae_ae_forward"),
    "ae_backward_without_ae_forward": ("step_nodrop_gauss", _seq_cut, ("open", "backward_done"),
                                       lambda fx, m, s: m.ae_backward(), "aae_ae_backward without aae_ae_forward"),
    "vae_decode_backward_without_vae_encode": ("step_vae", _seq_vae, ("open", "decoded"),
                                               lambda fx, m, s: m.vae_decode_backward(_zeros(m, fx.cfg["c"])),
                                               "aae_vae_decode_backward without aae_vae_encode(train)"),
    "vae_encoder_backward_without_vae_decode_backward": ("step_vae", _seq_vae, ("open", "encoded"),
                                                         lambda fx, m, s: m.vae_encoder_backward(_zeros(m, fx.cfg["c"])),
                                                         "aae_vae_encoder_backward without aae_vae_decode_backward"),
    # (only a handle that never saw a batch has none running: the first step's opening)
    "first_layer_forward_without_a_running_batch": ("step_nodrop_gauss", _seq_whole, ("open",),
                                                    lambda fx, m, s: m.first_layer_forward(),
                                                    "aae_first_layer_forward(batch = NULL) without a running batch", (0,)),
    "step_on_an_external_first_layer": ("step_nodrop_gauss", _seq_whole, ("open",), _step_on_an_external_first_layer,
                                        "aae_step: the first layer is external (aae_set_first_layer_external): drive the phases"),
    "more_rows_than_max_batch": ("step_nodrop_gauss", _seq_whole, ("open",),
                                 lambda fx, m, s: m.step(csr_of(fx, m, s), 0, fx.cfg["B"] + 1), "batch n_rows outside [1, max_batch]"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_abi_rejects_bad_calls(name, monkeypatch):
    """Every phase call out of order is refused with its text by a host-side check - also in the middle of a split step, which
    then continues - and leaves nothing behind: after two steps the handle holds the parameter and loss bytes of a twin that
    never saw a refusal.  (AAE_SPLIT_ANY: the split form's loss is reproducible at the fixtures' sizes.)"""
    import re
    from aaerec._hip import AaeHipError, HipAAE
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    fixture, sequence, points, call, text = BAD_CALLS[name][:5]
    steps = BAD_CALLS[name][5] if len(BAD_CALLS[name]) > 5 else (0, 1)
    fx = Fixture(fixture)

    def new_handle():
        if fixture != "step_vae":
            return make_model(fx)
        c = fx.cfg
        m = HipAAE(c["N"], c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=c["B"], rng_mode="inject", gen_lr=c["gen_lr"],
                   reg_lr=c["gen_lr"], dropout=(0.0, 0.0), vae=True)
        m.load_params(_vae_params(fx, "init"))
        return m

    m, twin = new_handle(), new_handle()
    refused = []
    for s in range(2):
        def at(point):
            if point not in points or s not in steps:
                return
            with pytest.raises(AaeHipError, match=re.escape(text)):
                call(fx, m, s)
            refused.append((s, point))
        sequence(fx, m, s, at)
        sequence(fx, twin, s, lambda point: None)
        got, want = np.array(m.losses(), dtype=np.float32), np.array(twin.losses(), dtype=np.float32)
        if fixture == "step_vae":
            # The KL sum is not reproducible from run to run on any build: chain.h's COP_REPARAM_BWD adds one partial per wave
            # with a float atomic, in the order the waves arrive (two runs of ONE library differ in it, tools/step_bits.py).
            # Every partial is a fixed-order sum of terms >= 0, so two orders of adding W of them differ by at most
            # 2 (W - 1) 2^-24 of the sum; W = 16 waves per 16-row workgroup.  Its gradient does not pass through the sum: the
            # parameters and the reconstruction loss are held to their bytes like everywhere else.
            waves = 16 * ((fx.cfg["B"] + 15) // 16)
            assert abs(float(got[1]) - float(want[1])) <= 2 * (waves - 1) * 2.0 ** -24 * max(got[1], want[1]), (name, s, got, want)
            got[1] = want[1] = 0.0
        assert got.tobytes() == want.tobytes(), (name, s, got, want)
    assert len(refused) == len(steps) * len(points)
    got, want = m.state_dict(), twin.state_dict()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (name, k)


@pytest.mark.parametrize("prefetch", [False, True, "early"])
def test_deferred_adam_matches_eager_oracle_over_many_sparse_steps(prefetch, monkeypatch):
    """The lazy W1T optimiser (rows of absent items are updated when next read, replay truncated
    after 128 steps) against the oracle's eager dense Adam: 260 steps over a 900-item vocabulary
    where most items are seen only a few times, so gaps of 0..250 steps all occur.
    prefetch: every batch is named one step ahead (aae_prefetch_batch: its unique-item list and catch-up are built on
    the side stream while the step before it runs) - except that every 7th hint is left out and every 11th names a
    batch that does not come (both must fall back to the step's own catch-up).
    'early' (late r4): the same with the early form of the prefetch forced onto this batch size (AAE_EARLY_ANY; the library
    takes it for batches beyond one fused launch): the side stream's mark rides on the LAST launch of the step before, the
    catch-up runs beside the step's opening gather on the optimiser-table entry written a step early and the step number from
    the host - and falls back to the mark on the gather after every missing or wrong hint."""
    if prefetch == "early":
        monkeypatch.setenv("AAE_EARLY_ANY", "1")
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    rng = np.random.default_rng(5)
    N, h, c, B, steps = 900, 12, 6, 6, 260
    params = init_params(N, h, c, seed=3)
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.0, 0.0))
    dev = HipAAE(N, h, c, max_batch=B, rng_mode="inject", **kw)
    dev.load_params(params)
    ora = O.OracleAAE(params, **kw)
    # skewed popularity: items 0..19 in most batches, the tail rarely
    p = 1.0 / np.arange(1, N + 1) ** 1.3
    p /= p.sum()
    batches = []
    for s in range(steps):
        rows = [np.sort(rng.choice(N, size=int(rng.integers(1, 6)), replace=False, p=p)) for _ in range(B)]
        ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        val = np.ones(len(idx), dtype=np.float32)
        zr = rng.standard_normal((B, c)).astype(np.float32)
        batches.append((ip, idx, val, zr, DeviceCSR.from_arrays(ip, idx, val, N, dev.device)))
    for s, (ip, idx, val, zr, csr) in enumerate(batches):
        if prefetch and s + 1 < steps and s % 7 != 3:
            dev.prefetch(batches[(s + 5) % steps if s % 11 == 5 else s + 1][4], 0, B)
        dev.step(csr, 0, B, z_real=zr)
        want = ora.partial_fit(ip, idx, val, zr)
        if s % 20 == 0 or s == steps - 1:
            np.testing.assert_allclose(dev.losses(), want, rtol=2e-4, atol=1e-6, err_msg=f"step {s}")
    got = dev.state_dict()
    for k, w in ora.p.items():
        np.testing.assert_allclose(got[k], w, atol=3e-5, rtol=0, err_msg=k)
    st = dev.adam_state("enc")
    np.testing.assert_allclose(st["lin1.weight"][0], ora.opt_enc.m["enc.lin1.weight"], atol=1e-8, rtol=1e-3)
    np.testing.assert_allclose(st["lin1.weight"][1], ora.opt_enc.v["enc.lin1.weight"], atol=1e-12, rtol=1e-3)
    st = dev.adam_state("gen")
    np.testing.assert_allclose(st["lin1.weight"][1], ora.opt_gen.v["enc.lin1.weight"], atol=1e-12, rtol=1e-3)
    assert st["step"] == steps


def test_a_refilled_batch_buffer_at_the_same_address_is_not_taken_for_the_batch_named_ahead():
    """ABI 3: a batch named with aae_prefetch_batch is matched by pointers, row window AND the caller's
    content id (aae_batch.generation), not by the pointers alone.  A caller that recycles ONE device buffer: it names the
    buffer as the next batch while it still holds this step's documents, then refills it in place (DeviceCSR.touch(): new
    generation) and runs the next step on it.  With pointer identity (r1-r4) that step took the item list built from the
    OLD content - first-layer rows missing from it got no update; now it must do its own list, and 40 such steps equal
    the oracle's.  An untouched buffer named ahead still matches (the same loop with honest hints is
    test_deferred_adam_matches_eager_oracle_over_many_sparse_steps)."""
    import torch
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    rng = np.random.default_rng(11)
    N, h, c, B, steps = 700, 12, 6, 8, 40
    params = init_params(N, h, c, seed=4)
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.0, 0.0))
    dev = HipAAE(N, h, c, max_batch=B, rng_mode="inject", **kw)
    dev.load_params(params)
    ora = O.OracleAAE(params, **kw)
    per_row = 5
    buf = DeviceCSR.from_arrays(np.arange(0, (B + 1) * per_row, per_row), np.zeros(B * per_row, dtype=np.int32),
                                np.ones(B * per_row, dtype=np.float32), N, dev.device)
    ptrs = (buf.indptr.data_ptr(), buf.indices.data_ptr(), buf.values.data_ptr())
    gens = set()
    for s in range(steps):
        rows = [np.sort(rng.choice(N, size=per_row, replace=False)) for _ in range(B)]
        idx = np.concatenate(rows).astype(np.int32)
        ip = np.arange(0, (B + 1) * per_row, per_row).astype(np.int64)
        zr = rng.standard_normal((B, c)).astype(np.float32)
        torch.cuda.synchronize()                       # (the work built from the old content has run: the refill races with nothing)
        buf.indices.copy_(torch.from_numpy(idx))       # the recycled buffer: same tensors, same addresses, new documents
        buf.touch()
        gens.add(buf.generation)
        assert ptrs == (buf.indptr.data_ptr(), buf.indices.data_ptr(), buf.values.data_ptr())
        dev.prefetch(buf, 0, B)                        # "the next batch" = this buffer, named while it holds THIS step's rows:
        dev.step(buf, 0, B, z_real=zr)                 # its item list is built beside this step, for the step after it
        want = ora.partial_fit(ip, idx, np.ones(len(idx), dtype=np.float32), zr)
        if s % 10 == 0 or s == steps - 1:
            np.testing.assert_allclose(dev.losses(), want, rtol=2e-4, atol=1e-6, err_msg=f"step {s}")
    assert len(gens) == steps
    got = dev.state_dict()
    for k, w in ora.p.items():
        np.testing.assert_allclose(got[k], w, atol=3e-5, rtol=0, err_msg=k)
    st = dev.adam_state("gen")
    np.testing.assert_allclose(st["lin1.weight"][1], ora.opt_gen.v["enc.lin1.weight"], atol=1e-12, rtol=1e-3)


@pytest.mark.parametrize("N,B", [(1500, 320), (9000, 100)])
def test_item_workgroups_sized_by_the_devices_count_leave_every_bit_alone(N, B, monkeypatch):
    """r5: the first-layer item workgroups of the weight-gradient launches are sized by the distinct-item count a workgroup of
    an EARLIER launch stored into host-visible memory (abi_chains.h) - a number the host reads without waiting, so it
    depends on timing.  The result must not: every item's sum is one workgroup's (or wave's) work in an order fixed by the
    batch, whatever the grid.  Six steps with the feedback (the launches shrink after the first step) and six with one
    workgroup per possible item (AAE_NO_ITEM_COUNT=1): every parameter and both moments of enc.lin1 bit for bit - on the wide
    batches' workgroup form (320 rows over 1 500 items) and on the hybrid form of a 100-row batch."""
    import torch
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle.dense_torch_port import init_params
    from tools.synth import throughput_corpus
    h, c, steps = 200, 50, 6
    X = throughput_corpus(steps * B, N, median_len=14, max_len=70, seed=9)
    params = init_params(N, h, c, seed=3)
    outs = []
    for no_count in (False, True):
        if no_count:
            monkeypatch.setenv("AAE_NO_ITEM_COUNT", "1")
        else:
            monkeypatch.delenv("AAE_NO_ITEM_COUNT", raising=False)
        m = HipAAE(N, h, c, max_batch=B, max_nnz=B * 80, rng_mode="device", seed=5, dropout=(0.2, 0.2))
        m.load_params(params)
        csr = DeviceCSR(X, m.device)
        for s in range(steps):
            m.step(csr, s * B, B)
        torch.cuda.synchronize()
        outs.append((m.state_dict(), m.adam_state("enc"), m.adam_state("gen")))
        m.close()
    (p0, e0, g0), (p1, e1, g1) = outs
    for k in p0:
        np.testing.assert_array_equal(p0[k], p1[k], err_msg=k)
    for a, b in ((e0, e1), (g0, g1)):
        np.testing.assert_array_equal(a["lin1.weight"][0], b["lin1.weight"][0])
        np.testing.assert_array_equal(a["lin1.weight"][1], b["lin1.weight"][1])


@pytest.mark.parametrize("N,h,c,B", [(5000, 200, 50, 100), (3001, 100, 50, 37), (4096, 200, 50, 104)])
def test_fused_decoder_equals_unfused_path_at_headline_width(N, h, c, B):
    """The persistent fused decoder kernel (dec_fused.h, used for B <= ~104) against the
    three-kernel path (GEMM + BCE epilogue, split-K dA2, dV3 GEMM + Adam epilogue) that the
    golden fixtures also pin, at the headline layer widths the small fixtures do not reach."""
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle.dense_torch_port import init_params
    from tools.synth import throughput_corpus
    X = throughput_corpus(3 * B, N, median_len=12, max_len=60, seed=3)
    params = init_params(N, h, c, seed=1)
    rng = np.random.default_rng(0)
    models = []
    for unfused in (False, True):
        m = HipAAE(N, h, c, max_batch=B, rng_mode="inject", dropout=(0.2, 0.2), unfused_decoder=unfused)
        m.load_params(params)
        models.append(m)
    csr = [DeviceCSR(X, m.device) for m in models]
    for s in range(3):
        masks = [(rng.random((B, h)) > 0.2).astype(np.uint8) for _ in range(12)]
        zr = rng.standard_normal((B, c)).astype(np.float32)
        out = []
        for m, cs in zip(models, csr):
            m.step(cs, s * B, B, masks=masks, z_real=zr)
            out.append(m.losses())
        np.testing.assert_allclose(out[0], out[1], rtol=2e-6, atol=1e-7)
    a, b = models[0].state_dict(), models[1].state_dict()
    for k in a:
        np.testing.assert_allclose(a[k], b[k], atol=2e-6, rtol=0, err_msg=k)
    for which in ("dec", "enc"):
        sa, sb = models[0].adam_state(which), models[1].adam_state(which)
        for k in ("lin3.weight", "lin1.weight"):
            np.testing.assert_allclose(sa[k][0], sb[k][0], atol=1e-9, rtol=1e-4)
            np.testing.assert_allclose(sa[k][1], sb[k][1], atol=1e-13, rtol=1e-4)


class _SoloDist:
    """torch.distributed stand-in for one rank: the exchange points become no-ops."""
    class ReduceOp:
        SUM = 0

    def get_world_size(self, group=None):
        return 1

    def get_rank(self, group=None):
        return 0

    def all_reduce(self, t, op=None, group=None, async_op=False):
        return None

    class _Done:
        def wait(self):
            return None

    def reduce_scatter_tensor(self, out, inp, op=None, group=None, async_op=False):
        out.copy_(inp.reshape(out.shape))
        return self._Done()

    def all_gather_into_tensor(self, out, inp, group=None, async_op=False):
        out.copy_(inp.reshape(out.shape))
        return self._Done()


@pytest.mark.parametrize("shard", [False, "force"])
@pytest.mark.parametrize("name", ["step_masks", "step_cond_concat", "step_sgd", "step_wide"])
def test_export_mode_through_parallel_wrapper_matches_reference(name, shard):
    """grad_mode='export' (gradients materialised, aae_apply_updates after the exchange point) driven
    by aaerec.parallel.DataParallelAAE must reproduce the same fixtures as the fused-optimiser path."""
    from aaerec.parallel import DataParallelAAE
    fx = Fixture(name)
    m = make_model(fx, grad_mode="export", dp_world=1)
    dp = DataParallelAAE(m, _SoloDist(), shard_decoder=shard)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = fx.cond_inputs(s)
        cond_fn = None
        if cond:
            ct = torch.as_tensor(cond[0], device=m.device)
            cond_fn = lambda z, ct=ct: (torch.cat([z, ct], 1), lambda dzc: dzc[:, :fx.cfg["c"]].contiguous())  # noqa: E731
        dp.step(csr, 0, B, global_rows=B, cond_fn=cond_fn, masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
        dp.wait_pending()
        np.testing.assert_allclose(m.losses(), fx.z[f"step{s}.losses"], rtol=TOL_LOSS, atol=1e-6)
        if fx.has_state(s):
            check_state(fx, m, s, name)


@pytest.mark.parametrize("name", ["step_nodrop_gauss", "step_masks"])
def test_torch_custom_ops_replay_fixture(name):
    """The same replay through torch.ops.aaerec.* (aaerec/ops.py), the torch-facing surface over the C ABI."""
    from aaerec import ops
    fx = Fixture(name)
    m = make_model(fx)
    mid = ops.register_model(m)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        masks = [None if k is None else torch.as_tensor(np.ascontiguousarray(k, dtype=np.uint8), device=m.device)
                 for k in (fx.masks(s) or [])]
        z_real = torch.as_tensor(fx.z[f"step{s}.z_real"], device=m.device)
        losses = torch.ops.aaerec.step(mid, csr.indptr, csr.indices, csr.values, None, 0, B, csr.nnz_per_row_max,
                                       None, masks, z_real)
        np.testing.assert_allclose(losses.cpu().numpy(), fx.z[f"step{s}.losses"], rtol=TOL_LOSS, atol=1e-6)
        if fx.has_state(s):
            check_state(fx, m, s, name)
    pcsr = csr_of(fx, m, 0, prefix="predict")
    n = pcsr.shape[0]
    out = torch.ops.aaerec.predict(mid, pcsr.indptr, pcsr.indices, pcsr.values, 0, n, pcsr.nnz_per_row_max, None)
    np.testing.assert_allclose(out.cpu().numpy(), fx.z["predict.out"], atol=TOL_RECON)
    ids, val = torch.ops.aaerec.predict_topk(mid, pcsr.indptr, pcsr.indices, pcsr.values, 0, n, pcsr.nnz_per_row_max,
                                             None, 5, True)
    ids2, val2 = m.predict_topk(pcsr, 0, n, 5)
    assert torch.equal(ids, ids2) and torch.equal(val, val2)
    z = torch.ops.aaerec.encode(mid, pcsr.indptr, pcsr.indices, pcsr.values, 0, n, pcsr.nnz_per_row_max)
    assert z.shape == (n, fx.cfg["c"])
    del m
    with pytest.raises(RuntimeError):
        torch.ops.aaerec.encode(mid, pcsr.indptr, pcsr.indices, pcsr.values, 0, n, pcsr.nnz_per_row_max)


@pytest.mark.parametrize("name", ["step_decoding", "step_decoding_trainable"])
def test_decoder_step_matches_reference(name):
    """aae_decoder_step (DecodingRecommender.partial_fit, aae.py:489-517) replayed against the reference's
    fixtures; the condition side (host plugins in production) is played by the oracle's stand-ins, which also
    check the dL/dzin the kernel hands back for trainable conditions."""
    from aaerec._hip import HipAAE
    from test_oracle_golden import build_decoding_oracle
    fx = Fixture(name)
    c = fx.cfg
    orc = build_decoding_oracle(fx)
    m = HipAAE(c["N"], c["h"], c["n_code"], cond_inc=0, max_batch=c["B"], rng_mode="inject", gen_lr=c["gen_lr"],
               reg_lr=c["gen_lr"], dropout=tuple(c["dropout"]))
    m.load_params(fx.init_params())
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = fx.cond_inputs(s)
        zin = orc.inputs(cond)                                   # with the embeddings as they are before this step
        dz = m.decoder_step(csr, 0, B, torch.as_tensor(zin, device=m.device), masks=fx.masks(s))
        loss = orc.partial_fit(cond, *fx.batch(s), fx.masks(s))  # advances the oracle's conditions as well
        np.testing.assert_allclose(m.losses()[0], fx.z[f"step{s}.losses"][0], rtol=TOL_LOSS, atol=1e-6)
        np.testing.assert_allclose(loss, fx.z[f"step{s}.losses"][0], rtol=TOL_LOSS, atol=1e-6)
        np.testing.assert_allclose(dz.cpu().numpy(), orc.last_dzin, rtol=2e-4, atol=2e-9, err_msg=f"{name} dzin {s}")
        got = m.state_dict()
        for k in ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"):
            np.testing.assert_allclose(got["dec." + k], fx.z[f"step{s}.dec.{k}"], atol=TOL_PARAM, rtol=0,
                                       err_msg=f"{name} step {s} {k}")
        st = m.adam_state("dec")
        for (tag, k), (em, ev, et) in fx.expected_adam(s).items():
            gm, gv = st[k.split(".", 1)[1]]
            assert st["step"] == et
            np.testing.assert_allclose(gm, em, atol=2e-9, rtol=1e-4)
            np.testing.assert_allclose(gv, ev, atol=1e-12, rtol=2e-4)
    zp = orc.inputs(fx.cond_inputs(0, prefix="predict"), train=False)
    out = m.decode(torch.as_tensor(zp, device=m.device)).cpu().numpy()
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)


def test_denoising_autoencoder_step_matches_reference():
    """DenoisingAutoEncoder (dae.py:144-314, corrupt='zeros'): the plain autoencoder step on the thinned bag -
    entries the reference's zeros_noise removed carry value 0 (they gather nothing and are zero targets)."""
    from aaerec._hip import DeviceCSR
    fx = Fixture("step_dae")
    m = make_model(fx, ae_only=True)
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        csr = DeviceCSR.from_arrays(ip, idx, val * fx.z[f"step{s}.keep"], fx.cfg["N"], m.device)
        m.step(csr, 0, csr.shape[0], masks=fx.masks(s) + [None] * 8)
        np.testing.assert_allclose(m.losses()[0], fx.z[f"step{s}.losses"][0], rtol=TOL_LOSS)
        check_state(fx, m, s, "dae")
    pcsr = csr_of(fx, m, 0, prefix="predict")
    np.testing.assert_allclose(m.predict(pcsr, 0, pcsr.shape[0]).cpu().numpy(), fx.z["predict.out"], atol=TOL_RECON)


def _vae_params(fx, prefix):
    g = lambda n, t: fx.z[f"{prefix}.{n}.{t}"]                                      # noqa: E731
    return {"enc.lin1.weight": g("fc1", "weight"), "enc.lin1.bias": g("fc1", "bias"),
            "enc.lin3.weight": np.vstack([g("fc21", "weight"), g("fc22", "weight")]),
            "enc.lin3.bias": np.concatenate([g("fc21", "bias"), g("fc22", "bias")]),
            "dec.lin1.weight": g("fc3", "weight"), "dec.lin1.bias": g("fc3", "bias"),
            "dec.lin3.weight": g("fc4", "weight"), "dec.lin3.bias": g("fc4", "bias")}


@pytest.mark.parametrize("name", ["step_vae", "step_vae_cond"])
def test_vae_step_matches_reference(name):
    """aae_vae_step / aae_vae_predict (VAE, reference vae.py:47-266) with the recorded eps of reparametrize():
    loss = (mean BCE + KL sum) / B as the reference logs it, all five Linears and their Adam moments after every
    step.  ENC_W3 holds [fc21; fc22]."""
    from aaerec._hip import HipAAE
    fx = Fixture(name)
    c = fx.cfg
    m = HipAAE(c["N"], c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=c["B"], rng_mode="inject", gen_lr=c["gen_lr"],
               reg_lr=c["gen_lr"], dropout=(0.0, 0.0), vae=True)
    m.load_params(_vae_params(fx, "init"))
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = fx.cond_inputs(s)
        cond_t = torch.as_tensor(cond[0], device=m.device) if cond else None
        m.vae_step(csr, 0, B, cond=cond_t, eps=fx.z[f"step{s}.eps"])
        l = m.losses()
        np.testing.assert_allclose((l[0] + l[1]) / B, fx.z[f"step{s}.losses"][0], rtol=2e-5)
        got, want = m.state_dict(), _vae_params(fx, f"step{s}")
        for k, w in want.items():
            np.testing.assert_allclose(got[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k}")
        enc, dec = m.adam_state("enc"), m.adam_state("dec")
        for st, key, names in ((enc, "lin1", ("fc1",)), (enc, "lin3", ("fc21", "fc22")), (dec, "lin1", ("fc3",)),
                               (dec, "lin3", ("fc4",))):
            for t, idx in (("weight", 0), ("bias", 1)):
                em = np.concatenate([fx.z[f"step{s}.A.{n}.{t}.m"] for n in names])
                ev = np.concatenate([fx.z[f"step{s}.A.{n}.{t}.v"] for n in names])
                gm, gv = st[f"{key}.{t}"]
                np.testing.assert_allclose(gm, em, atol=2e-8, rtol=2e-4, err_msg=f"{name} {s} m {key}.{t}")
                np.testing.assert_allclose(gv, ev, atol=1e-12, rtol=2e-4, err_msg=f"{name} {s} v {key}.{t}")
            assert st["step"] == float(fx.z[f"step{s}.A.{names[0]}.weight.t"])
    pcsr = csr_of(fx, m, 0, prefix="predict")
    pc = fx.cond_inputs(0, prefix="predict")
    pc_t = torch.as_tensor(pc[0], device=m.device) if pc else None
    out = m.vae_predict(pcsr, 0, pcsr.shape[0], cond=pc_t, eps=fx.z["predict.eps"]).cpu().numpy()
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)
    from aaerec._hip import AaeHipError
    with pytest.raises(AaeHipError):
        m.vae_step(csr, 0, B, cond=cond_t, eps=None)        # inject mode needs eps


@pytest.mark.parametrize("N,h,c,B,inc", [(3000, 200, 50, 100, 0), (2500, 100, 50, 37, 30), (2000, 207, 120, 64, 0)])
def test_layer_chain_equals_per_layer_path_at_headline_width(N, h, c, B, inc):
    """The row-blocked layer-chain kernel (chain.h: every hidden layer of the three phases, 13 column blocks at
    h = 200) against the per-layer GEMM path (AAE_NO_CHAIN=1 at creation; the path the small golden fixtures were
    first pinned on), at widths the fixtures do not reach, with dropout masks, a condition block and a ragged
    last row block."""
    import os
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle.dense_torch_port import init_params
    from tools.synth import throughput_corpus
    X = throughput_corpus(3 * B, N, median_len=12, max_len=60, seed=4)
    params = init_params(N, h, c, seed=2, cond_inc=inc) if inc else init_params(N, h, c, seed=2)
    rng = np.random.default_rng(1)
    models = []
    for no_chain in (False, True):
        if no_chain:
            os.environ["AAE_NO_CHAIN"] = "1"
        try:
            m = HipAAE(N, h, c, cond_inc=inc, max_batch=B, rng_mode="inject", dropout=(0.2, 0.2), gen_lr=2e-3,
                       reg_lr=1e-3)
        finally:
            os.environ.pop("AAE_NO_CHAIN", None)
        m.load_params(params)
        models.append(m)
    csr = [DeviceCSR(X, m.device) for m in models]
    for s in range(3):
        masks = [(rng.random((B, h)) > 0.2).astype(np.uint8) for _ in range(12)]
        zr = rng.standard_normal((B, c)).astype(np.float32)
        cond = torch.as_tensor(rng.standard_normal((B, inc)).astype(np.float32) * 0.3) if inc else None
        out = []
        for m, cs in zip(models, csr):
            m.step(cs, s * B, B, masks=masks, z_real=zr, cond=None if cond is None else cond.to(m.device))
            out.append(m.losses())
        np.testing.assert_allclose(out[0], out[1], rtol=3e-6, atol=1e-7, err_msg=f"step {s}")
    a, b = models[0].state_dict(), models[1].state_dict()
    for k in a:
        # (fp32 summation order differs between the paths - the 4-row chain kernel splits a layer's k over 4 to 16 waves -
        # and Adam turns a difference of a ~1e-8 gradient into a few 1e-6 of parameter: see tests/test_oracle_golden.py)
        np.testing.assert_allclose(a[k], b[k], atol=5e-6, rtol=0, err_msg=k)
    for which in ("enc", "gen", "dec", "disc"):
        sa, sb = models[0].adam_state(which), models[1].adam_state(which)
        for k in ("lin2.weight", "lin3.weight", "lin1.bias"):
            np.testing.assert_allclose(sa[k][0], sb[k][0], atol=2e-9, rtol=2e-4, err_msg=f"{which} m {k}")
            np.testing.assert_allclose(sa[k][1], sb[k][1], atol=1e-13, rtol=2e-4, err_msg=f"{which} v {k}")


def test_w1_import_all_peers_in_one_launch_equals_the_per_peer_launches():
    """Data parallel, world > 1: aae_w1_import folds every peer's packed first-layer rows (and the small encoder
    layers behind them) in one launch each, in rank order; the result must be BITWISE what consecutive per-peer
    launches give (AAE_W1_SERIAL=1), or replicas would drift apart.  Peers share some items and not others."""
    import os
    from aaerec._hip import HipAAE
    from oracle.dense_torch_port import init_params
    W, N, h, c, B, cap = 4, 1500, 40, 10, 16, 96
    params = init_params(N, h, c, seed=5)
    rng = np.random.default_rng(9)
    models = []
    for _ in range(2):
        m = HipAAE(N, h, c, max_batch=B, rng_mode="inject", grad_mode="export", dp_world=W, w1_cap=cap)
        m.load_params(params)
        models.append(m)
    for m in models:
        pk0 = m.w1_export()                            # allocates the packet: layout = header | rows | small layers
    n, hw = pk0.numel(), models[0]._w1_hdr
    host = np.zeros((W, n), dtype=np.float32)
    common = rng.choice(N, size=20, replace=False)
    for p in range(W):
        own = rng.choice(N, size=int(rng.integers(30, 60)), replace=False)
        items = np.unique(np.concatenate([common[: 5 + 4 * p], own]))[:cap]
        hdr = np.zeros(hw, dtype=np.int32)
        hdr[0] = len(items)
        hdr[1:1 + len(items)] = items
        host[p, :hw] = hdr.view(np.float32)
        host[p, hw:hw + len(items) * h] = rng.standard_normal(len(items) * h).astype(np.float32) * 1e-3
        host[p, hw + cap * h:] = rng.standard_normal(n - hw - cap * h).astype(np.float32) * 1e-3
    out = []
    for m, serial in zip(models, (False, True)):
        if serial:
            os.environ["AAE_W1_SERIAL"] = "1"
        try:
            m.w1_import(torch.as_tensor(host, device=m.device).reshape(-1), W, 0)
            st = m.adam_state("enc")
        finally:
            os.environ.pop("AAE_W1_SERIAL", None)
        out.append(st)
    for k in ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"):
        for j in (0, 1):
            assert np.array_equal(out[0][k][j], out[1][k][j]), k
    # and the sums are what they should be: first moment = 0.1 * summed gradient (fresh optimiser state)
    dense = np.zeros((N, h), dtype=np.float64)
    for p in range(W):
        cnt = int(host[p, :1].view(np.int32)[0])
        ids = host[p, 1:1 + cnt].view(np.int32)
        dense[ids] += host[p, hw:hw + cnt * h].reshape(cnt, h)
    np.testing.assert_allclose(out[0]["lin1.weight"][0].T, 0.1 * dense, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("N,B,h,c", [(20, 1, 8, 4), (33, 2, 8, 4), (64, 3, 16, 5), (31, 17, 12, 3)])
def test_tiny_shapes_match_oracle(N, B, h, c):
    """Degenerate sizes: one document, a vocabulary smaller than one 32-item decoder tile, a batch that ends one
    row into a second 16-row block - the kernels' clamped / masked lanes against the oracle (computed here)."""
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    rng = np.random.default_rng(N * 100 + B)
    params = init_params(N, h, c, seed=N)
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.2, 0.2))
    dev = HipAAE(N, h, c, max_batch=B, rng_mode="inject", **kw)
    dev.load_params(params)
    ora = O.OracleAAE(params, **kw)
    for s in range(3):
        rows = [np.sort(rng.choice(N, size=int(rng.integers(1, min(N, 6))), replace=False)) for _ in range(B)]
        ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        val = np.ones(len(idx), dtype=np.float32)
        masks = [(rng.random((B, h)) > 0.2).astype(np.uint8) for _ in range(12)]
        zr = rng.standard_normal((B, c)).astype(np.float32)
        dev.step(DeviceCSR.from_arrays(ip, idx, val, N, dev.device), 0, B, masks=masks, z_real=zr)
        want = ora.partial_fit(ip, idx, val, zr, masks)
        np.testing.assert_allclose(dev.losses(), want, rtol=2e-5, atol=1e-6, err_msg=f"step {s}")
    got = dev.state_dict()
    for k, w in ora.p.items():
        np.testing.assert_allclose(got[k], w, atol=1e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("rows,width,vocab,dim,mean", [(100, 9, 300, 200, False), (37, 4, 50, 33, True),
                                                       (64, 1, 40, 64, False), (3, 70, 9, 256, True)])
def test_categorical_condition_kernels_match_oracle(rows, width, vocab, dim, mean, sparse):
    """aae_cat_encode / aae_cat_update against the oracle's CategoricalEmbedding (itself pinned to the reference's
    CategoricalCondition fixtures): wide tables, values shared by many documents and repeated inside one list,
    padding in the middle of a list, a strided output block; five optimiser steps."""
    from aaerec import _hip
    from oracle import aae_oracle as O
    rng = np.random.default_rng(rows * 7 + width)
    table0 = (rng.standard_normal((vocab, dim)) * 0.1).astype(np.float32)
    table0[0] = 0
    ora = O.CategoricalEmbedding(table0, lr=3e-3, reduce="mean" if mean else "sum", sparse=sparse)
    dev = torch.device("cuda:0")
    table = torch.from_numpy(table0.copy()).to(dev)
    m, v = torch.zeros_like(table), torch.zeros_like(table)
    scratch = None if sparse else torch.zeros_like(table)
    off = 5                                                      # the block is a column slice of a wider buffer
    for step in range(1, 6):
        idx = rng.integers(0, vocab, size=(rows, width))
        idx[rng.random((rows, width)) < 0.3] = 0                 # padding / out of vocabulary anywhere in the list
        if width > 1:
            idx[:, 1] = idx[:, 0]                                # the same value twice in one document
        d = (rng.standard_normal((rows, dim)) * 0.05).astype(np.float32)
        idx_dev = torch.from_numpy(idx.astype(np.int32)).to(dev)
        block = torch.full((rows, dim + 11), 7.0, device=dev)
        _hip.cat_encode(table, idx_dev, block[:, off:off + dim], mean=mean)
        want = ora.encode(idx)
        np.testing.assert_allclose(block[:, off:off + dim].cpu().numpy(), want, atol=1e-6, rtol=1e-6)
        assert float(block[:, :off].min()) == 7.0 and float(block[:, off + dim:].min()) == 7.0
        dblock = torch.zeros(rows, dim + 11, device=dev)
        dblock[:, off:off + dim] = torch.from_numpy(d).to(dev)
        _hip.cat_update(table, m, v, idx_dev, dblock[:, off:off + dim], 3e-3, step, mean=mean, grad_scratch=scratch)
        ora._c = 0
        ora.bwd(d)
        ora.step()
        np.testing.assert_allclose(table.cpu().numpy(), ora.params["w"], atol=2e-6, rtol=0, err_msg=f"step {step}")
        om, ov = (ora.opt.m, ora.opt.v) if sparse else (ora.opt.m["w"], ora.opt.v["w"])
        np.testing.assert_allclose(m.cpu().numpy(), om, atol=1e-9, rtol=1e-5)
        np.testing.assert_allclose(v.cpu().numpy(), ov, atol=1e-13, rtol=1e-5)
        if scratch is not None:
            assert float(scratch.abs().max()) == 0.0             # consumed and cleared
    assert float(table[0].abs().max()) == 0.0


def test_categorical_condition_abi_rejects_bad_operands():
    from aaerec import _hip
    dev = torch.device("cuda:0")
    table = torch.zeros(10, 8, device=dev)
    idx = torch.zeros(4, 2, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        _hip.cat_encode(table, idx.long(), torch.zeros(4, 8, device=dev))
    with pytest.raises(TypeError):
        _hip.cat_encode(table, idx, torch.zeros(4, 9, device=dev))
    with pytest.raises(RuntimeError):
        _hip.cat_encode(table.cpu(), idx, torch.zeros(4, 8, device=dev))
    with pytest.raises(_hip.AaeHipError):                        # dim > 256
        _hip.cat_encode(torch.zeros(10, 300, device=dev), idx, torch.zeros(4, 300, device=dev))
    with pytest.raises(_hip.AaeHipError):                        # step counts from 1
        _hip.cat_update(table, torch.zeros_like(table), torch.zeros_like(table), idx, torch.zeros(4, 8, device=dev), 1e-3, 0)
    # out-of-range indices read as padding instead of faulting
    bad = torch.tensor([[11, -3], [1, 2], [0, 0], [9, 10]], dtype=torch.int32, device=dev)
    out = torch.empty(4, 8, device=dev)
    _hip.cat_encode(table + 1.0, bad, out)
    assert out.cpu().numpy()[:, 0].tolist() == [0.0, 2.0, 0.0, 1.0]


@pytest.mark.parametrize("name", ["step_masks", "step_cond_concat", "step_wide", "step_headline", "step_selu"])
def test_ae_phase_cut_at_the_output_layer_equals_fused_step(name):
    """aae_ae_forward + aae_output_layer_step(NULL) + aae_ae_backward(NULL) + disc_gen on one handle reproduce the
    fixtures of the whole step (the cut vocabulary-sharded data parallelism makes, without any sharding)."""
    fx = Fixture(name)
    m = make_model(fx)
    for s in range(fx.steps):
        csr = csr_of(fx, m, s)
        B = csr.shape[0]
        cond = fx.cond_inputs(s)
        m.ae_forward(csr, 0, B, cond=torch.as_tensor(cond[0], device=m.device) if cond else None, masks=fx.masks(s),
                     z_real=fx.z[f"step{s}.z_real"])
        m.output_layer_step()
        m.ae_backward()
        m.disc_gen()
        np.testing.assert_allclose(m.losses(), fx.z[f"step{s}.losses"], rtol=TOL_LOSS, atol=1e-6)
        if fx.has_state(s):
            check_state(fx, m, s, name)


class _ThreadDist:
    """torch.distributed stand-in for `world` ranks living in threads of one process on one GPU: every collective
    publishes a copy of the rank's operand, meets the others at a barrier and combines the copies in rank order."""
    class ReduceOp:
        SUM = "sum"

    def __init__(self, world):
        import threading
        self.world, self.bar, self.slots, self.tls = world, threading.Barrier(world), [None] * world, threading.local()

    def bind(self, rank):
        self.tls.rank = rank

    def get_rank(self, group=None):
        return self.tls.rank

    def get_world_size(self, group=None):
        return self.world

    def get_backend(self, group=None):
        return "threads"

    def _exchange(self, t):
        torch.cuda.synchronize()
        self.slots[self.tls.rank] = t.clone()
        torch.cuda.synchronize()
        self.bar.wait()
        parts = list(self.slots)
        self.bar.wait()
        return parts

    def all_reduce(self, t, op=None, group=None, async_op=False):
        parts = self._exchange(t)
        total = parts[0].clone()
        for p in parts[1:]:
            total += p
        t.copy_(total)

    def all_gather_into_tensor(self, out, inp, group=None, async_op=False):
        out.copy_(torch.cat([p.reshape(-1) for p in self._exchange(inp)]).view(out.shape))

    def reduce_scatter_tensor(self, out, inp, op=None, group=None, async_op=False):
        parts = self._exchange(inp)
        total = parts[0].clone()
        for p in parts[1:]:
            total += p
        out.copy_(total.reshape(self.world, -1)[self.tls.rank].view(out.shape))


@pytest.mark.parametrize("name,world", [("step_masks", 2), ("step_cond_concat", 2), ("step_headline", 2), ("step_wide", 4)])
def test_vocabulary_sharded_ranks_equal_single_process(name, world):
    """aaerec.parallel.VocabParallelAAE with `world` ranks as threads on one GPU: each rank holds a replica for its
    share of the documents and a slice model for its share of the items; after every step the replicas' parameters
    and the concatenated slices of dec.lin3 must be the reference's single-process parameters."""
    import threading
    import scipy.sparse as sp
    from aaerec._hip import HipAAE, DeviceCSR, T_DEC_V3
    from aaerec.parallel import VocabParallelAAE, item_slice
    fx = Fixture(name)
    c = fx.cfg
    N, B = c["N"], c["B"]
    assert B % world == 0
    Bl = B // world
    dist = _ThreadDist(world)
    kw = fx.model_kwargs()
    init = fx.init_params()
    locals_, slices, errors = [None] * world, [None] * world, []

    def rank_main(r):
        try:
            dist.bind(r)
            lo, hi = item_slice(N, r, world)
            m = HipAAE(N, c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=Bl, rng_mode="inject", grad_mode="export",
                       dp_world=world, **kw)
            m.load_params(init)
            sp_params = dict(init)
            sp_params["dec.lin3.weight"], sp_params["dec.lin3.bias"] = init["dec.lin3.weight"][lo:hi], init["dec.lin3.bias"][lo:hi]
            sp_params["enc.lin1.weight"] = init["enc.lin1.weight"][:, lo:hi]
            sl = HipAAE(hi - lo, c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=B, rng_mode="inject", **kw)
            sl.load_params(sp_params)
            locals_[r], slices[r] = m, sl
            vp = VocabParallelAAE(m, sl, dist, N)
            assert (vp.item_lo, vp.item_hi) == (lo, hi)
            for s in range(fx.steps):
                ip, idx, val = fx.batch(s)
                if len(ip) - 1 != B:
                    break                                       # (ragged last batch of a fixture: not divisible)
                X = sp.csr_matrix((val, idx, ip), shape=(B, N))
                csr = DeviceCSR(X, m.device)
                slice_csr = DeviceCSR(X[:, lo:hi], m.device)
                masks = fx.masks(s)
                if masks is not None:
                    masks = [None if k is None else k[r * Bl:(r + 1) * Bl] for k in masks]
                cond = fx.cond_inputs(s)
                vp.step(csr, r * Bl, Bl, slice_csr, 0, B,
                        cond=torch.as_tensor(cond[0][r * Bl:(r + 1) * Bl], device=m.device) if cond else None,
                        masks=masks, z_real=fx.z[f"step{s}.z_real"][r * Bl:(r + 1) * Bl])
                loss = vp.recon_loss()
                if r == 0:
                    np.testing.assert_allclose(loss, fx.z[f"step{s}.losses"][0], rtol=TOL_LOSS)
        except BaseException as e:              # noqa: B902 - a dead rank must not leave the others at a barrier
            errors.append((r, e))
            dist.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    last = fx.steps - 1
    want = fx.expected_params(last)
    got0 = locals_[0].state_dict()
    for k, w in want.items():
        if k.startswith("dec.lin3"):
            continue
        np.testing.assert_allclose(got0[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} {k}")
        for r in range(1, world):                                # replicas stay identical
            np.testing.assert_array_equal(locals_[r].state_dict()[k], got0[k], err_msg=f"rank {r} {k}")
    v3w = np.concatenate([slices[r].state_dict()["dec.lin3.weight"] for r in range(world)])
    v3b = np.concatenate([slices[r].state_dict()["dec.lin3.bias"] for r in range(world)])
    np.testing.assert_allclose(v3w, want["dec.lin3.weight"], atol=TOL_PARAM, rtol=0)
    np.testing.assert_allclose(v3b, want["dec.lin3.bias"], atol=TOL_PARAM, rtol=0)


def test_output_layer_cut_rejects_calls_out_of_order():
    from aaerec._hip import AaeHipError, HipAAE
    fx = Fixture("step_nodrop_gauss")
    m = make_model(fx)
    csr = csr_of(fx, m, 0)
    with pytest.raises(AaeHipError):
        m.output_layer_step()                     # continuing a step that aae_ae_forward never started
    with pytest.raises(AaeHipError):
        m.ae_backward()
    m.ae_forward(csr, 0, csr.shape[0], z_real=fx.z["step0.z_real"])
    with pytest.raises(AaeHipError):              # dL/d(dh2) with a foreign leading dimension
        m.ae_backward(torch.zeros(csr.shape[0], 7, device=m.device))
    m.output_layer_step()
    m.ae_backward()
    m.disc_gen()
    np.testing.assert_allclose(m.losses(), fx.z["step0.losses"], rtol=TOL_LOSS, atol=1e-6)
    # a model too wide for the layer-chain kernels has no cut (its output layer alone still works as a slice handle)
    wide = HipAAE(300, 256, 16, max_batch=8, rng_mode="inject")
    with pytest.raises(AaeHipError):
        wide.ae_forward(csr_of(fx, wide, 0), 0, 8)


@pytest.mark.parametrize("cut", [False, True])
def test_short_batch_on_a_model_sized_for_long_ones(cut):
    """max_batch = 130 (past the fused output-layer kernel's 112 rows) followed by a 90-row batch: the short batch
    qualifies for the fused kernel, whose per-workgroup dA2 slabs the arena must have room for (regression: it was
    sized for the three-kernel path only and the fused kernel wrote out of bounds)."""
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    N, h, c = 1500, 64, 20
    rng = np.random.default_rng(4)
    params = init_params(N, h, c, seed=4)
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.0, 0.0))
    dev = HipAAE(N, h, c, max_batch=130, rng_mode="inject", **kw)
    dev.load_params(params)
    ora = O.OracleAAE(params, **kw)
    for B in (130, 90, 130, 7):
        rows = [np.sort(rng.choice(N, size=int(rng.integers(1, 10)), replace=False)) for _ in range(B)]
        ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        val = np.ones(len(idx), dtype=np.float32)
        zr = rng.standard_normal((B, c)).astype(np.float32)
        csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
        if cut:
            dev.ae_forward(csr, 0, B, z_real=zr)
            dev.output_layer_step()
            dev.ae_backward()
            dev.disc_gen()
        else:
            dev.step(csr, 0, B, z_real=zr)
        np.testing.assert_allclose(dev.losses(), ora.partial_fit(ip, idx, val, zr), rtol=2e-5, atol=1e-6, err_msg=f"B={B}")
    got = dev.state_dict()
    for k, w in ora.p.items():
        np.testing.assert_allclose(got[k], w, atol=2e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("scheme,world", [("vocab", 2), ("replicated", 3), ("vocab", 4), ("vocab", 8), ("replicated", 8)])
def test_device_rng_draws_by_global_row_so_ranks_reproduce_the_single_process_run(scheme, world):
    """rng_mode='device' (the production generator): dropout masks and the prior sample are keyed by the row of the
    GLOBAL batch (aae_set_rng_rows), so `world` ranks with one seed, each holding a share of the batch, reproduce the
    single-process run of that seed up to fp32 summation order (1-GPU and N-GPU runs comparable)."""
    import threading
    import scipy.sparse as sp
    from aaerec._hip import HipAAE, DeviceCSR
    from aaerec.parallel import DataParallelAAE, VocabParallelAAE, item_slice
    from oracle.dense_torch_port import init_params
    N, h, c, Bl = 700, 48, 12, 12
    B = Bl * world
    rng = np.random.default_rng(world)
    params = init_params(N, h, c, seed=9)
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.2, 0.3), rng_mode="device", seed=1234)
    batches = []
    for s in range(4):
        rows = [np.sort(rng.choice(N, size=int(rng.integers(1, 10)), replace=False)) for _ in range(B)]
        ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        batches.append(sp.csr_matrix((np.ones(len(idx), dtype=np.float32), idx, ip), shape=(B, N)))
    one = HipAAE(N, h, c, max_batch=B, **kw)
    one.load_params(params)
    for X in batches:
        one.step(DeviceCSR(X, one.device), 0, B)
    want = one.state_dict()
    dist = _ThreadDist(world)
    locals_, slices, errors = [None] * world, [None] * world, []

    def rank_main(rk):
        try:
            dist.bind(rk)
            m = HipAAE(N, h, c, max_batch=Bl, grad_mode="export", dp_world=world, **kw)
            m.load_params(params)
            locals_[rk] = m
            if scheme == "vocab":
                lo, hi = item_slice(N, rk, world)
                sp_params = dict(params)
                sp_params["dec.lin3.weight"], sp_params["dec.lin3.bias"] = params["dec.lin3.weight"][lo:hi], params["dec.lin3.bias"][lo:hi]
                sp_params["enc.lin1.weight"] = params["enc.lin1.weight"][:, lo:hi]
                sl = HipAAE(hi - lo, h, c, max_batch=B, **kw)
                sl.load_params(sp_params)
                slices[rk] = sl
                dp = VocabParallelAAE(m, sl, dist, N)
                for X in batches:
                    dp.step(DeviceCSR(X, m.device), rk * Bl, Bl, DeviceCSR(X[:, lo:hi], m.device), 0, B)
            else:
                dp = DataParallelAAE(m, dist, shard_decoder=True)
                for X in batches:
                    dp.step(DeviceCSR(X, m.device), rk * Bl, Bl, global_rows=B)
                    dp.wait_pending()
        except BaseException as e:              # noqa: B902
            errors.append((rk, e))
            dist.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(rk,)) for rk in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    got0 = locals_[0].state_dict()
    for k, w in want.items():
        got = got0[k]
        if k.startswith("dec.lin3") and scheme == "vocab":
            got = np.concatenate([slices[rk].state_dict()[k] for rk in range(world)])
        d = np.abs(got - w)
        assert (d > 5e-5).sum() <= max(8, 0.01 * d.size) and d.max() <= 6e-3, f"{scheme} x{world} {k}: {(d > 5e-5).sum()} off, max {d.max():.2e}"
    # and a different seed does give a different run (the comparison above is not vacuous)
    other = HipAAE(N, h, c, max_batch=B, **dict(kw, seed=99))
    other.load_params(params)
    for X in batches:
        other.step(DeviceCSR(X, other.device), 0, B)
    assert np.abs(other.state_dict()["enc.lin2.weight"] - want["enc.lin2.weight"]).max() > 1e-3
