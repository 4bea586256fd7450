"""The deferred first-layer Adam on the device (csrc/kernels.h: lazy_replay, w1_catchup_kernel, advance_step_body) against
the float64 zero-gradient reference of tests/lazy_adam.py, under its derived bounds.

An item that only ever enters a batch with VALUE 0 is listed among the step's distinct items - its row is caught up and
passes through the sparse update - with a gradient of exactly 0: its row of enc.lin1 follows a trajectory that depends on
its own (p, m1, v1, m3, v3), the step numbers and the two learning rates alone.  Items 0..31 are busy (real values, train
normally, not compared here), items 64.. are such probe rows with the probe states of lazy_adam.probe_states loaded as
their moments.  The runs follow lazy_adam.Plan: learning rates changed by set_lr in mid-run, start steps on both sides of
the ring's wrap and at 2e7, lazy gaps of 1 .. 244 steps (and of 1 400), and every caller of the catch-up."""
import numpy as np
import pytest

import lazy_adam as L
from lazy_adam import KEYS, Plan, START_STEPS, WRAP

pytestmark = pytest.mark.gpu

N, C, B = 384, 6, 4
BUSY, PROBE0 = 32, 64
PATHS = ("own", "prefetch", "early", "hints", "predict", "export", "dense")
WORST = {}                                   # quantity -> the worst error / bound ratio seen in this session (printed)


def _csr(rows, vals, dev):
    from aaerec._hip import DeviceCSR
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    val = np.concatenate(vals).astype(np.float32)
    return ip, idx, val, DeviceCSR.from_arrays(ip, idx, val, N, dev.device)


def _batch(rng, probes, dev):
    """B documents of 1-4 busy items (value 1); the probe items are spread over them with value 0."""
    rows = [np.sort(rng.choice(BUSY, size=int(rng.integers(1, 5)), replace=False)) for _ in range(B)]
    vals = [np.ones(len(r), dtype=np.float32) for r in rows]
    for n, i in enumerate(probes):
        rows[n % B] = np.append(rows[n % B], PROBE0 + i)
        vals[n % B] = np.append(vals[n % B], np.float32(0.0))
    return _csr(rows, vals, dev)


def _moment_arrays(pl, h, rows):
    """[h, N] moment tensors of enc.lin1 (enc_optim's and gen_optim's), zero but for the probe states of `rows`."""
    out = {k: np.zeros((h, N), dtype=np.float32) for k in KEYS[1:]}
    for i in rows:
        for k in KEYS[1:]:
            out[k][:, PROBE0 + i] = pl.states[k][i]
    return out


def run_plan(pl, path, oracle=False, oracle_rtol=2e-4, oracle_atol=3e-5):
    """The plan on the device through `path`; -> worst error / bound per quantity (asserting every element's bound)."""
    from aaerec._hip import HipAAE, O_ENC, O_GEN
    from oracle.dense_torch_port import init_params
    h, T0, S = pl.h, pl.T0, pl.S
    rng = np.random.default_rng(17)
    params = init_params(N, h, C, seed=3)
    items = PROBE0 + np.arange(pl.P)
    params["enc.lin1.weight"][:, items] = pl.states["p"].T
    kw = dict(gen_lr=pl.base[0], reg_lr=pl.base[1], dropout=(0.0, 0.0))
    extra = dict(grad_mode="export", dp_world=1, w1_cap=N) if path == "export" else \
        dict(dense_noise=True, ae_only=True) if path == "dense" else {}
    dev = HipAAE(N, h, C, max_batch=B, rng_mode="inject", **kw, **extra)
    dev.load_params(params)
    first = [i for i in range(pl.P) if not pl.groups[i][0]]
    mom = _moment_arrays(pl, h, first)
    dev.load_adam(O_ENC, 1, m_w=mom["m1"], v_w=mom["v1"], step=T0)
    dev.load_adam(O_GEN, 1, m_w=mom["m3"], v_w=mom["v3"], step=T0)
    ora = None
    if oracle:
        from oracle import aae_oracle as O
        ora = O.OracleAAE(params, **kw)
        for opt, mk, vk in ((ora.opt_enc, "m1", "v1"), (ora.opt_gen, "m3", "v3")):
            for k, w in ora.p.items():
                if k.startswith("enc."):
                    opt.m[k], opt.v[k], opt.t[k] = np.zeros_like(w), np.zeros_like(w), T0
            opt.m["enc.lin1.weight"], opt.v["enc.lin1.weight"] = mom[mk].copy(), mom[vk].copy()
    if path == "export":
        from aaerec.parallel import DataParallelAAE
        from test_fuzz_gpu import _Solo
        dp = DataParallelAAE(dev, _Solo(), shard_decoder=False)
    batches = [None] + [_batch(rng, pl.probes_at(s), dev) for s in range(1, S + 1)]
    zs = [None] + [rng.standard_normal((B, C)).astype(np.float32) for _ in range(S)]
    decoy = _batch(rng, [], dev)
    preds = {s: _batch(rng, rows, dev) for s, rows in pl.pred_after.items()}
    hinted = path in ("prefetch", "early", "hints")
    for s in range(1, S + 1):
        ip, idx, val, csr = batches[s]
        if s in pl.lr:                                # (with hints: the list of this step's batch is built and pending)
            dev.set_lr(*pl.lr[s])
            if ora:
                ora.opt_enc.lr = ora.opt_dec.lr = float(pl.lr[s][0])
                ora.opt_gen.lr = ora.opt_disc.lr = float(pl.lr[s][1])
        if hinted and s < S and not (path == "hints" and s % 7 == 3):
            dev.prefetch(decoy[3] if path == "hints" and s % 11 == 5 else batches[s + 1][3], 0, B)
        if path == "dense" and s == pl.dense_at:
            import torch
            noise = 0.01 * rng.standard_normal((B, N)).astype(np.float32)
            noise[:, items] = 0.0                      # the probes' columns of the dense input stay 0: their gradient too
            dev.set_input_noise(torch.as_tensor(noise))
        if path == "export":
            dp.step(csr, 0, B, global_rows=B, z_real=zs[s])
            dp.wait_pending()
        else:
            dev.step(csr, 0, B, z_real=None if path == "dense" else zs[s])
        if ora:
            want = ora.partial_fit(ip, idx, val, zs[s])
            if s % 20 == 0 or s == S:
                got = np.asarray(dev.losses(), dtype=np.float64)
                print(f"step {s}: losses, largest relative difference to the oracle {np.max(np.abs(got - want) / np.abs(want)):.3g}")
                np.testing.assert_allclose(got, want, rtol=oracle_rtol, atol=1e-6, err_msg=f"step {s}")
        if s in preds:
            dev.predict(preds[s][3], 0, B)
        if s in pl.reloads:
            rows = [i for i in range(pl.P) if pl.groups[i][0] == s]
            new = _moment_arrays(pl, h, rows)
            cols = PROBE0 + np.array(rows)
            for oid, mk, vk, opt in ((O_ENC, "m1", "v1", ora and ora.opt_enc), (O_GEN, "m3", "v3", ora and ora.opt_gen)):
                mw, vw, _, _, _ = dev.store_adam(oid, 1, bias=False, step=False)      # (flushes every row through step s)
                mw[:, cols], vw[:, cols] = new[mk][:, cols], new[vk][:, cols]
                dev.load_adam(oid, 1, m_w=mw, v_w=vw)
                if opt:
                    opt.m["enc.lin1.weight"][:, cols] = new[mk][:, cols]
                    opt.v["enc.lin1.weight"][:, cols] = new[vk][:, cols]
    sd = dev.state_dict()
    enc, gen = dev.adam_state("enc"), dev.adam_state("gen")
    assert enc["step"] == T0 + S and gen["step"] == T0 + S
    got = dict(p=sd["enc.lin1.weight"], m1=enc["lin1.weight"][0], v1=enc["lin1.weight"][1],
               m3=gen["lin1.weight"][0], v3=gen["lin1.weight"][1])
    worst, bad = {k: 0.0 for k in KEYS}, []
    for i in range(pl.P):
        ref, _, tol = pl.reference(i)
        for k in KEYS:
            err = np.abs(got[k][:, PROBE0 + i].astype(np.float64) - ref[k])
            r = np.where(err > 0, err / np.maximum(tol[k], 1e-300), 0.0)
            worst[k] = max(worst[k], float(r.max()))
            if (err > tol[k]).any():
                c = int(r.argmax())
                bad.append((i, pl.groups[i], k, c, float(err[c]), float(tol[k][c]), float(ref[k][c])))
    for k in KEYS:
        WORST[k] = max(WORST.get(k, 0.0), worst[k])
    print(f"T0={T0} S={S} h={h} {path}: worst |device - replay64| / bound:", {k: round(v, 4) for k, v in worst.items()},
          "| so far:", {k: round(v, 4) for k, v in WORST.items()})
    assert not bad, (path, T0, bad[:8])
    if ora:
        print("parameters, largest |device - oracle|:", {k: float(np.max(np.abs(sd[k] - w))) for k, w in ora.p.items()})
        for k, w in ora.p.items():
            np.testing.assert_allclose(sd[k], w, atol=oracle_atol, rtol=0, err_msg=k)
        np.testing.assert_allclose(enc["lin1.weight"][0], ora.opt_enc.m["enc.lin1.weight"], atol=1e-8, rtol=1e-3)
        np.testing.assert_allclose(enc["lin1.weight"][1], ora.opt_enc.v["enc.lin1.weight"], atol=1e-12, rtol=1e-3)
        np.testing.assert_allclose(gen["lin1.weight"][1], ora.opt_gen.v["enc.lin1.weight"], atol=1e-12, rtol=1e-3)
    dev.close()
    return worst


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("T0", START_STEPS)
def test_probe_rows_follow_zero_gradient_adam(T0, path, monkeypatch):
    """Plan.main - 300 steps, six set_lr calls, gaps of 1 .. 244 steps - from step 0, from 140 steps short of the ring's wrap
    (the long gaps straddle it), from 5 short of its second wrap and from 2e7, with the rows caught up by: the step's own
    catch-up; the prefetch of the true next batch (every set_lr then falls on a built, pending list); its early form
    (AAE_EARLY_ANY: every set_lr sits in front of a step that would start its catch-up on the table entry written a step
    early); hints left out (s % 7 == 3) or naming a batch that does not come (s % 11 == 5); an eval-mode predict in mid-run;
    the gradient-export path of one data-parallel rank (w1_export / w1_import); a dense noisy-input step at 250, which reads
    every row (the plain autoencoder's: the library has the dense input for that model only, so gen_optim's moments are 0)."""
    if path == "early":
        monkeypatch.setenv("AAE_EARLY_ANY", "1")
    dense = dict(dense_at=250, ae_only=True) if path == "dense" else {}
    run_plan(Plan.main(T0, predict=path == "predict", **dense), path)


@pytest.mark.parametrize("path", ["own", "early"])
@pytest.mark.parametrize("T0", [0, L.CAP - 100, 20_000_000])
def test_the_replay_keeps_exactly_128_increments(T0, path, monkeypatch):
    """Plan.cut: the rates are 0 until step 128 of segments that start at T0, so the last increment the replay keeps is the
    first that moves p - one kept too few or too many is far outside the bounds (from L.CAP - 100 the replayed steps
    straddle the wrap)."""
    if path == "early":
        monkeypatch.setenv("AAE_EARLY_ANY", "1")
    run_plan(Plan.cut(T0), path)


@pytest.mark.parametrize("T0", [L.CAP - 700, 20_000_000])
def test_closed_form_decay_over_more_than_a_thousand_steps(T0):
    """Plan.long: 1 500 steps, one probe row touched once at step 1 400 and one never - 1 272 and 1 372 steps of closed-form
    decay (across the wrap from L.CAP - 700), which hold the two exp2f constants to 3e-5 relative in v."""
    run_plan(Plan.long(T0, 1500, 1400), "own")


def test_closed_form_decay_over_four_thousand_steps():
    """Plan.long at 4 000 steps from 2 000 short of the wrap: a row touched at step 2 and one never (2 s on an MI355X)."""
    run_plan(Plan.long(L.CAP - 2000, 4000, 2), "own")


def test_columns_beyond_256_on_the_per_layer_path():
    """h = 300: the catch-up's `c += 256` loop takes a second round (hidden widths beyond the layer-chain kernels)."""
    run_plan(Plan.main(0, h=300), "own")


def test_whole_model_matches_the_oracle_under_the_schedule_across_the_wrap():
    """The same run with missing and wrong hints from 140 steps short of the wrap, every parameter against the eager fp32
    oracle with its rates and step counts set alike (the tolerances of
    test_deferred_adam_matches_eager_oracle_over_many_sparse_steps): set_lr on the eager optimisers and on the sparse update.
    All rates are a tenth of the other cases' (2e-4 / 1e-4, so 2e-3 / 1e-3 at their highest - that test's rates).  Measured:
    losses within 2e-7 relative and parameters within 6e-7 of the oracle over the 300 steps.  At the other cases' rates the
    losses agree to 1e-6 for 240 steps and then part (4e-4 at step 260, 5e-3 at step 300; parameters up to 1e-2): a gradient
    of the order of Adam's eps whose step is of the order of the rate (tests/test_fuzz_gpu.py describes the effect), which a
    four-document batch at 2e-2 does not forgive - the probe rows, which no forward pass reads, are untouched by it."""
    run_plan(Plan.main(WRAP, lr_scale=0.1), "hints", oracle=True)
