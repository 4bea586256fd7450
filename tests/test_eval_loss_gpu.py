"""GPU parity of the held-out loss (csrc/loss_eval.h: the loss epilogue of rank_x3_kernel, loss_targets_kernel,
loss_finish_kernel, vae_kl_rows_kernel, loss_rows_dense_kernel; aae_predict_loss / aae_decode_loss / aae_vae_predict_loss /
aae_vae_decode_loss) and of eval_loss on the model classes.  Reference: aae.py:176-177, 693-695 and vae.py:132-145, 243-264.

The kernels are held to tests/loss_cases.py row_bce / row_kl of the ORACLE's logits (the restatement is pinned to torch on the
CPU, tests/test_eval_loss_cpu.py).  Tolerance per row: the per-row form of golden_util.bce_quantisation_bound plus TOL_LOSS
(2e-6, tests/test_oracle_golden.py: "fp32 summation order only") relative; the mean carries the same bound.  Fused against
dense: BOTH routes are measured against the oracle at that tolerance (the simpler of the two rules the feature's issue offers)."""
import contextlib
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

# A row's KL against the float64 restatement: its n_code cell terms -0.5 (1 + logvar - mu^2 - exp(logvar)) are formed in fp32 -
# four roundings of values of magnitude ~1, 2^-24 each, halved - so 2 * 2^-24 a cell of absolute error whatever the row's sum
# is (the terms cancel: a row of a barely trained model sums to 0.01), on top of the relative 2e-5 the total is held to.
KL_ATOL = LC.CODE * 2.0 ** -23


@contextlib.contextmanager
def _dense_route():
    """Handles created inside take the dense form of every ranking and loss call (option NO_RANK_FUSED)."""
    from aaerec import _hip
    _hip.set_option("NO_RANK_FUSED", "1")
    try:
        yield
    finally:
        _hip.set_option("NO_RANK_FUSED", None)


def _device(cs, dense, **kw):
    if not dense:
        dev = cs.device(**kw)
        assert dev.loss_max_rows() >= LC.ROWS, dev.loss_max_rows()
        return dev
    with _dense_route():
        dev = cs.device(**kw)
    assert dev.loss_max_rows() == LC.MAX_BATCH
    return dev


def _aae_rows(dev, cs, chunk, targets=True):
    """The 130 rows of the case, `chunk` rows a call."""
    return torch.cat([dev.predict_loss(cs.csr, s, min(chunk, LC.ROWS - s), cond=None if cs.cond_t is None else cs.cond_t[s:s + chunk],
                                       targets=cs.tcsr if targets else None) for s in range(0, LC.ROWS, chunk)])


def _vae_rows(dev, cs, chunk, eps=True, row0=None):
    """(BCE rows, KL rows) of the 130 rows, `chunk` rows a call; row0: None = every chunk's first row."""
    parts = [dev.vae_predict_loss(cs.csr, s, min(chunk, LC.ROWS - s), cond=None if cs.cond_t is None else cs.cond_t[s:s + chunk],
                                  eps=cs.eps_t[s:s + chunk] if eps else None, row0=(s if row0 is None else row0), targets=cs.tcsr)
             for s in range(0, LC.ROWS, chunk)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _snapshot(dev):
    """Every parameter and every Adam moment of the handle, by name."""
    out = dict(dev.state_dict())
    for which in ("enc", "dec", "gen", "disc"):
        for name, mv in dev.adam_state(which).items():
            if name == "step":
                out[f"{which}.step"] = np.asarray(mv)
            else:
                out[f"{which}.{name}.m"], out[f"{which}.{name}.v"] = mv
    return out


def _check_rows(got, want, bound, what):
    tol = bound + LC.TOL_LOSS * np.abs(want)
    err = np.abs(got - want)
    print(f"{what}: max |row diff| = {err.max():.3g} (relative {float((err / np.abs(want)).max()):.3g}), largest share of a row's "
          f"tolerance = {float((err / tol).max()):.3g}; mean diff = {abs(got.mean() - want.mean()):.3g} of {tol.mean():.3g}")
    assert np.all(err <= tol), (what, int(np.argmax(err / tol)), float((err / tol).max()))
    assert abs(got.mean() - want.mean()) <= tol.mean(), what


@pytest.mark.parametrize("dense", [False, True], ids=["fused", "dense"])
@pytest.mark.parametrize("case", LC.AAE_CASES, ids=[c[0] for c in LC.AAE_CASES])
def test_predict_loss_matches_the_oracle_on_both_routes(case, dense):
    """aae_predict_loss per row against row_bce of OracleAAE's logits: targets with an empty row, a 90-entry row, fractional
    values, other items than the inputs; one case with saturated cells on zero and non-zero targets.  The fused route in one
    call of 130 rows, the dense one max_batch rows at a time; then the decode form behind aae_encode."""
    cs = LC.AaeCase(*case)
    assert LC.zone_clear(cs.logits)
    dev = _device(cs, dense)
    want = LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval)
    bound = LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval)
    chunk = LC.MAX_BATCH if dense else LC.ROWS
    got = _aae_rows(dev, cs, chunk)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (LC.ROWS,)
    _check_rows(got.cpu().numpy(), want, bound, f"{cs.name} predict form")
    z = torch.cat([dev.encode(cs.csr, s, min(LC.MAX_BATCH, LC.ROWS - s)) for s in range(0, LC.ROWS, LC.MAX_BATCH)])
    zc = z if cs.cond_t is None else torch.cat([z, cs.cond_t], 1)
    got2 = torch.cat([dev.decode_loss(zc[s:s + chunk], cs.csr, s, targets=cs.tcsr) for s in range(0, LC.ROWS, chunk)])
    _check_rows(got2.cpu().numpy(), want, bound, f"{cs.name} decode form")
    # targets = None: the input rows themselves
    want_x = LC.row_bce(cs.logits, cs.ip, cs.idx, cs.val)
    _check_rows(_aae_rows(dev, cs, chunk, targets=False).cpu().numpy(), want_x, LC.row_bound(cs.logits, cs.ip, cs.idx, cs.val),
                f"{cs.name} targets = inputs")


def test_decode_loss_on_a_decoder_only_handle_matches_the_oracle():
    """The DecodingRecommender's handle (decoder alone, its input the caller's): aae_decode_loss against OracleDecoder."""
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    cs = LC.AaeCase("decoder", 24, 0, 4, False)
    n_in = 20
    p = LC.aae_params(24, n_in - LC.CODE, 4)
    ora = O.OracleDecoder(p, dropout=(0.0, 0.0))
    zin = (np.random.default_rng(8).standard_normal((LC.ROWS, n_in)) * 0.5).astype(np.float32)
    logits = LC.decoder_logits(ora, zin)
    assert LC.zone_clear(logits)
    dev = HipAAE(LC.N, 24, n_in, cond_inc=0, max_batch=LC.MAX_BATCH, max_nnz=LC.MAX_BATCH * LC.N, dropout=(0.0, 0.0), seed=1)
    dev.load_params({k: v for k, v in p.items() if k.startswith("dec.")})
    csr = DeviceCSR.from_arrays(cs.ip, cs.idx, cs.val, LC.N, dev.device)
    tcsr = DeviceCSR.from_arrays(cs.tip, cs.tidx, cs.tval, LC.N, dev.device)
    got = dev.decode_loss(torch.as_tensor(zin, device=dev.device), csr, 0, targets=tcsr).cpu().numpy()
    _check_rows(got, LC.row_bce(logits, cs.tip, cs.tidx, cs.tval), LC.row_bound(logits, cs.tip, cs.tidx, cs.tval), "decoder-only handle")


@pytest.mark.parametrize("dense", [False, True], ids=["fused", "dense"])
@pytest.mark.parametrize("case", LC.VAE_CASES, ids=[c[0] for c in LC.VAE_CASES])
def test_vae_predict_loss_matches_the_oracle_on_both_routes(case, dense):
    """aae_vae_predict_loss with injected eps: the BCE rows as above, the KL rows against row_kl of the oracle's (mu, logvar),
    and the reference's test loss (mean BCE + KL) / rows at rtol 2e-5, the figure test_vae_step_matches_reference holds the
    step's logged loss to."""
    cs = LC.VaeCase(*case)
    assert LC.zone_clear(cs.logits)
    dev = _device(cs, dense)
    chunk = LC.MAX_BATCH if dense else LC.ROWS
    bce, kl = _vae_rows(dev, cs, chunk)
    bce, kl = bce.cpu().numpy(), kl.cpu().numpy()
    want = LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval)
    _check_rows(bce, want, LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval), f"vae {cs.name}")
    want_kl = LC.row_kl(cs.mu, cs.lv)
    print("KL rows: max relative diff =", float(np.abs(kl / want_kl - 1).max()))
    np.testing.assert_allclose(kl, want_kl, rtol=2e-5, atol=KL_ATOL)
    np.testing.assert_allclose(LC.reference_test_loss(bce, kl, LC.N, LC.MAX_BATCH),
                               LC.reference_test_loss(want, want_kl, LC.N, LC.MAX_BATCH), rtol=2e-5)
    if not dense:        # the decode form behind aae_vae_encode(train = 0)
        z = torch.cat([dev.vae_encode(cs.csr, s, min(LC.MAX_BATCH, LC.ROWS - s), eps=cs.eps_t[s:s + LC.MAX_BATCH], train=False)
                       for s in range(0, LC.ROWS, LC.MAX_BATCH)])
        zc = z if cs.cond_t is None else torch.cat([z, cs.cond_t], 1)
        _check_rows(dev.vae_decode_loss(zc, cs.csr, 0, targets=cs.tcsr).cpu().numpy(), want,
                    LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval), f"vae {cs.name} decode form")


def test_the_evaluated_loss_is_the_loss_of_the_training_step_on_that_batch():
    """Dropout off: eval of a batch, then the step on the same batch - the step's loss is a function of the pre-step
    parameters.  AAE: the mean against losses()[0]; VAE (same eps): mean BCE against losses()[0], KL sum against losses()[1].
    TOL_LOSS relative."""
    n = LC.MAX_BATCH
    cs = LC.AaeCase(*LC.AAE_CASES[1])
    dev = cs.device()
    z_real = np.random.default_rng(3).standard_normal((n, LC.CODE)).astype(np.float32)
    for s in range(2):          # (the second round: behind a step - deferred launches in flight, first-layer rows pending)
        lo = s * n
        ev = float(dev.predict_loss(cs.csr, lo, n, cond=cs.cond_t[lo:lo + n]).sum().item()) / (n * LC.N)
        dev.step(cs.csr, lo, n, cond=cs.cond_t[lo:lo + n], z_real=z_real)
        st = dev.losses()[0]
        print(f"aae round {s}: evaluated {ev!r}, the step's {st!r}, relative difference {abs(ev - st) / st:.3g}")
        assert abs(ev - st) <= LC.TOL_LOSS * st
    vs = LC.VaeCase(*LC.VAE_CASES[1])
    vdev = vs.device()
    for s in range(2):
        lo = s * n
        bce, kl = vdev.vae_predict_loss(vs.csr, lo, n, cond=vs.cond_t[lo:lo + n], eps=vs.eps_t[lo:lo + n])
        ev_b, ev_k = float(bce.sum().item()) / (n * LC.N), float(kl.sum().item())
        vdev.vae_step(vs.csr, lo, n, cond=vs.cond_t[lo:lo + n], eps=vs.eps[lo:lo + n])
        st = vdev.losses()
        print(f"vae round {s}: BCE {ev_b!r} / {st[0]!r} ({abs(ev_b - st[0]) / st[0]:.3g}), KL {ev_k!r} / {st[1]!r} ({abs(ev_k - st[1]) / st[1]:.3g})")
        assert abs(ev_b - st[0]) <= LC.TOL_LOSS * st[0] and abs(ev_k - st[1]) <= LC.TOL_LOSS * st[1]


def test_chunked_calls_agree_and_two_calls_give_the_same_bits():
    """130 rows in one call, as 128 + 2 and as 7-row chunks: the cell terms are the same bits, only the fp64 order differs -
    N * 2^-53 relative per row.  Two identical calls: identical bits."""
    cs = LC.AaeCase(*LC.AAE_CASES[2])
    dev = cs.device()
    whole = _aae_rows(dev, cs, LC.ROWS)
    assert torch.equal(whole, _aae_rows(dev, cs, LC.ROWS))
    for chunk in (128, 7):
        part = _aae_rows(dev, cs, chunk)
        rel = ((part - whole).abs() / whole.abs()).max().item()
        print(f"chunks of {chunk}: max relative row difference {rel:.3g} (bound {LC.N * 2.0 ** -53:.3g})")
        assert rel <= LC.N * 2.0 ** -53
    with _dense_route():
        ddev = cs.device()
    a, b = _aae_rows(ddev, cs, LC.MAX_BATCH), _aae_rows(ddev, cs, LC.MAX_BATCH)
    assert torch.equal(a, b)
    assert ((_aae_rows(ddev, cs, 7) - a).abs() / a.abs()).max().item() <= LC.N * 2.0 ** -53


def test_vae_device_generator_row0_gives_every_chunk_its_own_draws():
    """rng_mode='device': with row0 = the chunk's first row a chunked evaluation equals the call over all rows (same bound);
    with row0 = 0 in every chunk the draws repeat and the rows beyond the first chunk differ.  Identical calls: identical bits."""
    cs = LC.VaeCase(*LC.VAE_CASES[0])
    dev = cs.device(rng_mode="device")
    whole_b, whole_k = _vae_rows(dev, cs, LC.ROWS, eps=False)
    again_b, again_k = _vae_rows(dev, cs, LC.ROWS, eps=False)
    assert torch.equal(whole_b, again_b) and torch.equal(whole_k, again_k)
    for chunk in (128, 7):
        b, k = _vae_rows(dev, cs, chunk, eps=False)
        assert ((b - whole_b).abs() / whole_b.abs()).max().item() <= LC.N * 2.0 ** -53, chunk
        assert torch.equal(k, whole_k), chunk           # (a row's KL: the same sums in the same order)
    b0, k0 = _vae_rows(dev, cs, 7, eps=False, row0=0)
    assert torch.equal(b0[:7], whole_b[:7])
    rel = ((b0[7:] - whole_b[7:]).abs() / whole_b[7:].abs())
    print("row0 = 0 in every chunk: rows whose BCE differs from the whole call's:", int((rel > LC.N * 2.0 ** -53).sum()), "of", LC.ROWS - 7)
    assert (rel > 1e-9).sum().item() >= (LC.ROWS - 7) * 0.9
    with _dense_route():
        ddev = cs.device(rng_mode="device")
    d_b, d_k = _vae_rows(ddev, cs, LC.MAX_BATCH, eps=False)
    np.testing.assert_allclose(d_k.cpu().numpy(), whole_k.cpu().numpy(), rtol=2e-5, atol=KL_ATOL)      # (the same mu / logvar: KL needs no draw)
    np.testing.assert_allclose(d_b.cpu().numpy(), whole_b.cpu().numpy(), rtol=1e-4)      # (the same draws: row0 reaches the dense route)


def test_bf16_handle_is_held_to_the_rounded_restatement():
    """A bf16 handle against the oracle in bf16 mode (tests/test_bf16_gpu.py: the operands of every matrix-core product, dh2 and
    V3 among them, through oracle.aae_oracle.bf16_round): loss_targets_kernel rounds its two operands the same way."""
    cs = LC.AaeCase("bf16", 200, 0, 5, False, bf16=True)
    assert LC.zone_clear(cs.logits)
    dev = cs.device()
    _check_rows(_aae_rows(dev, cs, LC.ROWS).cpu().numpy(), LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval),
                LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval), "bf16 handle")


def test_a_loss_call_between_two_steps_changes_nothing():
    """No parameter or Adam moment moves, and the step behind the call equals the same step without it, bit for bit (the call
    joins the deferred optimiser launch and flushes the pending first-layer updates as a ranking call does)."""
    cs = LC.AaeCase(*LC.AAE_CASES[1])
    n = LC.MAX_BATCH
    z_real = np.random.default_rng(3).standard_normal((2, n, LC.CODE)).astype(np.float32)
    states = []
    for with_call in (False, True):
        dev = cs.device()
        dev.step(cs.csr, 0, n, cond=cs.cond_t[:n], z_real=z_real[0])
        if with_call:
            before = _snapshot(dev)
            _aae_rows(dev, cs, LC.ROWS)
            after = _snapshot(dev)
            for k in before:
                assert np.array_equal(before[k], after[k]), k
        dev.step(cs.csr, n, n, cond=cs.cond_t[n:2 * n], z_real=z_real[1])
        states.append((_snapshot(dev), dev.losses()))
    for k in states[0][0]:
        assert np.array_equal(states[0][0][k], states[1][0][k]), k
    assert states[0][1] == states[1][1]


# ---- the Python surface ------------------------------------------------------------------------------------------------
class _Set:
    def __init__(self, X):
        self.X = X

    def tocsr(self):
        return self.X


def _host_mean_bce(pred, X):
    """mean of F.binary_cross_entropy(predict + 1e-12, X + 1e-12) as torch forms it (fp32)."""
    T = torch.as_tensor(np.asarray(X.todense(), dtype=np.float32))
    return float(torch.nn.functional.binary_cross_entropy(torch.as_tensor(np.asarray(pred, dtype=np.float32)) + 1e-12, T + 1e-12).item())


def _surface_tol(pred, X):
    """The bound of the oracle test from the library's own scores (logit = log(s / (1 - s)) where s < 1), plus TOL_LOSS and
    the rounding of torch's fp32 mean (2^-23 relative: pairwise sums of fp32 cells)."""
    from golden_util import bce_quantisation_bound
    s = np.clip(np.asarray(pred, dtype=np.float64), 1e-30, 1 - 2.0 ** -25)
    Xc = X.tocsr()
    return bce_quantisation_bound(np.log(s / (1 - s)), Xc.indptr, Xc.indices, Xc.data)


@pytest.mark.parametrize("kind", ["aae", "dae", "vae", "decoder"])
def test_recommenders_eval_loss_equals_the_host_loss_of_their_own_predict(kind):
    from test_rank_recommenders_gpu import _bags, _make
    torch.manual_seed(5)
    np.random.seed(5)
    bags = _bags().build_vocab()
    if kind == "aae":
        from aaerec.aae import AAERecommender
        rec = AAERecommender(n_hidden=40, n_code=16, n_epochs=4, batch_size=50, gen_lr=0.01, reg_lr=0.001, verbose=False, seed=11)
    else:
        rec = _make(kind)
    rec.train(bags)
    X = bags.tocsr()
    torch.manual_seed(77)
    got = rec.eval_loss(bags)
    torch.manual_seed(77)           # (the VAE in rng_mode='reference': the eps of predict())
    pred = rec.predict(bags)
    if kind == "vae":
        # the reference's test loss: per batch of batch_size rows the host BCE mean of predict()'s scores + the batch's KL
        # (predict() returns no mu / logvar: the KL rows are the per-row call's, held to the oracle in the tests above)
        torch.manual_seed(77)
        _, kl = rec.model.eval_loss(X, per_row=True)
        spans = [slice(s, s + 50) for s in range(0, X.shape[0], 50)]
        want_bce = sum(_host_mean_bce(pred[sl], X[sl]) for sl in spans)
        want = (want_bce + kl.sum()) / X.shape[0]
        tol = (sum(_surface_tol(pred[sl], X[sl]) for sl in spans) + (LC.TOL_LOSS + 2.0 ** -23) * want_bce) / X.shape[0]
    else:
        want = _host_mean_bce(pred, X)
        tol = _surface_tol(pred, X) + (LC.TOL_LOSS + 2.0 ** -23) * want
    print(f"{kind}: eval_loss {got!r}, host loss of predict() {want!r}, difference {abs(got - want):.3g} of {tol:.3g}")
    assert abs(got - want) <= tol


def test_vae_predict_prints_the_reference_test_loss_only_when_asked(capsys):
    from aaerec.vae import VAE
    from oracle import aae_oracle as O
    cs = LC.VaeCase(*LC.VAE_CASES[0])
    torch.manual_seed(1)
    m = VAE(LC.N, LC.N, n_hidden=cs.h, n_code=LC.CODE, batch_size=LC.MAX_BATCH, verbose=False, rng_mode="reference")
    m.hip.load_params(LC.vae_to_hip(cs.params))
    X = sp.csr_matrix((cs.val, cs.idx, cs.ip), shape=(LC.ROWS, LC.N))
    torch.manual_seed(9)
    plain = m.predict(X)
    assert "Test set loss" not in capsys.readouterr().out and m.last_test_loss is None
    torch.manual_seed(9)
    eps = torch.cat([torch.randn(min(LC.MAX_BATCH, LC.ROWS - s), LC.CODE) for s in range(0, LC.ROWS, LC.MAX_BATCH)]).numpy()
    torch.manual_seed(9)
    again = m.predict(X, test_loss=True)
    out = capsys.readouterr().out
    assert np.array_equal(plain, again)
    assert re.search(r"====> Test set loss: \d+\.\d{4}\n", out), out
    logits, mu, lv = LC.vae_logits(O.OracleVAE(cs.params), cs.ip, cs.idx, cs.val, eps)
    want = LC.reference_test_loss(LC.row_bce(logits, cs.ip, cs.idx, cs.val, tiny=0.0), LC.row_kl(mu, lv), LC.N, LC.MAX_BATCH)
    print("last_test_loss", m.last_test_loss, "the reference formula on the oracle", want)
    np.testing.assert_allclose(m.last_test_loss, want, rtol=2e-5)
    assert "{:.4f}".format(m.last_test_loss) in out
    torch.manual_seed(9)
    np.testing.assert_allclose(m.eval_loss(X), want, rtol=2e-5)


@pytest.mark.parametrize("kind", ["categorical_native", "bridged"])
def test_eval_loss_behind_conditions_follows_the_routes_of_predict(kind):
    """A device-native CategoricalCondition(reduce='sum') rides in the call; any other plugin goes encode -> encode_impose ->
    decode_loss.  Either way: the host loss of the model's own predict() with the same conditions."""
    from aaerec import condition as C
    from aaerec.aae import AdversarialAutoEncoder
    rng = np.random.RandomState(5)
    torch.manual_seed(5)
    np.random.seed(5)
    X = sp.random(150, 400, density=0.03, format="csr", random_state=rng, dtype=np.float32)
    X.data[:] = 1.0

    class ConstBias(C.ConditionalBiasing):
        def encode(self, inputs):
            return torch.as_tensor(np.asarray(inputs), dtype=torch.float32, device="cuda")
    if kind == "categorical_native":
        conds = C.ConditionList([("authors", C.CategoricalCondition(8, use_cuda=True, reduce="sum", lr=0.01))])
        data = conds.fit_transform([[["a%d" % rng.randint(1, 30) for _ in range(rng.randint(1, 4))] for _ in range(150)]])
    else:
        conds = C.ConditionList([("b", ConstBias())])
        data = [0.1 * rng.standard_normal((150, 16)).astype(np.float32)]
    m = AdversarialAutoEncoder(n_hidden=40, n_code=16, n_epochs=2, batch_size=50, gen_lr=0.01, reg_lr=0.001, conditions=conds,
                               verbose=False)
    m.fit(X, condition_data=data)
    assert m._is_device_native() == (kind == "categorical_native")
    got = m.eval_loss(X, condition_data=data)
    pred = m.predict(X, condition_data=data)
    want = _host_mean_bce(pred, X)
    tol = _surface_tol(pred, X) + (LC.TOL_LOSS + 2.0 ** -23) * want
    print(f"{kind}: eval_loss {got!r}, host {want!r}, difference {abs(got - want):.3g} of {tol:.3g}")
    assert abs(got - want) <= tol
    rows = m.eval_loss(X, condition_data=data, per_row=True)
    assert rows.dtype == np.float64 and rows.shape == (150,) and abs(rows.sum() / (150 * 400) - got) <= 1e-12 * got
    # other targets: the inputs plus held-out items move the loss
    Y = (X + sp.random(150, 400, density=0.01, format="csr", random_state=rng, dtype=np.float32)).tocsr()
    Y.data[:] = np.minimum(Y.data, 1.0)
    assert m.eval_loss(X, condition_data=data, targets=Y) > got


def test_argument_errors_name_the_call():
    from aaerec._hip import AaeHipError, DeviceCSR
    from aaerec.aae import AutoEncoder
    cs = LC.AaeCase(*LC.AAE_CASES[0])
    dev = cs.device()
    other = DeviceCSR(sp.csr_matrix((LC.ROWS, LC.N - 1), dtype=np.float32), dev.device)
    with pytest.raises(ValueError, match="predict_loss"):
        dev.predict_loss(cs.csr, 0, 10, targets=other)
    cap = dev.loss_max_rows()
    big = DeviceCSR(sp.csr_matrix((cap + 1, LC.N), dtype=np.float32), dev.device)
    with pytest.raises(AaeHipError, match="aae_predict_loss"):
        dev.predict_loss(big, 0, cap + 1)
    with pytest.raises(AaeHipError, match="aae_vae_predict_loss"):
        dev.vae_predict_loss(cs.csr, 0, 10)                      # not a VAE handle
    vs = LC.VaeCase(*LC.VAE_CASES[0])
    vdev = vs.device()                                           # rng_mode inject
    with pytest.raises(AaeHipError, match="aae_vae_predict_loss.*eps"):
        vdev.vae_predict_loss(vs.csr, 0, 10)
    m = AutoEncoder(n_hidden=24, n_code=8, n_epochs=1, batch_size=50, verbose=False)
    X = sp.csr_matrix((cs.val, cs.idx, cs.ip), shape=(LC.ROWS, LC.N))
    m.fit(X)
    with pytest.raises(ValueError, match="eval_loss: targets has shape"):
        m.eval_loss(X, targets=sp.csr_matrix((LC.ROWS, LC.N + 1), dtype=np.float32))
