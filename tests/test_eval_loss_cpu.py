"""What the held-out loss (csrc/loss_eval.h; aae_predict_loss / aae_decode_loss / aae_vae_predict_loss / aae_vae_decode_loss)
needs no device for: the host restatement the GPU tests hold the kernels to (tests/loss_cases.py row_bce / row_kl) is pinned
to torch and to the oracle FIRST, every case's oracle logits keep clear of the 24 ln 2 cut-off, and the library declares,
binds and exports the six calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_CALLS = ("aae_predict_loss", "aae_decode_loss", "aae_vae_predict_loss", "aae_vae_decode_loss", "aae_loss_max_rows",
              "aae_vae_loss_max_rows")


def _torch_rows(scores32, T, tiny):
    """F.binary_cross_entropy(scores + tiny, T + tiny, reduction='none').sum(1): fp32 cells as the reference forms them, the
    row sums in float64."""
    x, t = torch.as_tensor(scores32), torch.as_tensor(T)
    if tiny:
        x, t = x + tiny, t + tiny
    return torch.nn.functional.binary_cross_entropy(x, t, reduction="none").double().sum(1).numpy()


@pytest.mark.parametrize("case", LC.AAE_CASES, ids=[c[0] for c in LC.AAE_CASES])
def test_the_restatement_equals_torch_on_the_aae_oracle(case):
    """row_bce of OracleAAE's logits against torch's BCE of its fp32 scores (+ 1e-12 on both sides, aae.py:693-695), per row
    within the per-row form of golden_util.bce_quantisation_bound.  The case states: no logit within ZONE of the cut-off."""
    from oracle.aae_oracle import sigmoid
    cs = LC.AaeCase(*case)
    assert LC.zone_clear(cs.logits), "choose another seed: an oracle logit lies within ZONE of 24 ln 2"
    got = LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval)
    want = _torch_rows(sigmoid(cs.logits), LC.dense_targets(cs.tip, cs.tidx, cs.tval), 1e-12)
    bound = LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval)
    err = np.abs(got - want)
    print(f"{cs.name}: row sums {got.min():.4g} .. {got.max():.4g}; max |restatement - torch| = {err.max():.3g},"
          f" largest share of its row's bound = {(err / bound).max():.3g}")
    assert np.all(err <= bound), (float((err / bound).max()), int(np.argmax(err / bound)))
    if case[4]:         # the saturated case: the 100s are in every row's sum, on zero targets and on non-zero ones
        L = np.asarray(cs.logits)
        T = LC.dense_targets(cs.tip, cs.tidx, cs.tval)
        for b in range(LC.ROWS):
            assert (L[b] >= LC.BCE_CUT).sum() >= 5 and got[b] >= 500.0, b
            if b != LC.EMPTY_ROW:
                assert ((L[b] >= LC.BCE_CUT) & (T[b] > 0)).any() and ((L[b] < -20.0) & (T[b] > 0)).any(), b


@pytest.mark.parametrize("case", LC.VAE_CASES, ids=[c[0] for c in LC.VAE_CASES])
def test_the_restatement_equals_torch_on_the_vae_oracle(case):
    """The same for OracleVAE, whose reference is nn.BCELoss without the 1e-12 (vae.py:133-136): tiny = 0 on both sides; and
    the 1e-12 form the kernels charge a VAE handle with lies within a thousandth of the bound of it."""
    cs = LC.VaeCase(*case)
    assert LC.zone_clear(cs.logits), "choose another seed: an oracle logit lies within ZONE of 24 ln 2"
    scores = cs.ora.predict(cs.ip, cs.idx, cs.val, cs.eps, [cs.cond] if cs.inc else None)
    got = LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval, tiny=0.0)
    want = _torch_rows(scores, LC.dense_targets(cs.tip, cs.tidx, cs.tval), 0.0)
    bound = LC.row_bound(cs.logits, cs.tip, cs.tidx, cs.tval)
    err = np.abs(got - want)
    print(f"{cs.name}: max |restatement - torch| = {err.max():.3g}, largest share of its row's bound = {(err / bound).max():.3g}")
    assert np.all(err <= bound)
    assert np.all(np.abs(LC.row_bce(cs.logits, cs.tip, cs.tidx, cs.tval) - got) <= 1e-3 * bound)


@pytest.mark.parametrize("case", LC.VAE_CASES, ids=[c[0] for c in LC.VAE_CASES])
def test_the_kl_restatement_equals_the_oracles_step(case):
    """row_kl(mu, logvar) summed over a batch's rows is OracleVAE.partial_fit's last['kld'] for that batch (the step's KL is a
    function of the pre-step parameters)."""
    cs = LC.VaeCase(*case)
    n = LC.MAX_BATCH
    want_rows = LC.row_kl(cs.mu[:n], cs.lv[:n])
    cs.ora.partial_fit(cs.ip[:n + 1], cs.idx[:cs.ip[n]], cs.val[:cs.ip[n]], cs.eps[:n], [cs.cond[:n]] if cs.inc else None)
    np.testing.assert_allclose(want_rows.sum(), cs.ora.last["kld"], rtol=1e-12)


def test_the_library_exports_the_loss_calls_and_the_abi_version_stands():
    from aaerec import _build, _hip
    _build.build()                       # no-op when up to date; hipcc cross-compiles without a GPU
    header = open(os.path.join(ROOT, "include", "aaerec_hip.h")).read()
    declared = set(re.findall(r"^int\s+(aae_\w+)\s*\(", header, flags=re.M))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in LOSS_CALLS:
        assert name in declared, name
        assert name in _hip._PROTOS, name
        assert hasattr(lib, name), name
        assert _hip._PROTOS[name][0] is ctypes.c_int
    P, B, V = _hip._PROTOS, ctypes.POINTER(_hip.AaeBatch), ctypes.c_void_p
    # the arguments in the header's order: (handle, batch, cond, [eps, row0,] targets, row_bce, [row_kl,] stream) and the decode
    # form (handle, zc, zc_ld, batch, targets, row_bce, stream)
    assert P["aae_predict_loss"][1] == [V, B, V, B, V, V]
    assert P["aae_vae_predict_loss"][1] == [V, B, V, V, ctypes.c_int64, B, V, V, V]
    assert P["aae_decode_loss"][1] == P["aae_vae_decode_loss"][1] == [V, V, ctypes.c_int64, B, B, V, V]
    assert P["aae_loss_max_rows"][1] == P["aae_vae_loss_max_rows"][1] == P["aae_rank_full_max_rows"][1]
    assert re.search(r"aae_vae_predict_loss\(aae_handle h, const aae_batch\* batch, const float\* cond_dev, const float\* eps_dev, "
                     r"int64_t row0,\s+const aae_batch\* targets, double\* row_bce_dev, double\* row_kl_dev, void\* stream\)", header)
    assert re.search(r"aae_predict_loss\(aae_handle h, const aae_batch\* batch, const float\* cond_dev, const aae_batch\* targets, "
                     r"double\* row_bce_dev,\s+void\* stream\)", header)
    assert _hip.ABI_VERSION == 4 and _hip.load_library().aae_abi_version() == 4      # additive: the version stands


def test_every_autoencoder_and_its_recommender_offer_eval_loss():
    from aaerec.aae import AAERecommender, AdversarialAutoEncoder, AutoEncoder, DecodingRecommender
    from aaerec.dae import DAERecommender, DenoisingAutoEncoder
    from aaerec.vae import VAE, VAERecommender
    from aaerec._hip import HipAAE
    import inspect
    for cls in (AdversarialAutoEncoder, AutoEncoder, DenoisingAutoEncoder, VAE, AAERecommender, DAERecommender, VAERecommender,
                DecodingRecommender):
        assert callable(getattr(cls, "eval_loss", None)), cls.__name__
    for name in ("predict_loss", "decode_loss", "vae_predict_loss", "vae_decode_loss", "loss_max_rows"):
        assert callable(getattr(HipAAE, name, None)), name
    sig = inspect.signature(VAE.predict)
    assert list(sig.parameters)[1:] == ["X", "condition_data", "test_loss"] and sig.parameters["test_loss"].default is False
