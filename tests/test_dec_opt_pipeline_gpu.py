"""The deferred launch of the split output layer (csrc/dec_crit_x3.h dec_opt_x3_kernel) requests a tile's four streams -
stored dL/dlogits, V3a and both Adam moments - a whole tile ahead into a second register set, and keeps the third bf16
term of the resident dh2 fragments in LDS.  A tile's arithmetic depends neither on the workgroup that takes it nor on the
iteration it is taken in, so the results must be BITWISE the same for every width of the launch (aae_set_split): a wrong
rotation of the register sets, a wrong last iteration (the workgroup's last tile requests nothing) or a stale set of
moments each break exactly that.

Widths: 1 (one workgroup walks every tile: the steady state and the final iteration), 2, 4 (of 6 tiles: two workgroups
with two tiles, two with one), 6 (the prologue's requests only) and 64 (more workgroups than tiles).  Shapes: 167 items
(6 tiles, the last with 7 items) and 32 (one tile); hidden 200 (13 column blocks: waves 10..15 split the item halves) and
100 (7); batches of 1, 100, 109 and 112 rows: 112 is the kernels' row block, 109 the largest batch the library sends through
them (csrc/abi_chains.h output_form: the single-launch form's LDS image of dh2 has to fit 160 KB, at any hidden
width) - a batch of 112 takes the three-kernel path, where the width must change nothing either.  Three consecutive aae_output_layer_step calls on
seeded parameters with non-zero Adam moments loaded, so that the moments, the late join and the operand copies are live."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 6, 64)
STEPS = 3
FUSED_ROWS = 109     # 4 * (212 * rows + 17664) bytes <= 160 KB (dec_fused_lds_bytes): batches beyond it never reach the deferred launch


@functools.lru_cache(maxsize=None)
def _inputs(N, h, B):
    """Seeded parameters, moments, batches and last hidden activations of a case (host arrays, shared by every width)."""
    from oracle.dense_torch_port import init_params
    from tools.synth import throughput_corpus
    rng = np.random.default_rng(1000 * N + 10 * h + B)
    X = throughput_corpus(STEPS * B, N, median_len=min(12, max(1, N // 4)), max_len=min(60, N - 1), seed=3)
    params = init_params(N, h, 50, seed=1)
    mom = dict(m_w=(rng.standard_normal((N, h)) * 1e-4).astype(np.float32), v_w=(rng.random((N, h)) * 1e-7).astype(np.float32),
               m_b=(rng.standard_normal(N) * 1e-4).astype(np.float32), v_b=(rng.random(N) * 1e-7).astype(np.float32))
    dh2 = [rng.random((B, h)).astype(np.float32) * (rng.random((B, h)) > 0.3) for _ in range(STEPS)]   # (post-ReLU: zeros among them)
    return X, params, mom, dh2


def _run(N, h, B, width, dtype="f32", optimizer="adam", unfused=False):
    """Three output-layer steps at one width of the deferred launch -> (weight, bias, m_w, v_w, m_b, v_b) of dec.lin3."""
    from aaerec import _hip
    from aaerec._hip import HipAAE, DeviceCSR
    X, params, mom, dh2 = _inputs(N, h, B)
    m = HipAAE(N, h, 50, max_batch=B, rng_mode="inject", dtype=dtype, optimizer=optimizer, unfused_decoder=unfused)
    m.load_params(params)
    m.load_adam(_hip.O_DEC, 3, mom["m_w"], mom["v_w"], mom["m_b"], mom["v_b"], step=5)
    if not unfused:
        m.set_split(width)
        m.profile_enable(True, kernels=(_hip.K_DEC_OPT,))
    csr = DeviceCSR(X, m.device)
    for s in range(STEPS):
        rows = m.dh2_rows(B)
        rows[:, :h].copy_(torch.from_numpy(dh2[s]))
        rows[:, h] = 1.0
        m.output_layer_step(csr, s * B, B)
    torch.cuda.synchronize()
    if not unfused:
        m.sync()
        m.profile_enable(False)
        assert m.profile_read(_hip.K_DEC_OPT)[1] == (STEPS if B <= FUSED_ROWS else 0), "deferred launches of the three steps"
    sd, st = m.state_dict(), m.adam_state("dec")
    out = (sd["dec.lin3.weight"], sd["dec.lin3.bias"], st["lin3.weight"][0], st["lin3.weight"][1], st["lin3.bias"][0], st["lin3.bias"][1])
    m.close()
    return tuple(np.array(a, copy=True) for a in out)


NAMES = ("dec.lin3.weight", "dec.lin3.bias", "m of the weight", "v of the weight", "m of the bias", "v of the bias")


def _same_bits_at_every_width(N, h, B, **kw):
    base = _run(N, h, B, WIDTHS[0], **kw)
    assert np.isfinite(base[0]).all()
    _, params, mom, _ = _inputs(N, h, B)
    assert not np.array_equal(base[0], params["dec.lin3.weight"]), "the steps changed nothing"
    if kw.get("optimizer", "adam") == "adam":
        assert not np.array_equal(base[2], mom["m_w"]) and not np.array_equal(base[3], mom["v_w"])
    for w in WIDTHS[1:]:
        got = _run(N, h, B, w, **kw)
        for name, a, b in zip(NAMES, base, got):
            assert np.array_equal(a, b), (f"{name}: width {w} differs from width {WIDTHS[0]} at N={N} h={h} B={B} {kw}: "
                                          f"{int((a != b).sum())} cells, max |diff| {float(np.abs(a - b).max()):.3g}")
    return base


@pytest.mark.parametrize("B", [1, 100, 109, 112])
@pytest.mark.parametrize("h", [200, 100])
@pytest.mark.parametrize("N", [167, 32])
def test_every_width_of_the_deferred_launch_gives_the_same_bits(N, h, B, monkeypatch):
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    _same_bits_at_every_width(N, h, B)


def test_every_width_gives_the_same_bits_on_the_one_term_instantiation(monkeypatch):
    """bf16 mode: the one-term instantiation (both register sets resident, no LDS block)."""
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    _same_bits_at_every_width(167, 100, 100, dtype="bf16")


def test_every_width_gives_the_same_bits_with_sgd(monkeypatch):
    """SGD: the moments are requested and never stored (their stores name an offset beyond the descriptor): they must come
    back as they were loaded, at every width."""
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    base = _same_bits_at_every_width(167, 200, 100, optimizer="sgd")
    mom = _inputs(167, 200, 100)[2]
    assert np.array_equal(base[2], mom["m_w"]) and np.array_equal(base[3], mom["v_w"])


@pytest.mark.parametrize("N,h,B", [(167, 200, 100), (167, 100, 109), (32, 200, 1)])
def test_deferred_launch_equals_the_three_kernel_path(N, h, B, monkeypatch):
    """The same three steps on the three-kernel path (the handle's unfused-decoder switch), at the tolerances of the forced-path
    comparison tests/test_parity_abi_gpu.py::test_fused_decoder_equals_unfused_path_at_headline_width: parameters atol 2e-6,
    first moments atol 1e-9 / rtol 1e-4, second moments atol 1e-13 / rtol 1e-4."""
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    got = _run(N, h, B, 4)
    want = _run(N, h, B, 0, unfused=True)
    for i in (0, 1):
        np.testing.assert_allclose(got[i], want[i], atol=2e-6, rtol=0, err_msg=NAMES[i])
    for i in (2, 4):
        np.testing.assert_allclose(got[i], want[i], atol=1e-9, rtol=1e-4, err_msg=NAMES[i])
    for i in (3, 5):
        np.testing.assert_allclose(got[i], want[i], atol=1e-13, rtol=1e-4, err_msg=NAMES[i])
