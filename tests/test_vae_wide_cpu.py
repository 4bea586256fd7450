"""A VAE handle whose decoder input [z | condition | 1] is wider than one 208-column slot of the layer-chain kernel (the
reference drivers' CONDITIONS: 383 columns, 983 in eval/mpd/mpd.py): what can be checked without a GPU - the sizes
aae_arena_bytes accepts and refuses, VAE.__init__'s ValueError in front of handle creation, and the oracle's replay of the
two fixtures the GPU tests (test_vae_wide_gpu.py) hold the kernels to."""
import ctypes

import numpy as np
import pytest

from golden_util import Fixture
from oracle import aae_oracle as O
from vae_wide_cases import W_MAX, WIDE_FIXTURES, VAE_NAMES, build_wide_oracle

TOL_PARAM = 5e-6        # test_oracle_golden.py's tolerances, unchanged


def _arena(lib, _hip, **kw):
    cfg = _hip.AaeConfig()
    cfg.abi_version = _hip.ABI_VERSION
    cfg.n_items, cfg.n_hidden, cfg.n_code, cfg.max_batch, cfg.max_nnz = 5000, 100, 50, 100, 25000
    cfg.model_kind = _hip.MODEL_VAE
    for k, v in kw.items():
        setattr(cfg, k, v)
    n = ctypes.c_size_t()
    rc = lib.aae_arena_bytes(ctypes.byref(cfg), ctypes.byref(n))
    return rc, n.value, lib.aae_last_error().decode()


def test_arena_bytes_takes_the_drivers_widths_and_names_the_bound_beyond_it():
    from aaerec import _hip
    lib = _hip.load_library()
    rc, base, _ = _arena(lib, _hip, cond_inc=0)
    assert rc == 0
    for inc in (300, 932):                      # main.py / aminer.py / econis.py: 332 with n_code 50 -> 383; mpd.py: 983
        rc, n, msg = _arena(lib, _hip, cond_inc=inc)
        assert rc == 0, msg
        # fc3 [100][50 + inc + 1] with both Adam moments, and zc / gzc [100 rows][50 + inc + 1]: at least the columns added
        assert n - base >= 4 * (3 * 100 * inc + 2 * 100 * inc), (inc, n - base)
    rc, n, msg = _arena(lib, _hip, cond_inc=W_MAX - 1 - 50)
    assert rc == 0, msg                         # exactly W_MAX columns
    rc, _, msg = _arena(lib, _hip, cond_inc=W_MAX - 50)
    assert rc == -1 and str(W_MAX) in msg and "n_code + cond_inc + 1" in msg, msg
    rc, _, msg = _arena(lib, _hip, n_code=105, cond_inc=0)
    assert rc == -1 and "2 * n_code <= 208" in msg, msg
    rc, _, msg = _arena(lib, _hip, n_hidden=208, cond_inc=300)
    assert rc == -1 and "n_hidden <= 207" in msg, msg
    # the AAE family keeps its own rule: any width is laid out (beyond 416 columns it runs layer by layer)
    rc, _, msg = _arena(lib, _hip, model_kind=_hip.MODEL_AAE, cond_inc=2000)
    assert rc == 0, msg


def test_vae_init_names_the_bound_before_it_asks_for_a_handle(monkeypatch):
    from aaerec import _hip, vae

    class Wide:
        def __init__(self, inc):
            self.inc = inc

        def size_increment(self):
            return self.inc

        def __bool__(self):
            return True

    def no_handle(*a, **k):
        raise AssertionError("the width check must sit in front of handle creation")
    monkeypatch.setattr(_hip, "HipAAE", no_handle)
    assert vae.DEC_IN_MAX == W_MAX
    with pytest.raises(ValueError, match=str(W_MAX)):
        vae.VAE(300, 300, n_code=50, conditions=Wide(W_MAX - 50))
    with pytest.raises(ValueError, match=str(W_MAX)):
        vae.VAE(300, 300, n_code=10, conditions=Wide(5000))


@pytest.mark.parametrize("name", WIDE_FIXTURES)
def test_oracle_reproduces_the_reference_on_the_wide_fixtures(name):
    """VAE.partial_fit / predict of the reference behind ConditionList([constant block, CategoricalCondition(32)]) with the
    recorded eps: loss, all five Linears, their Adam moments where the fixture holds them, the embedding table, predict."""
    fx = Fixture(name)
    assert fx.cfg["c"] + fx.cfg["cond_inc"] + 1 == {"step_vae_wide": 343, "step_vae_wide5": 943}[name]
    m = build_wide_oracle(fx)
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        loss = m.partial_fit(ip, idx, val, fx.z[f"step{s}.eps"], fx.cond_inputs(s))
        np.testing.assert_allclose(loss, fx.z[f"step{s}.losses"][0], rtol=5e-6)
        for n in VAE_NAMES:
            for t in ("weight", "bias"):
                k = f"{n}.{t}"
                np.testing.assert_allclose(m.p[k], fx.z[f"step{s}.{k}"], atol=TOL_PARAM, rtol=0, err_msg=f"{name} {s} {k}")
                if f"step{s}.A.{k}.m" in fx.z.files:
                    assert m.opt.t[k] == float(fx.z[f"step{s}.A.{k}.t"])
                    np.testing.assert_allclose(m.opt.m[k], fx.z[f"step{s}.A.{k}.m"], atol=2e-8, rtol=2e-4)
                    np.testing.assert_allclose(m.opt.v[k], fx.z[f"step{s}.A.{k}.v"], atol=1e-12, rtol=2e-4)
        np.testing.assert_allclose(m.conditions[1].params["w"], fx.z[f"step{s}.cond.embedding"], atol=TOL_PARAM)
    assert f"step{fx.steps - 1}.A.fc3.weight.m" in fx.z.files
    ip, idx, val = fx.batch(0, prefix="predict")
    out = m.predict(ip, idx, val, fx.z["predict.eps"], fx.cond_inputs(0, prefix="predict"))
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=2e-6)
    assert isinstance(m.conditions[0], O.ConcatConst)


@pytest.mark.parametrize("name", WIDE_FIXTURES)
def test_the_wide_fixtures_hold_no_element_that_rounding_alone_moves(name, monkeypatch):
    """The second screen of a wide fixture's seed (tools/gen_golden.py): the oracle restated in float64 - exact arithmetic, to
    the eye of a float32 reference - stays within the same TOL_PARAM of the reference's parameters and table.  Adam's first
    step turns a gradient near its eps into up to lr of parameter whatever the arithmetic; a fixture that holds such an
    element (one fc3 element of the 943-column case at seed 52: 1.25e-5 between the reference and exact arithmetic) pins
    the reference's rounding, and no other implementation can be held to it."""
    monkeypatch.setattr(O, "f32", np.float64)
    fx = Fixture(name)
    m = build_wide_oracle(fx)
    worst = 0.0
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        m.partial_fit(ip, idx, val, fx.z[f"step{s}.eps"], fx.cond_inputs(s))
        for n in VAE_NAMES:
            for t in ("weight", "bias"):
                worst = max(worst, float(np.abs(m.p[f"{n}.{t}"] - fx.z[f"step{s}.{n}.{t}"]).max()))
        worst = max(worst, float(np.abs(m.conditions[1].params["w"] - fx.z[f"step{s}.cond.embedding"]).max()))
    print(f"{name}: the reference against exact arithmetic, worst parameter element {worst:.3g}")
    assert m.p["fc3.weight"].dtype == np.float64
    assert worst <= TOL_PARAM
