"""The bag reductions of csrc/cond_bag.h without a GPU: the NumPy restatement (bag_cases.py) held to torch itself - what the
reference calls - and, wired into the oracle, to the reference's recorded runs; the device_native() decisions; the exported
symbols."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bag_cases as BC
from golden_util import Fixture

# test_oracle_golden.py's tolerances, unchanged
TOL_LOSS, TOL_PARAM = 2e-6, 5e-6


def _three_steps(seed, rows, width, dim, vocab, reduce, pad):
    c = BC.make_case(seed, rows, width, dim, vocab, reduce, pad)
    rng = np.random.default_rng(seed + 1000)
    idx = [c["idx"]] + [BC.make_idx(rng, rows, width, vocab, pad) for _ in range(2)]
    dout = [c["dout"]] + [BC.settle_mean_gradients(i, BC.grid(rng, (rows, dim)), vocab, pad, reduce) for i in idx[1:]]
    return c["table"], idx, dout


@pytest.mark.parametrize("reduce,sparse", [(r, s) for r in BC.NAMES for s in (False, True) if BC.torch_exists(r, s)],
                         ids=lambda x: BC.NAMES[x] if not isinstance(x, bool) else ("sparse_adam" if x else "adam"))
def test_restatement_equals_torch_for_three_steps(reduce, sparse):
    """nn.Embedding(padding_idx=0) + .mean(1) / .max(1)[0] and nn.EmbeddingBag(sum / mean / max, with and without padding_idx)
    under torch.optim.Adam / SparseAdam, three steps on the CPU.  Step 0 runs on the 1/8 grid (tie-free across rows, exact
    sums): encodes of sum and max bit for bit.  From step 1 on the tables hold what Adam made of them.
    (nn.EmbeddingBag(mode='max') has no sparse gradient: torch has nothing to hold that one combination to.)"""
    for pad in BC.PADS[reduce]:
        for si, (rows, width, dim, vocab) in enumerate([(1, 1, 1, 2), (3, 2, 7, 2), (5, 5, 9, 40), (17, 3, 8, 12)]):
            table, idx, dout = _three_steps(100 * reduce + si, rows, width, dim, vocab, reduce, pad)
            want_out, want_p, want_m, want_v = BC.torch_steps(table, idx, reduce, pad, dout, 1e-2, sparse)
            p, m, v = table.copy(), np.zeros_like(table), np.zeros_like(table)
            for t in range(3):
                out = BC.bag_step(p, m, v, idx[t], reduce, pad, dout[t], 1e-2, t + 1, sparse)
                tag = f"{BC.NAMES[reduce]} pad {pad} shape {(rows, width, dim, vocab)} step {t}"
                if t == 0 and reduce in (BC.SUM, BC.MAX_PAD0, BC.MAX):
                    assert np.array_equal(out, want_out[t]), tag
                else:
                    np.testing.assert_allclose(out, want_out[t], rtol=3e-7, atol=1e-7, err_msg=tag)
            np.testing.assert_allclose(m, want_m, atol=2e-8, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(v, want_v, atol=1e-12, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(p, want_p, atol=1e-5, rtol=0, err_msg=tag)
            if pad >= 0:
                assert np.array_equal(p[pad], table[pad]), tag + ": the padding row moved"


def test_restatement_skips_indices_outside_the_table():
    table = BC.make_table(np.random.default_rng(5), 6, 4, -1)
    idx = np.array([[1, -3, 2], [9, 9, 9], [4, 6, 4]])
    clean = np.array([[1, 5, 2], [5, 5, 5], [4, 5, 4]])               # the same bags with row 5 as the padding row
    for reduce in BC.NAMES:
        a, b = BC.bag_encode(table, idx, reduce, -1)[0], BC.bag_encode(table, clean, reduce, 5)[0]
        assert np.array_equal(a, b), BC.NAMES[reduce]
    assert not BC.bag_encode(table, idx, BC.MAX, -1)[0][1].any()         # an empty bag gives 0


@pytest.mark.parametrize("name", list(BC.BAG_FIXTURES))
def test_oracle_with_the_restatement_reproduces_the_reference(name):
    """The reference's recorded runs (tools/gen_golden.py bagcond), replayed by the oracle with the restatement as its condition."""
    fx = Fixture(name)
    m = BC.build_oracle(fx)
    cond = m.conditions[0]
    worst = 0.0
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        if fx.cfg.get("vae"):
            loss = m.partial_fit(ip, idx, val, fx.z[f"step{s}.eps"], fx.cond_inputs(s))
            np.testing.assert_allclose(loss, fx.z[f"step{s}.losses"][0], rtol=5e-6)
            want = {f"{n}.{t}": fx.z[f"step{s}.{n}.{t}"] for n in ("fc1", "fc21", "fc22", "fc3", "fc4") for t in ("weight", "bias")}
        else:
            losses = m.partial_fit(ip, idx, val, fx.z[f"step{s}.z_real"], fx.masks(s), fx.cond_inputs(s))
            np.testing.assert_allclose(losses, fx.z[f"step{s}.losses"], rtol=TOL_LOSS, atol=1e-7, err_msg=f"{name} step {s}")
            want = fx.expected_params(s)
        for k, w in want.items():
            worst = max(worst, float(np.abs(m.p[k] - w).max()))
            np.testing.assert_allclose(m.p[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k}")
        worst = max(worst, float(np.abs(cond.params["w"] - fx.z[f"step{s}.cond.embedding"]).max()))
        np.testing.assert_allclose(cond.params["w"], fx.z[f"step{s}.cond.embedding"], atol=TOL_PARAM, err_msg=f"{name} table {s}")
        assert cond.t == float(fx.z[f"step{s}.cond.t"])
        np.testing.assert_allclose(cond.m, fx.z[f"step{s}.cond.m"], atol=1e-9, rtol=2e-5, err_msg=f"{name} m {s}")
        np.testing.assert_allclose(cond.v, fx.z[f"step{s}.cond.v"], atol=1e-13, rtol=5e-5, err_msg=f"{name} v {s}")
    print(f"{name}: worst parameter / table difference {worst:.3g}")
    ip, idx, val = fx.batch(0, prefix="predict")
    pc = fx.cond_inputs(0, prefix="predict")
    out = m.predict(ip, idx, val, fx.z["predict.eps"], pc) if fx.cfg.get("vae") else m.predict(ip, idx, val, pc)
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=2e-6)


def test_device_native_decisions_on_cpu_objects():
    """Every refusal the conditions document: a table that is not on that GPU, an unsupported option, too wide a table."""
    from aaerec import condition as C
    for kw in (dict(), dict(mode="sum"), dict(mode="max"), dict(max_norm=1.0), dict(scale_grad_by_freq=True),
               dict(mode="sum", sparse=True), dict(padding_idx=0)):
        bag = C.EmbeddingBagCondition(12, 8, **kw)
        assert bag.device_native("cuda:0") is False, kw                 # the weight is in host memory
    assert C.EmbeddingBagCondition(12, 300).device_native("cuda:0") is False
    # the same decisions with the table's placement taken out of the question: the module's options behind a weight that
    # says it lives on cuda:0
    def native(dim=8, device="cuda:0", **kw):
        bag = C.EmbeddingBagCondition(12, dim, **kw)
        mod = bag.embedding_bag
        bag.embedding_bag = SimpleNamespace(weight=SimpleNamespace(is_cuda=True, device=torch.device("cuda:0")), mode=mod.mode,
                                            max_norm=mod.max_norm, scale_grad_by_freq=mod.scale_grad_by_freq, sparse=mod.sparse,
                                            padding_idx=mod.padding_idx)
        return bag.device_native(device)
    assert native() and native(mode="sum") and native(mode="max") and native(padding_idx=0) and native(dim=256)
    assert not native(max_norm=1.0) and not native(scale_grad_by_freq=True) and not native(mode="sum", sparse=True)
    assert not native(dim=257)
    assert not native(device="cuda:1")                                  # another GPU's table
    for reduce in (None, "sum", "mean", "max"):
        cat = C.CategoricalCondition(8, use_cuda=False, reduce=reduce)
        assert not cat.device_native("cuda:0")                          # not fitted: no table
        cat.fit([["a", "b"], ["b"]] if reduce else ["a", "b", "b"])
        assert not cat.device_native("cuda:0")                          # the table is in host memory
    assert not C.CategoricalCondition(8, use_cuda=False, reduce="max", max_norm=1.0).fit([["a"]]).device_native("cuda:0")
    assert C.EmbeddingBagCondition(12, 8).padded_width(np.zeros((4, 3), dtype=np.int64)) == 3
    assert C.EmbeddingBagCondition(12, 8).padded_width([[1, 2], [3, 4]]) == 2


def test_library_exports_the_bag_calls_and_the_abi_version_stands():
    import os
    import re
    from aaerec import _hip
    lib = _hip.load_library()
    with open(os.path.join(BC.ROOT, "include", "aaerec_hip.h")) as fh:
        text = fh.read()
    for name in ("aae_bag_encode", "aae_bag_update"):
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
        decl = text[text.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_hip._PROTOS[name][1]), name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    enum = re.search(r"enum \{ AAE_BAG_SUM = 0, AAE_BAG_MEAN_WIDTH = 1, AAE_BAG_MEAN_COUNT = 2, AAE_BAG_MAX_PAD0 = 3, AAE_BAG_MAX = 4 \}", text)
    assert enum and (_hip.BAG_SUM, _hip.BAG_MEAN_WIDTH, _hip.BAG_MEAN_COUNT, _hip.BAG_MAX_PAD0, _hip.BAG_MAX) == (0, 1, 2, 3, 4)
    assert (BC.SUM, BC.MEAN_WIDTH, BC.MEAN_COUNT, BC.MAX_PAD0, BC.MAX) == (0, 1, 2, 3, 4)
    from aaerec.condition import EmbeddingBagCondition
    assert EmbeddingBagCondition._BAG_MODES == {"sum": _hip.BAG_SUM, "mean": _hip.BAG_MEAN_COUNT, "max": _hip.BAG_MAX}
    assert "enum { AAE_CAT_SUM = 0, AAE_CAT_MEAN = 1 };" in text          # aae_cat_* keep their values
    p = 0x1000                                                          # pointers nothing may dereference: the checks come first
    S = None
    assert lib.aae_bag_encode(p, 12, 300, p, 4, 3, 0, -1, p, 300, S) != 0          # dim > 256
    assert lib.aae_bag_encode(p, 12, 8, p, 4, 3, 5, -1, p, 8, S) != 0              # unknown reduce
    assert lib.aae_bag_encode(p, 12, 8, p, 4, 3, 0, 12, p, 8, S) != 0              # padding_idx outside the table
    assert lib.aae_bag_encode(p, 12, 8, p, 4, 3, 0, -1, p, 7, S) != 0              # out_ld < dim
    assert lib.aae_bag_update(p, p, p, None, 12, 8, p, 4, 3, 4, -1, p, 8, 0, 1e-3, 1, S) != 0     # max without a scratch
    assert lib.aae_bag_update(p, p, p, None, 12, 8, p, 4, 3, 0, -1, p, 8, 1, 1e-3, 1, S) != 0     # dense Adam without one
    assert lib.aae_bag_update(p, p, p, p, 12, 8, p, 4, 3, 0, -1, p, 8, 1, 1e-3, 0, S) != 0        # step counts from 1
