"""max_norm and scale_grad_by_freq of the trainable conditions without a GPU: the NumPy restatement (bag_opt_cases.py) held to
CPU torch where CPU torch is right, the one place where it is not, the device_native() decisions over the option
combinations, the data-parallel predicate and the argument checks of the new entry points."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import bag_cases as BC
import bag_opt_cases as OC

f32 = np.float32
EINVAL = -1                 # include/aaerec_hip.h: AAE_EINVAL


# ---- max_norm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bag", [False, True], ids=["embedding", "embedding_bag"])
@pytest.mark.parametrize("norm_type", OC.NORM_TYPES, ids=["l1", "l2", "inf"])
def test_renorm_restatement_equals_torch(norm_type, bag):
    """The float32 restatement (the kernels' order) and torch's own renorm on the CPU, both within the bound of the float64
    restatement; rows the input does not name keep their bits; on the grid the row exactly at max_norm does not move."""
    for si, (rows, width, dim, vocab) in enumerate([(1, 1, 1, 2), (3, 2, 7, 2), (5, 5, 65, 40), (17, 3, 256, 40)]):
        for on_grid in (True, False):
            table, idx, max_norm, at = OC.renorm_case(10 * si + on_grid, rows, width, dim, vocab, 0, norm_type, on_grid)
            valid = np.where((idx >= 0) & (idx < vocab), idx, 0)            # (torch raises on an index outside the table)
            want64 = table.astype(np.float64)
            OC.renorm(want64, valid, max_norm, norm_type, np.float64)
            got = table.copy()
            scaled = OC.renorm(got, valid, max_norm, norm_type)
            ref = OC.torch_renorm(table, valid, max_norm, norm_type, bag)
            bound = OC.renorm_bound(table, dim, max_norm)
            tag = f"p {norm_type} shape {(rows, width, dim, vocab)} grid {on_grid}"
            assert (np.abs(got - want64) <= bound).all(), tag
            assert (np.abs(ref - want64) <= bound).all(), tag + " (torch)"
            unnamed = np.setdiff1d(np.arange(vocab), OC.named_rows(valid, vocab))
            assert np.array_equal(got[unnamed], table[unnamed]) and np.array_equal(ref[unnamed], table[unnamed]), tag
            if at >= 0:
                assert at not in scaled and np.array_equal(got[at], table[at]) and np.array_equal(ref[at], table[at]), tag
            if vocab == 40:
                assert scaled and len(scaled) < len(OC.named_rows(valid, vocab)), tag + ": rows above and below max_norm"


def test_renorm_scales_a_row_once_and_the_padding_row_too():
    """The issue's two observations, on torch and on the restatement: a row named twice in a bag and again in another is
    scaled once; padding_idx=0, an input naming index 0 and max_norm=0.5 leave row 0 with norm 0.5."""
    rng = np.random.default_rng(3)
    table = (rng.standard_normal((5, 6)) * 4).astype(f32)
    idx = np.array([[2, 2, 0], [2, 1, 1]])
    once = table.copy()
    for j in (0, 1, 2):
        once[j] = once[j] * (f32(0.5) / (np.linalg.norm(once[j].astype(np.float64)).astype(f32) + f32(1e-7)))
    got = table.copy()
    assert OC.renorm(got, idx, 0.5, 2.0) == [0, 1, 2]
    np.testing.assert_allclose(got, once, rtol=1e-6)
    for mod in (nn.Embedding(5, 6, padding_idx=0, max_norm=0.5), nn.EmbeddingBag(5, 6, padding_idx=0, max_norm=0.5, mode="sum")):
        with torch.no_grad():
            mod.weight.copy_(torch.from_numpy(table))
        mod(torch.from_numpy(idx))
        w = mod.weight.detach().numpy()
        np.testing.assert_allclose(w, once, rtol=1e-6)
        np.testing.assert_allclose(np.linalg.norm(w[0]), 0.5, rtol=1e-6)            # the padding row, renormalised
        assert np.array_equal(w[3:], table[3:])


# ---- scale_grad_by_freq -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", [BC.SUM, BC.MEAN_WIDTH, BC.MAX_PAD0], ids=["sum", "mean", "max"])
@pytest.mark.parametrize("max_norm", [None, 2.5], ids=["freq", "freq_max_norm"])
def test_frequency_scaling_equals_torch_embedding_for_three_steps(reduce, max_norm):
    """nn.Embedding(sparse=False, scale_grad_by_freq=True) + .sum(1) / .mean(1) / .max(1)[0] under torch.optim.Adam, three
    steps on the CPU (its dense backward is right), with and without max_norm, at test_cond_bag_cpu.py's tolerances."""
    for pad in (-1, 0) if reduce == BC.SUM else (0,):
        for si, (rows, width, dim, vocab) in enumerate([(1, 1, 1, 2), (3, 2, 7, 2), (5, 5, 9, 40), (17, 3, 8, 12)]):
            c = BC.make_case(300 + 10 * reduce + si, rows, width, dim, vocab, reduce, pad)
            rng = np.random.default_rng(si)
            idx = [c["idx"]] + [BC.make_idx(rng, rows, width, vocab, pad) for _ in range(2)]
            dout = [c["dout"]] + [BC.grid(rng, (rows, dim)) for _ in range(2)]
            p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
            outs = []
            for t in range(3):
                seen = p.copy()                                 # the table the step's lookup sees: renormalised
                if max_norm is not None:
                    OC.renorm(seen, idx[t], max_norm, 2.0)
                dout[t] = OC.settle_gradients(seen, idx[t], dout[t], reduce, pad)
                outs.append(OC.step(p, m, v, idx[t], reduce, pad, dout[t], 1e-2, t + 1, max_norm=max_norm, by_freq=True))
            want_out, want_p, want_m, want_v = OC.torch_embedding_steps(c["table"], idx, reduce, pad, dout, 1e-2, max_norm=max_norm,
                                                                         by_freq=True)
            tag = f"{BC.NAMES[reduce]} pad {pad} shape {(rows, width, dim, vocab)}"
            for t in range(3):
                np.testing.assert_allclose(outs[t], want_out[t], rtol=3e-6, atol=1e-6, err_msg=f"{tag} step {t}")
            np.testing.assert_allclose(m, want_m, atol=2e-8, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(v, want_v, atol=1e-12, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(p, want_p, atol=1e-5, rtol=0, err_msg=tag)


def test_cpu_embedding_bag_scales_by_the_wrong_count():
    """idx [[0, 1, 1], [1, 2, 0]], sum mode, dout = 1: every table row's gradient is (its count) / (its count) = 1.  CPU
    nn.Embedding's dense backward says so; CPU nn.EmbeddingBag's looks the count up by the ordinal of the unique index and
    returns something else, so it is no oracle for frequency scaling.  The restatement follows the definition."""
    idx = np.array([[0, 1, 1], [1, 2, 0]])
    table, dout = np.ones((3, 2), dtype=f32), np.ones((2, 2), dtype=f32)
    g, rows = OC.freq_grad(table, idx, BC.SUM, -1, dout)
    assert list(rows) == [0, 1, 2] and np.array_equal(g, np.ones((3, 2), dtype=f32))
    assert list(OC.counts(idx, 3)) == [2, 3, 1]
    emb = nn.Embedding(3, 2, scale_grad_by_freq=True)
    emb(torch.from_numpy(idx)).sum(1).backward(torch.ones(2, 2))
    assert np.array_equal(emb.weight.grad.numpy(), g)
    bag = nn.EmbeddingBag(3, 2, mode="sum", scale_grad_by_freq=True)
    bag(torch.from_numpy(idx)).backward(torch.ones(2, 2))
    print("CPU nn.EmbeddingBag(scale_grad_by_freq=True) gradient of column 0:", bag.weight.grad.numpy()[:, 0])


# ---- device_native ----------------------------------------------------------------------------------------------------------
_FAKE_W = SimpleNamespace(is_cuda=True, device=torch.device("cuda:0"))


def _bag_native(**kw):
    """EmbeddingBagCondition.device_native with the table's placement taken out of the question (test_cond_bag_cpu.py)."""
    from aaerec import condition as C
    bag = C.EmbeddingBagCondition(12, 8, **kw)
    mod = bag.embedding_bag
    bag.embedding_bag = SimpleNamespace(weight=_FAKE_W, mode=mod.mode, max_norm=mod.max_norm, norm_type=mod.norm_type,
                                        scale_grad_by_freq=mod.scale_grad_by_freq, sparse=mod.sparse, padding_idx=mod.padding_idx)
    return bag


def _cat_native(reduce="sum", sparse=True, **params):
    from aaerec import condition as C
    cat = C.CategoricalCondition(8, use_cuda=False, reduce=reduce, sparse=sparse, **params)
    cat.fit([["a", "b"], ["b"]] if reduce else ["a", "b", "b"])
    mod = cat.embedding
    cat.embedding = SimpleNamespace(weight=_FAKE_W, max_norm=mod.max_norm, norm_type=mod.norm_type,
                                    scale_grad_by_freq=mod.scale_grad_by_freq, sparse=mod.sparse, padding_idx=mod.padding_idx)
    return cat


def test_device_native_truth_table_over_the_options():
    """CategoricalCondition takes the options natively wherever torch accepts them.  EmbeddingBagCondition still refuses both
    keywords - test_cond_bag_cpu.py pins that refusal - although the kernels under it carry them (test_cond_bag_opts_gpu.py
    holds nn.EmbeddingBag's forms to torch at the kernel level)."""
    for mode in ("sum", "mean", "max"):
        assert _bag_native(mode=mode).device_native("cuda:0") is True
        for kw in (dict(max_norm=1.0), dict(max_norm=1.0, norm_type=1.0), dict(scale_grad_by_freq=True),
                   dict(scale_grad_by_freq=True, max_norm=1.0), dict(sparse=True)):
            assert _bag_native(mode=mode, **kw).device_native("cuda:0") is False, (mode, kw)
            assert _bag_native(mode=mode, **kw).has_table_options() is ("sparse" not in kw)
    with pytest.raises(ValueError):
        nn.EmbeddingBag(4, 2, mode="max", scale_grad_by_freq=True)(torch.tensor([[0, 1]]))
    for reduce in (None, "sum", "mean", "max"):
        for sparse in (True, False):
            kw = dict(reduce=reduce, sparse=sparse)
            assert _cat_native(**kw).device_native("cuda:0")
            assert _cat_native(max_norm=1.0, **kw).device_native("cuda:0")
            assert _cat_native(max_norm=1.0, norm_type=float("inf"), **kw).device_native("cuda:0")
            assert not _cat_native(max_norm=1.0, norm_type=3.0, **kw).device_native("cuda:0")
            # a sparse gradient scaled by frequency raises in torch's embedding_backward: only sparse=False is native;
            # reduce='max' over nn.Embedding(sparse=False) is legal
            assert _cat_native(scale_grad_by_freq=True, **kw).device_native("cuda:0") is (not sparse)
            assert _cat_native(scale_grad_by_freq=True, max_norm=2.0, **kw).device_native("cuda:0") is (not sparse)
            assert not _cat_native(_weight=torch.zeros(3, 8), **kw).device_native("cuda:0")      # any other keyword: bridged
    emb = nn.Embedding(4, 2, sparse=True, scale_grad_by_freq=True)
    with pytest.raises(RuntimeError):
        emb(torch.tensor([[0, 1]])).sum().backward()


def test_options_are_not_device_native_under_data_parallelism():
    """A rank encodes only its share of a batch: a renorm there would scale different rows on different ranks.  One
    predicate (condition.device_native_conditions) decides for AdversarialAutoEncoder and VAE."""
    from aaerec import condition as C
    from aaerec.aae import AdversarialAutoEncoder
    const = SimpleNamespace(constant_concat=True)
    for make, expect in ((lambda: _bag_native(mode="mean"), True),
                         (lambda: _cat_native(sparse=False, scale_grad_by_freq=True), False),
                         (lambda: _cat_native(sparse=False, max_norm=1.0, norm_type=1.0), False),
                         (lambda: _cat_native(max_norm=1.0), False), (lambda: _cat_native(), True)):
        conds = {"const": const, "table": make()}
        assert make().has_table_options() is (not expect)
        assert C.device_native_conditions(conds, "cuda:0") is True
        assert C.device_native_conditions(conds, "cuda:0", data_parallel=True) is expect
        assert C.device_native_conditions(conds, "cuda:1") is False
        for dp, want in ((None, True), (False, True), (True, expect), (object(), expect)):
            m = AdversarialAutoEncoder(conditions=C.ConditionList([("table", make())]), device="cuda:0", data_parallel=dp)
            assert m._is_device_native() is want, (dp, want)
    assert C.device_native_conditions({"x": SimpleNamespace()}, "cuda:0") is False       # a plugin without device_native
    assert not C.CategoricalCondition(8, use_cuda=False, max_norm=1.0).has_table_options()   # not fitted: no table yet


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_new_entry_points_check_their_arguments():
    import os
    from aaerec import _hip
    lib = _hip.load_library()
    with open(os.path.join(BC.ROOT, "include", "aaerec_hip.h")) as fh:
        text = fh.read()
    for name in ("aae_bag_renorm", "aae_bag_csr_renorm", "aae_bag_update_flags", "aae_bag_csr_update_flags"):
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
        decl = text[text.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_hip._PROTOS[name][1]), name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4                      # additive: the version stands
    assert "enum { AAE_BAG_NORM_INF = 0, AAE_BAG_NORM_L1 = 1, AAE_BAG_NORM_L2 = 2 };" in text
    assert "enum { AAE_BAG_SCALE_BY_FREQ = 1 };" in text
    assert _hip.BAG_NORM_TYPES == {float("inf"): 0, 1.0: 1, 2.0: 2} and _hip.BAG_SCALE_BY_FREQ == 1
    p, S = 0x1000, None                          # pointers nothing may dereference: the checks come first
    for max_norm, norm_type in ((0.0, 2), (-1.0, 2), (float("nan"), 2), (1e-60, 2), (1.0, 3), (1.0, -1)):
        assert lib.aae_bag_renorm(p, 12, 8, p, 4, 3, max_norm, norm_type, S) == EINVAL, (max_norm, norm_type)
        assert lib.aae_bag_csr_renorm(p, 12, 8, p, p, 4, 9, None, 0, 4, 9, max_norm, norm_type, p, 1 << 20, S) == EINVAL
    assert lib.aae_bag_renorm(p, 12, 300, p, 4, 3, 1.0, 2, S) == EINVAL            # dim > 256
    assert lib.aae_bag_renorm(None, 12, 8, p, 4, 3, 1.0, 2, S) == EINVAL           # no table
    assert lib.aae_bag_renorm(p, 12, 8, None, 4, 3, 1.0, 2, S) == EINVAL           # no index block
    assert lib.aae_bag_csr_renorm(p, 12, 8, p, p, 4, 9, None, 0, 4, 0, 1.0, 2, p, 1 << 20, S) == EINVAL    # max_entries < 1
    assert lib.aae_bag_csr_renorm(p, 12, 8, p, p, 4, 9, None, 0, 4, 9, 1.0, 2, p, 8, S) == EINVAL          # scratch too small
    assert lib.aae_bag_csr_renorm(p, 12, 8, p, p, 4, 9, None, 2, 4, 9, 1.0, 2, p, 1 << 20, S) == EINVAL    # rows outside
    upd = lambda opt, flags: lib.aae_bag_update_flags(p, p, p, p, 12, 8, p, 4, 3, 0, -1, p, 8, opt, 1e-3, 1, flags, S)     # noqa: E731
    csr = lambda opt, flags: lib.aae_bag_csr_update_flags(p, p, p, p, 12, 8, p, p, None, 4, 9, None, 0, 4, 9, 0, -1, p, 8, opt,  # noqa: E731
                                                          1e-3, 1, flags, p, 1 << 20, S)
    for call in (upd, csr):
        assert call(_hip.CAT_SPARSE_ADAM, _hip.BAG_SCALE_BY_FREQ) == EINVAL      # no sparse gradient scaled by frequency
        assert call(_hip.CAT_ADAM, 2) == EINVAL and call(_hip.CAT_ADAM, -1) == EINVAL      # unknown flags
    # the scratch of a step is what it was: the renorm needs no more
    assert _hip.bag_csr_scratch_bytes(16, 100) == (16 * 100 + 4 * (16 + 17 + 16 + 100 + 16 * 256) + 255) // 256 * 256
