"""max_norm (aae_bag_renorm / aae_bag_csr_renorm) and scale_grad_by_freq (AAE_BAG_SCALE_BY_FREQ) on the device: the renorm on
the grid and against the float64 restatement and torch's device module, the frequency-scaled update of every reduction
against the restatement (bag_opt_cases.py) and torch's device kernel, the padded and the resident route bit for bit, and the
models - native against the bridged route, resident against padded, predict's renorm.

Tolerances: a renormalised element within bag_opt_cases.renorm_bound; moments and table at test_cond_bag_gpu.py's
(exp_avg 2e-8 / 2e-4, exp_avg_sq 1e-12 / 2e-4, table 1e-5); models at its TOL_PARAM / TOL_RECON 1e-5."""
import numpy as np
import pytest
import torch

import bag_cases as BC
import bag_opt_cases as OC
import ragged_cases as RC
import test_cond_bag_gpu as TG
import test_cond_ragged_gpu as RG
from golden_util import Fixture

pytestmark = pytest.mark.gpu
f32 = np.float32
LR = 1e-2
# rows x width x dim x vocab whose 4100 entries make two sort runs of the resident route: every table row's run straddles them
TWO_RUNS = (82, 50, 7, 40)


# ---- the device side ---------------------------------------------------------------------------------------------------------
def _guarded(table):
    """The table on the device between two NaN rows nothing may write."""
    buf = torch.full((table.shape[0] + 2, table.shape[1]), float("nan"), device="cuda")
    buf[1:-1] = torch.from_numpy(np.asarray(table, dtype=f32)).cuda()
    return buf, buf[1:-1]


def _source(idx, route, weights=None):
    """A [rows, width] array or value lists as the route's source: an int32 block, or a window over resident bags."""
    from aaerec import _hip
    if route == "padded":
        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    lists = [[int(j) for j in row] for row in idx]
    bags = _hip.DeviceBags(lists, torch.device("cuda"), weights=None if weights is None else RC.flat(lists, weights)[2])
    return bags.window(row0=0, rows=len(lists))


def _renorm(table, idx, max_norm, norm_type, route):
    from aaerec import _hip
    buf, t = _guarded(table)
    (_hip.bag_renorm if route == "padded" else _hip.bag_csr_renorm)(t, _source(idx, route), max_norm, norm_type)
    buf = buf.cpu().numpy()
    assert np.isnan(buf[0]).all() and np.isnan(buf[-1]).all(), "the renorm wrote outside the table"
    return buf[1:-1]


def _step(table, idx, dout, reduce, pad, route, max_norm=None, norm_type=2.0, by_freq=False, weights=None):
    """renorm + encode + dense-Adam update, step 1: (out, table, exp_avg, exp_avg_sq)."""
    from aaerec import _hip
    buf, t = _guarded(table)
    m, v, scratch = torch.zeros_like(t), torch.zeros_like(t), torch.zeros_like(t)
    src = _source(idx, route, weights)
    out = torch.empty(len(idx), table.shape[1], device="cuda")
    d = torch.from_numpy(np.asarray(dout, dtype=f32)).cuda()
    padded = route == "padded"
    if max_norm is not None:
        (_hip.bag_renorm if padded else _hip.bag_csr_renorm)(t, src, max_norm, norm_type)
    (_hip.bag_encode if padded else _hip.bag_csr_encode)(t, src, out, reduce=reduce, padding_idx=pad)
    (_hip.bag_update if padded else _hip.bag_csr_update)(t, m, v, src, d, LR, 1, reduce=reduce, padding_idx=pad, grad_scratch=scratch,
                                                          sparse=False, scale_by_freq=by_freq)
    assert not scratch.any(), "the gradient scratch is left zero"
    buf = buf.cpu().numpy()
    assert np.isnan(buf[0]).all() and np.isnan(buf[-1]).all(), "the step wrote outside the table"
    return out.cpu().numpy(), buf[1:-1], m.cpu().numpy(), v.cpu().numpy()


def _same(got, want, tag):
    for name, a, b in zip(("encode", "table", "exp_avg", "exp_avg_sq"), got, want):
        assert np.array_equal(a, b), f"{tag}: {name} differs"


def _close(got, want, tag):
    """table and moments at the file's tolerances: got / want = (table, exp_avg, exp_avg_sq)."""
    np.testing.assert_allclose(got[1], want[1], atol=2e-8, rtol=2e-4, err_msg=tag + " exp_avg")
    np.testing.assert_allclose(got[2], want[2], atol=1e-12, rtol=2e-4, err_msg=tag + " exp_avg_sq")
    np.testing.assert_allclose(got[0], want[0], atol=1e-5, rtol=0, err_msg=tag + " table")


# ---- 1. the renorm on the grid -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", OC.NORM_TYPES, ids=["l1", "l2", "inf"])
def test_renorm_on_the_grid(norm_type):
    """Every shape of bag_cases.SHAPES and the two-sort-run shape, tables on the 1/8 grid: rows above max_norm are scaled
    once however often they are named (a second scaling would be off by max_norm / norm), the row exactly at max_norm (norm
    types 1 and inf: exact norms) and the all-zero row keep their bits, the padding row named is renormalised, indices
    outside the table touch nothing, rows the input does not name keep their bits; the padded and the resident route give
    the same bits, and so do two runs."""
    worst = 0.0
    for si, (rows, width, dim, vocab) in enumerate(BC.SHAPES + [TWO_RUNS]):
        pad = min(7, vocab - 1)                                 # make_idx names it in a whole bag (rows >= 3)
        table, idx, max_norm, at = OC.renorm_case(50 + si, rows, width, dim, vocab, pad, norm_type)
        tag = f"p {norm_type} rows {rows} width {width} dim {dim} vocab {vocab}"
        want, want64 = table.copy(), table.astype(np.float64)
        scaled = OC.renorm(want, idx, max_norm, norm_type)
        OC.renorm(want64, idx, max_norm, norm_type, np.float64)
        got = _renorm(table, idx, max_norm, norm_type, "padded")
        assert np.array_equal(_renorm(table, idx, max_norm, norm_type, "padded"), got), tag + ": two runs differ"
        assert np.array_equal(_renorm(table, idx, max_norm, norm_type, "csr"), got), tag + ": the resident route differs"
        bound = OC.renorm_bound(table, dim, max_norm)
        worst = max(worst, float((np.abs(got - want64) / np.maximum(bound, 1e-30)).max()))
        assert (np.abs(got - want64) <= bound).all() and (np.abs(got - want.astype(np.float64)) <= bound).all(), tag
        named = OC.named_rows(idx, vocab)
        unnamed = np.setdiff1d(np.arange(vocab), named)
        assert np.array_equal(got[unnamed], table[unnamed]), tag + ": a row nobody names moved"
        zero = [j for j in named if not table[j].any()]
        assert np.array_equal(got[zero], table[zero]), tag
        if at >= 0:
            assert at not in scaled and np.array_equal(got[at], table[at]), tag + ": the row at max_norm moved"
        if vocab == 40 and rows >= 5:
            n = OC.counts(idx, vocab)
            often = [j for j in scaled if n[j] >= 3 and OC.row_norm(table[j], norm_type, np.float64) > 1.05 * max_norm]
            assert often, tag + ": no row far above max_norm is named three times"
            assert zero and len(scaled) < len(named) and pad in scaled and (idx >= vocab).any() and (idx < 0).any(), tag
            assert not np.array_equal(got[pad], table[pad]), tag + ": the padding row is renormalised"
    print(f"p {norm_type}: worst |device - float64| / bound {worst:.3g}")


# ---- 2. the renorm against the float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", OC.NORM_TYPES, ids=["l1", "l2", "inf"])
def test_renorm_within_the_bound_of_float64(norm_type):
    """Tables off the grid (every sum rounds): the kernels and torch's device module (nn.Embedding and nn.EmbeddingBag on the
    same GPU, the bridged route's arithmetic) each within the bound of the float64 restatement, and within twice the bound
    of each other.  The bound is continuous across the threshold: a row whose decision flips has a scale of about 1.
    norm_type inf: torch's device kernel is no reference - it accumulates pow(|x|, p) and takes pow(., 1 / p), which for
    p = inf is 1 for every row with an element above 1 (measured on this GPU: 8e5 times the bound away from the float64
    restatement that CPU torch follows) - so there the kernels are held to float64 alone and torch's figure is printed.
    Known to fail now and then, on the assertion about TORCH: in 12 fresh processes on an MI355X the kernels' figures were the
    same to the last digit every time (p = 2, rows 65 width 5 dim 256: 0.00724 of the bound), while torch's device module gave
    other bits on identical inputs in two of them - once 0.272 instead of 0.125 against the kernels (p = 1, rows 65 width 2
    dim 7), once 1.62e3 times the bound away from float64 (p = 2, rows 65 width 5 dim 256: this assertion failed).  The
    assertions stand as the issue sets them; DESIGN 3.7b."""
    worst = [0.0, 0.0, 0.0]
    for si, (rows, width, dim, vocab) in enumerate(BC.SHAPES):
        table, idx, max_norm, _ = OC.renorm_case(90 + si, rows, width, dim, vocab, 0, norm_type, on_grid=False)
        idx = np.where((idx >= 0) & (idx < vocab), idx, 0)                  # (torch takes indices inside the table only)
        tag = f"p {norm_type} rows {rows} width {width} dim {dim} vocab {vocab}"
        want64 = table.astype(np.float64)
        OC.renorm(want64, idx, max_norm, norm_type, np.float64)
        bound = OC.renorm_bound(table, dim, max_norm)
        got = _renorm(table, idx, max_norm, norm_type, "padded")
        assert np.array_equal(_renorm(table, idx, max_norm, norm_type, "csr"), got), tag + ": the resident route differs"
        refs = [OC.torch_renorm(table, idx, max_norm, norm_type, bag, device="cuda") for bag in (False, True)]
        ratio = lambda a, b: float((np.abs(a - b) / np.maximum(bound, 1e-30)).max())      # noqa: E731
        figures = [ratio(got, want64), max(ratio(r, want64) for r in refs), max(ratio(got, r.astype(np.float64)) for r in refs)]
        worst = [max(a, b) for a, b in zip(worst, figures)]
        print(f"{tag}: native {figures[0]:.3g}, torch {figures[1]:.3g}, native against torch {figures[2]:.3g} (of the bound)")
        assert figures[0] <= 1, tag + ": the kernels against float64"
        if norm_type != OC.INF:
            assert figures[1] <= 1, tag + ": torch's device module against float64"
            assert figures[2] <= 2, tag + ": the kernels against torch's device module"
    print(f"p {norm_type}: worst figures {worst}")


# ---- 3. frequency scaling ----------------------------------------------------------------------------------------------------
def _freq_case(reduce, pad, si):
    rows, width, dim, vocab = (BC.SHAPES + [TWO_RUNS])[si]
    c = BC.make_case(2000 + 100 * reduce + 10 * si + pad + 1, rows, width, dim, vocab, reduce, pad)
    c["dout"] = OC.settle_gradients(c["table"], c["idx"], c["dout"], reduce, pad)
    return c, f"{BC.NAMES[reduce]} pad {pad} rows {rows} width {width} dim {dim} vocab {vocab}"


def _torch_device_bag_step(c, reduce, pad):
    """One step of nn.EmbeddingBag(scale_grad_by_freq=True) under torch.optim.Adam on the GPU: (table, exp_avg, exp_avg_sq)."""
    vocab, dim = c["table"].shape
    mod = torch.nn.EmbeddingBag(vocab, dim, mode={BC.SUM: "sum", BC.MEAN_COUNT: "mean"}[reduce],
                                padding_idx=None if pad < 0 else pad, scale_grad_by_freq=True).cuda()
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(c["table"]))
    opt = torch.optim.Adam(mod.parameters(), lr=LR)
    mod(torch.from_numpy(c["idx"].astype(np.int64)).cuda()).backward(torch.from_numpy(c["dout"]).cuda())
    opt.step()
    st = opt.state[mod.weight]
    return mod.weight.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


@pytest.mark.parametrize("reduce", list(BC.NAMES), ids=list(BC.NAMES.values()))
def test_frequency_scaled_update(reduce):
    """Every reduction under dense Adam (torch has no sparse gradient scaled by frequency), with and without a padding row,
    every shape of bag_cases.SHAPES and the two-sort-run shape: the restatement at the file's tolerances, the resident route
    bit for bit, and - nn.EmbeddingBag's sum and mean - torch's device kernel at the same tolerances.  (nn.EmbeddingBag's max
    mode refuses scale_grad_by_freq: the kernels' kBagMax is held to the restatement alone.)  dout is settled; table rows
    named once, twice, three times and 64 times or more all occur."""
    seen = set()
    for pad in BC.PADS[reduce]:
        for si in range(len(BC.SHAPES) + (pad == BC.PADS[reduce][0])):           # (the two-sort-run shape once a reduction)
            c, tag = _freq_case(reduce, pad, si)
            vocab = c["table"].shape[0]
            n = OC.counts(c["idx"], vocab)
            seen |= {int(x) for x in n[[j for j in range(vocab) if j != pad]]}
            p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
            want_out = OC.step(p, m, v, c["idx"], reduce, pad, c["dout"], LR, 1, by_freq=True)
            got = _step(c["table"], c["idx"], c["dout"], reduce, pad, "padded", by_freq=True)
            _same(_step(c["table"], c["idx"], c["dout"], reduce, pad, "csr", by_freq=True), got, tag + " (resident route)")
            if si == 0:
                _same(_step(c["table"], c["idx"], c["dout"], reduce, pad, "padded", by_freq=True), got, tag + " (second run)")
            np.testing.assert_allclose(got[0], want_out, rtol=3e-7, atol=0, err_msg=tag)
            _close(got[1:], (p, m, v), tag)
            if pad >= 0:
                assert np.array_equal(got[1][pad], c["table"][pad]) and not got[2][pad].any(), tag + ": the padding row moved"
            if reduce in (BC.SUM, BC.MEAN_COUNT):
                _close(got[1:], _torch_device_bag_step(c, reduce, pad), tag + " (torch's device kernel)")
    assert {1, 2, 3} <= seen and max(seen) >= 64, sorted(seen)


def test_frequency_scaling_with_per_sample_weights_on_the_resident_route():
    """Ragged lists with weights (sum mode): the count is every occurrence, whatever it weighs; against the restatement."""
    for pad in (-1, 0):
        for rows, dim, vocab in ((3, 7, 40), (65, 65, 40), (65, 256, 2)):
            rng = np.random.default_rng(rows + dim)
            c = RC.make_case(19 + rows + pad, rows, dim, vocab, BC.SUM, pad, outside=False)
            wts = RC.make_weights(rng, c["lists"])
            p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
            want_out = OC.step(p, m, v, c["lists"], BC.SUM, pad, c["dout"], LR, 1, by_freq=True, weights=wts)
            got = _step(c["table"], c["lists"], c["dout"], BC.SUM, pad, "csr", by_freq=True, weights=wts)
            tag = f"weights pad {pad} rows {rows} dim {dim} vocab {vocab}"
            assert np.array_equal(got[0], want_out), tag
            _close(got[1:], (p, m, v), tag)
            plain = _step(c["table"], c["lists"], c["dout"], BC.SUM, pad, "csr", by_freq=False, weights=wts)
            assert not np.array_equal(plain[2], got[2]), tag + ": the flag changed nothing"


def test_both_options_in_one_step_on_both_routes():
    """max_norm and scale_grad_by_freq together, off the grid, on the two-sort-run shape and a small one: the resident route's
    bits equal the padded route's, and the step lands on the restatement (the lookup and the update see the renormalised table)."""
    for rows, width, dim, vocab in (TWO_RUNS, (5, 5, 65, 40)):
        for reduce, pad in ((BC.SUM, -1), (BC.MEAN_COUNT, 1), (BC.MAX_PAD0, 0)):
            rng = np.random.default_rng(rows + reduce)
            table = rng.standard_normal((vocab, dim)).astype(f32)
            if pad >= 0:
                table[pad] = 0
            idx = BC.make_idx(rng, rows, width, vocab, pad)
            dout = rng.standard_normal((rows, dim)).astype(f32)
            tag = f"{BC.NAMES[reduce]} rows {rows}"
            got = _step(table, idx, dout, reduce, pad, "padded", max_norm=2.0, by_freq=True)
            _same(_step(table, idx, dout, reduce, pad, "csr", max_norm=2.0, by_freq=True), got, tag)
            p, m, v = table.copy(), np.zeros_like(table), np.zeros_like(table)
            want_out = OC.step(p, m, v, idx, reduce, pad, dout, LR, 1, max_norm=2.0, by_freq=True)
            # (a renormalised row may differ from the restatement's by a rounding of its scale - square root, division -
            # and a bag sums up to 50 of them: 50 x 2^-23 of values of order 1)
            np.testing.assert_allclose(got[0], want_out, rtol=1e-5, atol=1e-5, err_msg=tag)
            _close(got[1:], (p, m, v), tag)


# ---- 4. the models -----------------------------------------------------------------------------------------------------------
MAX_NORM = 3.0            # the recorded tables' rows have norms of 1.9 .. 3.6: some above, some below


def _table_condition(fx, kind, bridged):
    """(condition with its table on the GPU, its weight, prefix -> condition_data) over a recorded run's table and indices:
    CategoricalCondition(reduce='sum', sparse=False, max_norm) - kind 'cat_max_norm' - or CategoricalCondition(reduce='mean',
    sparse=False, max_norm, scale_grad_by_freq=True) - 'cat_both'.  bridged: test_cond_bag_gpu.py's subclass whose
    device_native refuses."""
    from aaerec import condition as C
    init = torch.from_numpy(fx.z["init.cond.embedding"]).clone()
    cls = C.CategoricalCondition
    if bridged:
        cls = type("Bridged", (cls,), {"device_native": lambda self, device: False})
    init[0] = 0                                                 # nn.Embedding reads its padding row
    opts = dict(max_norm=MAX_NORM) if kind == "cat_max_norm" else dict(max_norm=MAX_NORM, scale_grad_by_freq=True)
    cond = cls(init.shape[1], sparse=False, use_cuda=True, reduce="sum" if kind == "cat_max_norm" else "mean", lr=1e-3, **opts)
    cond.vocab = {"a%d" % i: i for i in range(1, init.shape[0])}
    cond.embedding = torch.nn.Embedding(init.shape[0], init.shape[1], padding_idx=0, sparse=False, **opts).cuda()
    with torch.no_grad():
        cond.embedding.weight.copy_(init)
    cond.optimizer = torch.optim.Adam(cond.embedding.parameters(), lr=1e-3)
    return cond, cond.embedding.weight, (lambda prefix: [[[int(j) for j in row if j != 0] or [0] for row in fx.z[prefix + ".cond0"]]])


def _model(fx, kind, bridged=False):
    from aaerec import condition as C
    cfg = fx.cfg
    cond, weight, inputs = _table_condition(fx, kind, bridged)
    conds = C.ConditionList([("authors", cond)])
    if cfg.get("vae"):
        from aaerec.vae import VAE
        m = VAE(cfg["N"], cfg["N"], n_hidden=cfg["h"], n_code=cfg["c"], lr=cfg["gen_lr"], batch_size=cfg["B"], conditions=conds,
                verbose=True, rng_mode="reference")
        m.hip.load_params(TG._vae_params(fx, "init"))
        assert m._cond_native == (not bridged), "the VAE does not take the condition natively"
    else:
        from aaerec.aae import AdversarialAutoEncoder
        m = AdversarialAutoEncoder(n_hidden=cfg["h"], n_code=cfg["c"], batch_size=cfg["B"], conditions=conds, verbose=True,
                                   rng_mode="reference", **fx.model_kwargs())
        m._build(cfg["N"], cfg["cond_inc"])
        m.hip.load_params(fx.init_params())
        assert m._is_device_native() == (not bridged), "the AAE does not take the condition natively"
    return m, cond, weight, inputs


@pytest.mark.parametrize("kind", ["cat_max_norm", "cat_both"])
@pytest.mark.parametrize("name", ["step_bag_mean", "step_vae_bag"], ids=["aae", "vae"])
def test_models_train_a_condition_with_the_options_on_the_fused_route(name, kind):
    """Three partial_fit steps with the recorded draws: the model takes the condition natively (without the feature this
    assertion fails), and agrees with a second model forced onto the bridged route - torch's device kernels behind autograd -
    in its parameters, the table and predict.  predict on a fresh copy renormalises the rows it names, once, and nothing else.
    The conditions: CategoricalCondition(reduce="sum", sparse=False, max_norm) and the same with reduce="mean" and
    scale_grad_by_freq=True as well.  (EmbeddingBagCondition still refuses both keywords - test_cond_bag_cpu.py pins that -
    so the issue's EmbeddingBagCondition(mode="mean", max_norm, scale_grad_by_freq=True) model is not built; nn.EmbeddingBag's
    forms are held to torch at the kernel level above.)"""
    from aaerec import _hip
    fx = Fixture(name)
    m, cond, weight, inputs = _model(fx, kind)
    mb, condb, weightb, inputsb = _model(fx, kind, bridged=True)
    assert cond.device_native(m.hip.device) and cond.has_table_options() and not condb.device_native(mb.hip.device)
    for s in range(3):
        TG._fit_step(fx, m, s, inputs)
        TG._fit_step(fx, mb, s, inputsb)
        got, gotb = TG._params(fx, m), TG._params(fx, mb)
        worst = max(float(np.abs(gotb[k] - got[k]).max()) for k in got)
        table, tableb = weight.detach().cpu().numpy(), weightb.detach().cpu().numpy()
        print(f"{name} {kind} step {s}: parameters within {worst:.3g}, table within {float(np.abs(tableb - table).max()):.3g}")
        for k in got:
            np.testing.assert_allclose(gotb[k], got[k], atol=TG.TOL_PARAM, rtol=0, err_msg=f"{name} {kind} step {s} {k}")
        np.testing.assert_allclose(tableb, table, atol=TG.TOL_PARAM, rtol=0, err_msg=f"{name} {kind} table {s}")
    norms = np.linalg.norm(weight.detach().cpu().numpy().astype(np.float64), axis=1)
    assert (norms > 0.99 * MAX_NORM).sum() >= 2 and (norms < 0.95 * MAX_NORM).sum() >= 2      # rows held at max_norm, rows below
    out, outb = TG._predict(fx, m, inputs), TG._predict(fx, mb, inputsb)
    np.testing.assert_allclose(outb, out, atol=TG.TOL_RECON)
    # predict on a fresh copy: one renorm of the rows the input names
    fresh, _, fweight, finputs = _model(fx, kind)
    before = fweight.detach().clone()
    fresh.batch_size = fx.cfg["B"]                              # one chunk: every named row meets the renorm once
    if fx.cfg.get("vae"):
        fresh._eps = lambda B: torch.from_numpy(fx.z["predict.eps"])
    fresh.predict(TG._X(fx, 0, "predict"), condition_data=finputs("predict"))
    idx = fx.z["predict.cond0"]
    once = before.clone()
    _hip.bag_renorm(once, torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda(), MAX_NORM, 2.0)
    assert torch.equal(fweight.detach(), once) and not torch.equal(once, before)
    want64 = before.cpu().numpy().astype(np.float64)
    OC.renorm(want64, idx, MAX_NORM, 2.0, np.float64)
    assert (np.abs(fweight.detach().cpu().numpy() - want64) <= OC.renorm_bound(before.cpu().numpy(), before.shape[1], MAX_NORM)).all()
    unnamed = np.setdiff1d(np.arange(before.shape[0]), OC.named_rows(idx, before.shape[0]))
    assert torch.equal(fweight.detach()[unnamed], before[unnamed])


@pytest.mark.parametrize("model", ["aae", "vae"])
def test_fit_with_resident_conditions_gives_the_padded_route_its_bits(model):
    """fit() of two epochs with resident_conditions=True against the padded route on the same data:
    CategoricalCondition(reduce='sum', sparse=False, max_norm) and CategoricalCondition(reduce='mean', sparse=False, max_norm,
    scale_grad_by_freq=True)."""
    from aaerec.condition import CategoricalCondition
    cat = lambda: CategoricalCondition(8, reduce="sum", sparse=False, max_norm=2.0)            # noqa: E731
    a, b = RG._fit(model, True, cat), RG._fit(model, False, cat)
    assert a[0]._is_device_native() and a[1].has_table_options() and float(RG._table_state(a[1])[1]) == 6.0
    RG._assert_same_fit(a, b, model + " cat")
    norms = np.linalg.norm(RG._table_state(a[1])[0].astype(np.float64), axis=1)
    assert norms.max() <= 2.0 * (1 + 1e-2) and (norms > 1.9).any()              # (Adam moves a renormalised row by lr a step)

    both = lambda: CategoricalCondition(8, reduce="mean", sparse=False, max_norm=2.0, scale_grad_by_freq=True)   # noqa: E731
    a, b = RG._fit(model, True, both), RG._fit(model, False, both)
    assert a[0]._is_device_native() and a[1].has_table_options()
    RG._assert_same_fit(a, b, model + " cat, both options")
