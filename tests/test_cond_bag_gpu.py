"""aae_bag_encode / aae_bag_update (csrc/cond_bag.h) on the device, at three levels: the kernels against torch on the CPU,
the C ABI on the reference's recorded runs, and the Python models (CategoricalCondition(reduce="max") and
EmbeddingBagCondition on the fused route) on the same runs, against the bridged route and through a checkpoint.

Tolerances are the project's own, unchanged: optimiser moments at test_oracle_golden.py's VAE figures (exp_avg 2e-8 / 2e-4,
exp_avg_sq 1e-12 / 2e-4), tables 1e-5; the reference's runs at test_parity_abi_gpu.py's (loss rtol 2e-5, parameters, condition
table and predict 1e-5)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bag_cases as BC
from golden_util import Fixture
from vae_wide_cases import to_hip

pytestmark = pytest.mark.gpu

TOL_PARAM, TOL_RECON = 1e-5, 1e-5
VAE_NAMES = ("fc1", "fc21", "fc22", "fc3", "fc4")
AAE_FIXTURES = [n for n, (model, _) in BC.BAG_FIXTURES.items() if model == "aae"]


# ---- 1. the kernels against torch --------------------------------------------------------------------------------------------
def _device_step(c, lr, sparse, step=1):
    """bag_encode into a column slice of a wider block, bag_update from a column slice of a wider block: (out, table, m, v)."""
    from aaerec import _hip
    dev = torch.device("cuda")
    table = torch.from_numpy(c["table"]).to(dev)
    m, v, scratch = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    idx = torch.from_numpy(c["idx"].astype(np.int32)).to(dev)
    rows, dim = c["dout"].shape
    block = torch.full((rows, dim + 5), float("nan"), device=dev)
    dblock = torch.full((rows, dim + 3), float("nan"), device=dev)
    dblock[:, 2:2 + dim] = torch.from_numpy(c["dout"]).to(dev)
    _hip.bag_encode(table, idx, block[:, 3:3 + dim], reduce=c["reduce"], padding_idx=c["pad"])
    _hip.bag_update(table, m, v, idx, dblock[:, 2:2 + dim], lr, step, reduce=c["reduce"], padding_idx=c["pad"],
                    grad_scratch=scratch, sparse=sparse)
    block = block.cpu().numpy()
    assert np.isnan(block[:, :3]).all() and np.isnan(block[:, 3 + dim:]).all(), "bag_encode wrote outside its columns"
    assert not scratch.any(), "the gradient scratch is left zero"
    return block[:, 3:3 + dim], table.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def _want(c, lr, sparse):
    """torch on the CPU; the one combination torch does not have (EmbeddingBag max + SparseAdam): the restatement, which
    test_cond_bag_cpu.py holds to torch on every other combination."""
    if BC.torch_exists(c["reduce"], sparse):
        outs, p, m, v = BC.torch_steps(c["table"], [c["idx"]], c["reduce"], c["pad"], [c["dout"]], lr, sparse)
        return outs[0], p, m, v
    p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
    out = BC.bag_step(p, m, v, c["idx"], c["reduce"], c["pad"], c["dout"], lr, 1, sparse)
    return out, p, m, v


@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
@pytest.mark.parametrize("reduce", list(BC.NAMES), ids=list(BC.NAMES.values()))
def test_kernels_equal_torch(reduce, sparse):
    """Every shape of bag_cases.SHAPES, with and without a padding row: inputs on the 1/8 grid (exact sums), no two different
    table rows tying in a column of a bag (checked by the generator), repeats of one row kept.  Encodes of sum and of both max
    modes bit for bit, mean within 2 ulp (torch may multiply by a reciprocal); moments and table at the optimiser tolerances;
    each case twice with identical bits."""
    lr = 1e-2
    for pad in BC.PADS[reduce]:
        for si, (rows, width, dim, vocab) in enumerate(BC.SHAPES):
            c = BC.make_case(1000 * reduce + 10 * si + pad + 1, rows, width, dim, vocab, reduce, pad)
            if reduce >= BC.MAX_PAD0:
                assert BC.no_cross_ties(c["table"], c["idx"], reduce, pad)
            tag = f"{BC.NAMES[reduce]} pad {pad} rows {rows} width {width} dim {dim} vocab {vocab}"
            want_out, want_p, want_m, want_v = _want(c, lr, sparse)
            got = _device_step(c, lr, sparse)
            again = _device_step(c, lr, sparse)
            for a, b in zip(got, again):
                assert np.array_equal(a, b), tag + ": two runs differ"
            out, p, m, v = got
            if reduce in (BC.SUM, BC.MAX_PAD0, BC.MAX):
                assert np.array_equal(out, want_out), tag
            else:
                ulp = np.spacing(np.abs(want_out).astype(np.float32))
                assert (np.abs(out - want_out) <= 2 * ulp).all(), tag
            np.testing.assert_allclose(m, want_m, atol=2e-8, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(v, want_v, atol=1e-12, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(p, want_p, atol=1e-5, rtol=0, err_msg=tag)
            if pad >= 0:
                assert np.array_equal(p[pad], c["table"][pad]), tag + ": the padding row moved"


@pytest.mark.parametrize("reduce", list(BC.NAMES), ids=list(BC.NAMES.values()))
def test_indices_outside_the_table_are_skipped(reduce):
    """torch raises on them; the kernels handle them like padding slots (the restatement's rule): nothing is read or written
    outside the table."""
    c = BC.make_case(77 + reduce, 9, 4, 33, 12, reduce, -1)
    c["idx"][0, 1], c["idx"][3, :], c["idx"][5, 0] = -3, 12, 2 ** 30
    c["dout"] = BC.settle_mean_gradients(c["idx"], c["dout"], 12, -1, reduce)
    for sparse in (False, True):
        p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
        want = BC.bag_step(p, m, v, c["idx"], reduce, -1, c["dout"], 1e-2, 1, sparse)
        out, gp, gm, gv = _device_step(c, 1e-2, sparse)
        np.testing.assert_allclose(out, want, rtol=3e-7, atol=0)
        assert not out[3].any()
        np.testing.assert_allclose(gm, m, atol=2e-8, rtol=2e-4)
        np.testing.assert_allclose(gv, v, atol=1e-12, rtol=2e-4)
        np.testing.assert_allclose(gp, p, atol=1e-5, rtol=0)


# ---- 2. the reference's recorded runs through the C ABI ------------------------------------------------------------------------
def _csr(fx, m, s, prefix=None):
    from aaerec._hip import DeviceCSR
    ip, idx, val = fx.batch(s, prefix)
    return DeviceCSR.from_arrays(ip, idx, val, fx.cfg["N"], m.device)


def _vae_params(fx, prefix):
    return to_hip({f"{n}.{t}": fx.z[f"{prefix}.{n}.{t}"] for n in VAE_NAMES for t in ("weight", "bias")})


@pytest.mark.parametrize("name", list(BC.BAG_FIXTURES))
def test_abi_replays_the_reference(name):
    """HipAAE's fused step with [bag_encode(table)] as its condition block and bag_update from AAE_T_ACT_DZC's columns, on
    the reference's recorded steps of CategoricalCondition(reduce="max") (SparseAdam / Adam) and EmbeddingBagCondition (mean,
    max; sum behind the VAE)."""
    from aaerec import _hip
    fx = Fixture(name)
    c, vae = fx.cfg, bool(fx.cfg.get("vae"))
    reduce, pad, sparse, lr = BC.fixture_kind(fx)
    if vae:
        m = _hip.HipAAE(c["N"], c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=c["B"], rng_mode="inject", gen_lr=c["gen_lr"],
                        reg_lr=c["gen_lr"], dropout=(0.0, 0.0), vae=True)
        m.load_params(_vae_params(fx, "init"))
    else:
        m = _hip.HipAAE(c["N"], c["h"], c["c"], cond_inc=c["cond_inc"], max_batch=c["B"], rng_mode="inject", **fx.model_kwargs())
        m.load_params(fx.init_params())
    table = torch.as_tensor(fx.z["init.cond.embedding"], device=m.device).contiguous()
    t_m, t_v, scratch = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    dim = table.shape[1]

    def block(prefix):
        idx = torch.as_tensor(fx.z[prefix + ".cond0"].astype(np.int32), device=m.device).contiguous()
        b = torch.empty(idx.shape[0], dim, dtype=torch.float32, device=m.device)
        _hip.bag_encode(table, idx, b, reduce=reduce, padding_idx=pad)
        return b, idx
    for s in range(fx.steps):
        csr = _csr(fx, m, s)
        B = csr.shape[0]
        cond, idx = block(f"step{s}")
        if vae:
            m.vae_step(csr, 0, B, cond=cond, eps=fx.z[f"step{s}.eps"])
            l = m.losses()
            got_loss, want_loss = (l[0] + l[1]) / B, fx.z[f"step{s}.losses"][0]
            want = _vae_params(fx, f"step{s}")
        else:
            m.step(csr, 0, B, cond=cond, masks=fx.masks(s), z_real=fx.z[f"step{s}.z_real"])
            got_loss, want_loss = m.losses(), fx.z[f"step{s}.losses"]
            want = fx.expected_params(s)
        _hip.bag_update(table, t_m, t_v, idx, m.cond_grad(B)[:, :dim], lr, s + 1, reduce=reduce, padding_idx=pad,
                        grad_scratch=scratch, sparse=sparse)
        np.testing.assert_allclose(got_loss, want_loss, rtol=2e-5, err_msg=f"{name} step {s} loss")
        got = m.state_dict()
        worst = max(float(np.abs(got[k] - w).max()) for k, w in want.items())
        for k, w in want.items():
            np.testing.assert_allclose(got[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k}")
        tdiff = float(np.abs(table.cpu().numpy() - fx.z[f"step{s}.cond.embedding"]).max())
        print(f"{name} step {s}: parameters within {worst:.3g}, table within {tdiff:.3g}")
        np.testing.assert_allclose(table.cpu().numpy(), fx.z[f"step{s}.cond.embedding"], atol=1e-5, err_msg=f"{name} table {s}")
        np.testing.assert_allclose(t_m.cpu().numpy(), fx.z[f"step{s}.cond.m"], atol=2e-8, rtol=2e-4, err_msg=f"{name} m {s}")
        np.testing.assert_allclose(t_v.cpu().numpy(), fx.z[f"step{s}.cond.v"], atol=1e-12, rtol=2e-4, err_msg=f"{name} v {s}")
    pcsr = _csr(fx, m, 0, prefix="predict")
    pcond = block("predict")[0]
    if vae:
        out = m.vae_predict(pcsr, 0, pcsr.shape[0], cond=pcond, eps=fx.z["predict.eps"]).cpu().numpy()
    else:
        out = m.predict(pcsr, 0, pcsr.shape[0], cond=pcond).cpu().numpy()
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)


# ---- 3. the Python models ------------------------------------------------------------------------------------------------------
def _condition(fx, bridged):
    """(the fixture's condition with its table on the GPU, prefix -> condition_data).  bridged: a subclass whose device_native
    refuses, so that the model cuts the step at the condition boundary for torch autograd."""
    from aaerec import condition as C
    init = torch.from_numpy(fx.z["init.cond.embedding"])
    if "bag" in fx.cfg:
        b = fx.cfg["bag"]
        cls = C.EmbeddingBagCondition
        if bridged:
            cls = type("BridgedBag", (cls,), {"device_native": lambda self, device: False})
        cond = cls(b["num_embeddings"], b["dim"], **b["kwargs"])
        cond.embedding_bag.cuda()
        with torch.no_grad():
            cond.embedding_bag.weight.copy_(init)
        return cond, cond.embedding_bag.weight, (lambda prefix: [fx.z[prefix + ".cond0"]])
    k = fx.cfg["cat"]
    cls = C.CategoricalCondition
    if bridged:
        cls = type("BridgedCat", (cls,), {"device_native": lambda self, device: False})
    cond = cls(init.shape[1], sparse=k["sparse"], use_cuda=True, reduce=k["reduce"], lr=k["lr"])
    cond.vocab = {"a%d" % i: i for i in range(1, init.shape[0])}          # indices are given pre-transformed
    cond.embedding = torch.nn.Embedding(init.shape[0], init.shape[1], padding_idx=0, sparse=k["sparse"]).cuda()
    with torch.no_grad():
        cond.embedding.weight.copy_(init)
    cond.optimizer = (torch.optim.SparseAdam if k["sparse"] else torch.optim.Adam)(cond.embedding.parameters(), lr=k["lr"])
    # the fixture stores the batch-padded lists: strip the padding again (one row always spans the padded width)
    return cond, cond.embedding.weight, (lambda prefix: [[[int(j) for j in row if j != 0] or [0] for row in fx.z[prefix + ".cond0"]]])


def _model(fx, bridged=False):
    from aaerec import condition as C
    cfg = fx.cfg
    cond, weight, inputs = _condition(fx, bridged)
    conds = C.ConditionList([("authors", cond)])
    if cfg.get("vae"):
        from aaerec.vae import VAE
        m = VAE(cfg["N"], cfg["N"], n_hidden=cfg["h"], n_code=cfg["c"], lr=cfg["gen_lr"], batch_size=cfg["B"], conditions=conds,
                verbose=True, rng_mode="reference")
        m.hip.load_params(_vae_params(fx, "init"))
        assert m._cond_native == (not bridged)
    else:
        from aaerec.aae import AdversarialAutoEncoder
        m = AdversarialAutoEncoder(n_hidden=cfg["h"], n_code=cfg["c"], batch_size=cfg["B"], conditions=conds, verbose=True,
                                   rng_mode="reference", **fx.model_kwargs())
        m._build(cfg["N"], cfg["cond_inc"])
        m.hip.load_params(fx.init_params())
        assert m._is_device_native() == (not bridged) and not m._is_constant_concat()
    return m, cond, weight, inputs


def _X(fx, s, prefix=None):
    ip, idx, val = fx.batch(s, prefix)
    return sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, fx.cfg["N"]))


def _fit_step(fx, m, s, inputs):
    if fx.cfg.get("vae"):
        eps = fx.z[f"step{s}.eps"]
        m._eps = lambda B, eps=eps: torch.from_numpy(eps)
    else:
        masks, zr = fx.masks(s), fx.z[f"step{s}.z_real"]
        m._host_randomness = lambda B, masks=masks, zr=zr: (masks, torch.from_numpy(zr))
    m.partial_fit(_X(fx, s), condition_data=inputs(f"step{s}"))


def _params(fx, m):
    if fx.cfg.get("vae"):
        return {k: v.numpy() for k, v in m.state_dict().items() if k.split(".")[0] in VAE_NAMES}
    return m.hip.state_dict()


def _predict(fx, m, inputs):
    if fx.cfg.get("vae"):
        m._eps = lambda B: torch.from_numpy(fx.z["predict.eps"])
    else:
        m.batch_size = 7
    return m.predict(_X(fx, 0, "predict"), condition_data=inputs("predict"))


@pytest.mark.parametrize("name", list(BC.BAG_FIXTURES))
def test_models_train_the_condition_on_the_fused_route(name):
    """AdversarialAutoEncoder / VAE .partial_fit / .predict with the recorded draws: the condition is device-native, the
    table and the torch-layout optimiser state follow the reference, and a second model whose condition is forced onto the
    bridged route (torch autograd through encode_impose) agrees with it."""
    fx = Fixture(name)
    vae = bool(fx.cfg.get("vae"))
    m, cond, weight, inputs = _model(fx)
    mb, condb, weightb, inputsb = _model(fx, bridged=True)
    assert cond.device_native(m.hip.device) and not condb.device_native(mb.hip.device)
    for s in range(fx.steps):
        _fit_step(fx, m, s, inputs)
        _fit_step(fx, mb, s, inputsb)
        if vae:
            np.testing.assert_allclose(m.last_loss, fx.z[f"step{s}.losses"][0], rtol=2e-5)
            np.testing.assert_allclose(mb.last_loss, m.last_loss, rtol=2e-5)
            want = {f"{n}.{t}": fx.z[f"step{s}.{n}.{t}"] for n in VAE_NAMES for t in ("weight", "bias")}
        else:
            np.testing.assert_allclose(m.last_losses, fx.z[f"step{s}.losses"], rtol=2e-5, atol=1e-6)
            np.testing.assert_allclose(mb.last_losses, m.last_losses, rtol=2e-5, atol=1e-6)
            want = fx.expected_params(s)
        got, gotb = _params(fx, m), _params(fx, mb)
        for k, w in want.items():
            np.testing.assert_allclose(got[k], w, atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k}")
            np.testing.assert_allclose(gotb[k], got[k], atol=TOL_PARAM, rtol=0, err_msg=f"{name} step {s} {k} bridged")
        table, tableb = weight.detach().cpu().numpy(), weightb.detach().cpu().numpy()
        np.testing.assert_allclose(table, fx.z[f"step{s}.cond.embedding"], atol=1e-5, err_msg=f"{name} table {s}")
        np.testing.assert_allclose(tableb, table, atol=1e-5, err_msg=f"{name} table {s} bridged")
        st, stb = cond.optimizer.state[weight], condb.optimizer.state[weightb]
        assert float(st["step"]) == float(fx.z[f"step{s}.cond.t"]) == float(stb["step"])
        if not getattr(cond, "sparse", False):
            assert torch.is_tensor(st["step"])                            # torch's own layout for dense Adam
        np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), fx.z[f"step{s}.cond.m"], atol=2e-8, rtol=2e-4)
        np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), fx.z[f"step{s}.cond.v"], atol=1e-12, rtol=2e-4)
        np.testing.assert_allclose(stb["exp_avg"].cpu().numpy(), st["exp_avg"].cpu().numpy(), atol=2e-8, rtol=2e-4)
        np.testing.assert_allclose(stb["exp_avg_sq"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), atol=1e-12, rtol=2e-4)
    out, outb = _predict(fx, m, inputs), _predict(fx, mb, inputsb)
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=TOL_RECON)
    np.testing.assert_allclose(outb, out, atol=TOL_RECON)
    sd = cond.optimizer.state_dict()                                      # a later torch-side step sees the same tensors
    assert sd["state"][0]["exp_avg"].shape == tuple(weight.shape)


@pytest.mark.parametrize("name", ["step_cat_max", "step_bag_max"])
def test_rank_calls_behind_the_native_conditions(name):
    """predict_topk and predict_ranks with the condition in the fused call, against the host ranker over the model's own
    predict(), as test_predict_topk_with_trainable_and_generic_conditions does."""
    from aaerec.evaluation import argtopk, remove_non_missing
    fx = Fixture(name)
    m, cond, weight, inputs = _model(fx)
    for s in range(2):
        _fit_step(fx, m, s, inputs)
    assert m._is_device_native()
    Xp, pc = _X(fx, 0, "predict"), inputs("predict")
    m.batch_size = 7
    scores = np.asarray(m.predict(Xp, condition_data=pc), dtype=np.float32)
    full = remove_non_missing(scores, Xp, copy=True)
    rows, cols = argtopk(full, 10)
    ids, vals = m.predict_topk(Xp, k=10, condition_data=pc)
    np.testing.assert_allclose(vals, full[rows, cols], atol=2e-6)
    assert np.all((ids == cols) | np.isclose(full[rows, ids], full[rows, cols], atol=1e-7))
    # three held-out items per row, none of them a known item
    r = np.random.default_rng(3)
    known = Xp.toarray() > 0
    Y = sp.lil_matrix(Xp.shape)
    for b in range(Xp.shape[0]):
        Y[b, r.choice(np.nonzero(~known[b])[0], size=3, replace=False)] = 1
    Y = Y.tocsr()
    Y.sort_indices()
    got = m.predict_ranks(Xp, Y, condition_data=pc)
    assert np.array_equal(got.indptr, Y.indptr) and np.array_equal(got.indices, Y.indices)
    masked = np.where(known, -np.inf, scores)
    for b in range(Xp.shape[0]):
        for j, rank in zip(got.indices[got.indptr[b]:got.indptr[b + 1]], got.data[got.indptr[b]:got.indptr[b + 1]]):
            lo = 1 + int((masked[b] > masked[b, j] + 2e-6).sum())
            hi = int((masked[b] >= masked[b, j] - 2e-6).sum())
            assert lo <= rank <= hi, (name, b, j, rank, lo, hi)


def test_embedding_bag_condition_through_a_checkpoint(tmp_path):
    """Save after three steps (the model's parameters and Adam state, the table, the condition's optimizer.state_dict() - torch's
    own layout), restore into a fresh model and a fresh condition, take the fourth step: the unbroken run's numbers."""
    fx = Fixture("step_bag_mean")
    m, cond, weight, inputs = _model(fx)
    for s in range(3):
        _fit_step(fx, m, s, inputs)
    torch.save({"params": m.hip.state_dict(), "adam": {w: m.hip.adam_state(w) for w in ("enc", "dec", "gen", "disc")},
                "bag": cond.embedding_bag.state_dict(), "bag_optim": cond.optimizer.state_dict()}, tmp_path / "ck.pt")
    _fit_step(fx, m, 3, inputs)
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)
    m2, cond2, weight2, inputs2 = _model(fx)
    m2.hip.load_params(ck["params"])
    for w, st in ck["adam"].items():
        m2.hip.load_adam_state(w, st)
    cond2.embedding_bag.load_state_dict(ck["bag"])
    cond2.optimizer.load_state_dict(ck["bag_optim"])
    assert cond2.device_native(m2.hip.device)
    _fit_step(fx, m2, 3, inputs2)
    a, b = m.hip.state_dict(), m2.hip.state_dict()
    for k in a:
        np.testing.assert_allclose(b[k], a[k], atol=1e-7, rtol=0, err_msg=k)
    np.testing.assert_allclose(weight2.detach().cpu().numpy(), weight.detach().cpu().numpy(), atol=1e-7, rtol=0)
    st, st2 = cond.optimizer.state[weight], cond2.optimizer.state[weight2]
    assert float(st2["step"]) == float(st["step"]) == 4.0
    np.testing.assert_allclose(st2["exp_avg"].cpu().numpy(), st["exp_avg"].cpu().numpy(), atol=1e-9, rtol=1e-6)
    np.testing.assert_allclose(st2["exp_avg_sq"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), atol=1e-13, rtol=1e-6)
    np.testing.assert_allclose(weight.detach().cpu().numpy(), fx.z["step3.cond.embedding"], atol=1e-5)
