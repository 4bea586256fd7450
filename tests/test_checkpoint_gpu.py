"""The checkpoint surface of the C ABI - aae_store_linear / aae_load_linear / aae_store_adam / aae_load_adam
(include/aaerec_hip.h) - on handles that have RUN: a run that saves at step k and carries on must equal, bit for bit, a
second handle that loads that checkpoint and carries on (parameters, every Adam moment, step counts, losses per step),
and a handle rolled back to its own checkpoint must repeat itself.  A step depends on state the host derives from the
step count (the count of opened steps the step-opening gather and the early catch-up take their step number from, the
item list built ahead for a named batch, the optimiser table's entry written a step early, the interleaved weight
copies, the pending deferred dec_optim launch): these tests are what holds a restore to all of it.

Bit equality needs no tolerance (README: runs are reproducible to the bit).  Every comparison with the eager oracle
(oracle.aae_oracle) uses the numbers of test_parity_abi_gpu.test_deferred_adam_matches_eager_oracle_over_many_sparse_steps:
losses rtol 2e-4 / atol 1e-6, parameters atol 3e-5, exp_avg atol 1e-8 / rtol 1e-3, exp_avg_sq atol 1e-12 / rtol 1e-3.
The bf16 handle is the exception the bf16 suite already documents (a gradient within bf16 noise of zero flips the
direction of Adam's first steps): it takes test_bf16_gpu.test_bf16_step_matches_the_rounded_oracle's criteria as they
are, against the oracle with bf16-rounded operands."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = ("enc", "dec", "disc")
OPTS = ("enc", "dec", "gen", "disc")
LOSS_TOL = dict(rtol=2e-4, atol=1e-6)
PARAM_ATOL = 3e-5
M_TOL = dict(atol=1e-8, rtol=1e-3)
V_TOL = dict(atol=1e-12, rtol=1e-3)
LRS = dict(gen_lr=2e-3, reg_lr=1e-3)
EINVAL = -1


# ---- batches ------------------------------------------------------------------------------------------------------------
class Batch:
    def __init__(self, ip, idx, val, zr, masks, eps, cond, N):
        self.ip, self.idx, self.val, self.zr, self.masks, self.eps, self.cond, self.N = ip, idx, val, zr, masks, eps, cond, N
        self._csr = None

    @property
    def csr(self):
        if self._csr is None:
            from aaerec._hip import DeviceCSR
            self._csr = DeviceCSR.from_arrays(self.ip, self.idx, self.val, self.N, torch.device("cuda:0"))
        return self._csr


@functools.lru_cache(maxsize=None)
def batches_of(N, h, c, B, steps, seed, inc=0, planted=()):
    """The skewed-popularity batches of the deferred-Adam test (items 0..19 in most batches, the tail rarely - some
    never again), with the recorded randomness of inject mode.  planted: ((item, (steps it is seen at)), ...) - such an
    item is drawn nowhere else."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, N + 1) ** 1.3
    for item, _ in planted:
        p[item] = 0.0
    p /= p.sum()
    out = []
    for s in range(steps):
        rows = [np.sort(rng.choice(N, size=int(rng.integers(1, min(N, 6))), replace=False, p=p)) for _ in range(B)]
        for item, at in planted:
            if s in at:
                rows[0] = np.union1d(rows[0], [item])
        ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        val = np.ones(len(idx), dtype=np.float32)
        zr = rng.standard_normal((B, c)).astype(np.float32)
        masks = tuple((rng.random((B, h)) > 0.2).astype(np.uint8) for _ in range(12))
        eps = rng.standard_normal((B, c)).astype(np.float32)
        cond = rng.standard_normal((B, inc)).astype(np.float32) if inc else None
        out.append(Batch(ip, idx, val, zr, masks, eps, cond, N))
    return tuple(out)


# ---- models of every kind -----------------------------------------------------------------------------------------------
KINDS = {"aae": {}, "ae_only": dict(ae_only=True), "vae": dict(vae=True), "sgd": dict(optimizer="sgd"),
         "bf16": dict(dtype="bf16"), "cond": {}}


def cond_inc(kind):
    return 3 if kind == "cond" else 0


@functools.lru_cache(maxsize=None)
def init_of(N, h, c, kind):
    from oracle.dense_torch_port import init_params
    p = init_params(N, h, c, cond_inc=cond_inc(kind), seed=3)
    if kind == "vae":       # enc.lin3 = [fc21; fc22]
        q = init_params(N, h, c, seed=4)
        p["enc.lin3.weight"] = np.vstack([p["enc.lin3.weight"], q["enc.lin3.weight"]])
        p["enc.lin3.bias"] = np.concatenate([p["enc.lin3.bias"], q["enc.lin3.bias"]])
    return p


def model_kwargs(kind):
    kw = dict(LRS, dropout=(0.2, 0.2))
    if kind == "vae":
        kw = dict(gen_lr=LRS["gen_lr"], reg_lr=LRS["gen_lr"], dropout=(0.0, 0.0))
    return kw


def make(N, h, c, B, kind="aae", rng_mode="inject", load=True):
    from aaerec._hip import HipAAE
    dev = HipAAE(N, h, c, cond_inc=cond_inc(kind), max_batch=B, rng_mode=rng_mode, seed=1234, **model_kwargs(kind), **KINDS[kind])
    if load:
        dev.load_params(init_of(N, h, c, kind))
    return dev


def step(dev, kind, b, inject=True):
    B = len(b.ip) - 1
    if kind == "vae":
        dev.vae_step(b.csr, 0, B, eps=b.eps if inject else None)
    elif kind == "ae_only":
        dev.step(b.csr, 0, B, masks=list(b.masks[:4]) + [None] * 8 if inject else None)
    else:
        cond = torch.as_tensor(b.cond, device=dev.device) if b.cond is not None else None
        dev.step(b.csr, 0, B, cond=cond, masks=list(b.masks) if inject else None, z_real=b.zr if inject else None)
    return dev.losses()


# ---- the four entry points, whole checkpoints ------------------------------------------------------------------------------
def abi_store(dev):
    from aaerec import _hip
    ck = {"params": {}, "adam": {}}
    for n, net in enumerate(NETS):
        for layer in (1, 2, 3):
            ck["params"][f"{net}.lin{layer}.weight"], ck["params"][f"{net}.lin{layer}.bias"] = dev.store_linear(n, layer)
    for which in OPTS:
        st, steps = {}, set()
        for layer in (1, 2, 3):
            mw, vw, mb, vb, t = dev.store_adam(_hip._OPTIM_ID[which], layer)
            st[f"lin{layer}.weight"], st[f"lin{layer}.bias"] = (mw, vw), (mb, vb)
            steps.add(t)
        assert len(steps) == 1, (which, steps)
        st["step"] = steps.pop()
        ck["adam"][which] = st
    return ck


def abi_load(dev, ck):
    from aaerec import _hip
    for n, net in enumerate(NETS):
        for layer in (1, 2, 3):
            dev.load_linear(n, layer, ck["params"][f"{net}.lin{layer}.weight"], ck["params"][f"{net}.lin{layer}.bias"])
    for which in OPTS:
        st = ck["adam"][which]
        for layer in (1, 2, 3):
            (mw, vw), (mb, vb) = st[f"lin{layer}.weight"], st[f"lin{layer}.bias"]
            dev.load_adam(_hip._OPTIM_ID[which], layer, mw, vw, mb, vb, step=st["step"])


def assert_same_checkpoint(a, b, what):
    for k in a["params"]:
        np.testing.assert_array_equal(a["params"][k], b["params"][k], err_msg=f"{what}: {k}")
    for which in OPTS:
        assert a["adam"][which]["step"] == b["adam"][which]["step"], (what, which)
        for k, mv in a["adam"][which].items():
            if k != "step":
                np.testing.assert_array_equal(mv[0], b["adam"][which][k][0], err_msg=f"{what}: {which} exp_avg {k}")
                np.testing.assert_array_equal(mv[1], b["adam"][which][k][1], err_msg=f"{what}: {which} exp_avg_sq {k}")


def assert_store_equals_python_views(dev, ck):
    sd = dev.state_dict()
    assert set(sd) == set(ck["params"])
    for k, v in sd.items():
        assert ck["params"][k].shape == v.shape, (k, ck["params"][k].shape, v.shape)
        np.testing.assert_array_equal(ck["params"][k], v, err_msg=f"aae_store_linear vs state_dict: {k}")
    for which in OPTS:
        st = dev.adam_state(which)
        assert st["step"] == ck["adam"][which]["step"], which
        for k, mv in st.items():
            if k != "step":
                np.testing.assert_array_equal(ck["adam"][which][k][0], mv[0], err_msg=f"aae_store_adam vs adam_state: {which} m {k}")
                np.testing.assert_array_equal(ck["adam"][which][k][1], mv[1], err_msg=f"aae_store_adam vs adam_state: {which} v {k}")


# ---- the eager oracle -------------------------------------------------------------------------------------------------------
def _oracle_snapshot(ora, kind, steps):
    """The oracle's state in a checkpoint's shape (what it has no tensor for is absent)."""
    cp = lambda a: np.array(a, copy=True)                                            # noqa: E731
    if kind == "vae":
        P, o = ora.p, ora.opt
        cat = lambda a, b: np.concatenate([a, b])                                    # noqa: E731
        params = {"enc.lin1.weight": cp(P["fc1.weight"]), "enc.lin1.bias": cp(P["fc1.bias"]),
                  "enc.lin3.weight": cat(P["fc21.weight"], P["fc22.weight"]), "enc.lin3.bias": cat(P["fc21.bias"], P["fc22.bias"]),
                  "dec.lin1.weight": cp(P["fc3.weight"]), "dec.lin1.bias": cp(P["fc3.bias"]),
                  "dec.lin3.weight": cp(P["fc4.weight"]), "dec.lin3.bias": cp(P["fc4.bias"])}
        mv = lambda n: (cp(o.m[n]), cp(o.v[n]))                                      # noqa: E731
        mv2 = lambda a, b: (cat(o.m[a], o.m[b]), cat(o.v[a], o.v[b]))                # noqa: E731
        adam = {"enc": {"lin1.weight": mv("fc1.weight"), "lin1.bias": mv("fc1.bias"),
                        "lin3.weight": mv2("fc21.weight", "fc22.weight"), "lin3.bias": mv2("fc21.bias", "fc22.bias"), "step": steps},
                "dec": {"lin1.weight": mv("fc3.weight"), "lin1.bias": mv("fc3.bias"),
                        "lin3.weight": mv("fc4.weight"), "lin3.bias": mv("fc4.bias"), "step": steps}}
        return {"params": params, "adam": adam}
    params = {k: cp(v) for k, v in ora.p.items() if kind != "ae_only" or not k.startswith("disc.")}
    adam = {}
    for which, opt, net in (("enc", ora.opt_enc, "enc"), ("dec", ora.opt_dec, "dec"), ("gen", ora.opt_gen, "enc"), ("disc", ora.opt_disc, "disc")):
        if kind == "ae_only" and which in ("gen", "disc"):
            continue
        adam[which] = {k[len(net) + 1:]: (cp(opt.m[k]), cp(opt.v[k])) for k in opt.m}
        adam[which]["step"] = steps
    return {"params": params, "adam": adam}


@functools.lru_cache(maxsize=None)
def oracle_run(N, h, c, B, kind, seed, planted, marks):
    """The eager oracle over max(marks) of batches_of(...)'s steps: ({steps: snapshot} for steps in marks, losses per
    step).  Computed once per case and shared; nothing mutates it."""
    from oracle import aae_oracle as O
    bs = batches_of(N, h, c, B, max(marks), seed, cond_inc(kind), planted)
    init = init_of(N, h, c, kind)
    if kind == "vae":
        cc = c
        ora = O.OracleVAE({"fc1.weight": init["enc.lin1.weight"], "fc1.bias": init["enc.lin1.bias"],
                           "fc21.weight": init["enc.lin3.weight"][:cc], "fc21.bias": init["enc.lin3.bias"][:cc],
                           "fc22.weight": init["enc.lin3.weight"][cc:], "fc22.bias": init["enc.lin3.bias"][cc:],
                           "fc3.weight": init["dec.lin1.weight"], "fc3.bias": init["dec.lin1.bias"],
                           "fc4.weight": init["dec.lin3.weight"], "fc4.bias": init["dec.lin3.bias"]}, lr=LRS["gen_lr"])
    else:
        conds = [O.ConcatConst(cond_inc(kind))] if cond_inc(kind) else []
        ora = O.OracleAAE(init, conditions=conds, bf16=kind == "bf16", optimizer="sgd" if kind == "sgd" else "adam", **model_kwargs(kind))
    snaps, losses = {}, []
    for s, b in enumerate(bs):
        if kind == "vae":
            losses.append((ora.partial_fit(b.ip, b.idx, b.val, b.eps),))
        elif kind == "ae_only":
            losses.append((ora.ae_step(b.ip, b.idx, b.val, list(b.masks[:4])),))
        else:
            losses.append(tuple(ora.partial_fit(b.ip, b.idx, b.val, b.zr, list(b.masks), [b.cond] if b.cond is not None else None)))
        if s + 1 in marks:
            snaps[s + 1] = _oracle_snapshot(ora, kind, s + 1)
    return snaps, tuple(losses)


def oracle_loss_view(kind, dev_losses, B):
    """The device's loss triple as the number(s) the oracle of this kind returns."""
    if kind == "vae":
        return ((dev_losses[0] + dev_losses[1]) / B,)
    return dev_losses[:1] if kind == "ae_only" else dev_losses


def assert_close_to_oracle(ck, snap, kind, what, steps):
    if kind == "bf16":
        # test_bf16_gpu.test_bf16_step_matches_the_rounded_oracle's criteria, as they are
        lr = max(LRS.values())
        for k, w in snap["params"].items():
            d = np.abs(ck["params"][k].astype(np.float64) - w)
            frac, mx, bound = float((d > 1e-4 * max(1.0, lr / 1e-3)).mean()), float(d.max()), 3.0 * lr * steps * (2 if k.startswith("enc.") else 1)
            print(f"{what} bf16 {k}: fraction beyond {frac:.5f}, max {mx:.3g}, bound {bound:.3g}")
            assert frac <= 1e-2 and mx <= bound, (what, k, frac, mx, bound)
        for which, st in snap["adam"].items():
            assert ck["adam"][which]["step"] == st["step"], (what, which)
        return
    fails = []

    def near(name, got, want, atol, rtol):
        err = np.abs(got.astype(np.float64) - want) - rtol * np.abs(want)
        print(f"{what} {name}: max |difference| {np.abs(got.astype(np.float64) - want).max():.3g} (atol {atol:g}, rtol {rtol:g})")
        if got.shape != want.shape or err.max() > atol:
            fails.append((name, float(err.max())))
    for k, w in snap["params"].items():
        near(k, ck["params"][k], w, PARAM_ATOL, 0.0)
    for which, st in snap["adam"].items():
        assert ck["adam"][which]["step"] == st["step"], (what, which, ck["adam"][which]["step"], st["step"])
        for k, mv in st.items():
            if k != "step":
                near(f"{which} exp_avg {k}", ck["adam"][which][k][0], mv[0], **M_TOL)
                near(f"{which} exp_avg_sq {k}", ck["adam"][which][k][1], mv[1], **V_TOL)
    assert not fails, (what, fails)


# ---- (a) what store writes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,h,c,B", [(33, 8, 4, 2), (31, 12, 3, 17), (900, 12, 6, 6), (3001, 100, 50, 37)])
def test_store_writes_the_reference_layout_after_sparse_steps(N, h, c, B):
    """12 steps on batches whose tail items never recur (deferred first-layer updates pending when the store is called):
    aae_store_linear of every (net, layer) == HipAAE.state_dict() and aae_store_adam of every (optimiser, layer) ==
    adam_state(), bit for bit and step counts included, and both == the eager oracle.  (33, 8, 4, 2): h + 1 == ldh
    while c + 1 != ldz; (3001, 100, 50, 37): a vocabulary that is no multiple of the 32-item tile, enc.lin1 transposed
    across a padded row.  Then the partial calls: weight only, bias only, step only, and moments loaded with step = -1,
    which leaves the count alone."""
    from aaerec import _hip
    steps = 12
    dev = make(N, h, c, B)
    bs = batches_of(N, h, c, B, steps, 11)
    snaps, want = oracle_run(N, h, c, B, "aae", 11, (), (steps,))
    for s, b in enumerate(bs):
        got = step(dev, "aae", b)
        np.testing.assert_allclose(got, want[s], err_msg=f"step {s}", **LOSS_TOL)
    ck = abi_store(dev)
    assert ck["params"]["enc.lin1.weight"].shape == (h, N) and ck["params"]["dec.lin3.weight"].shape == (N, h)
    assert ck["params"]["enc.lin3.weight"].shape == (c, h) and ck["params"]["disc.lin3.weight"].shape == (1, h)
    assert_store_equals_python_views(dev, ck)
    assert all(ck["adam"][w]["step"] == steps for w in OPTS)
    assert_close_to_oracle(ck, snaps[steps], "aae", f"({N},{h},{c},{B})", steps)
    # partial stores
    for n, net in enumerate(NETS):
        for layer in (1, 2, 3):
            w, none = dev.store_linear(n, layer, bias=False)
            assert none is None
            np.testing.assert_array_equal(w, ck["params"][f"{net}.lin{layer}.weight"])
            none, b = dev.store_linear(n, layer, weight=False)
            assert none is None
            np.testing.assert_array_equal(b, ck["params"][f"{net}.lin{layer}.bias"])
    for which in OPTS:
        assert dev.store_adam(_hip._OPTIM_ID[which], 1, weight=False, bias=False)[4] == steps
        mw, vw, _, _, t = dev.store_adam(_hip._OPTIM_ID[which], 3, bias=False)
        np.testing.assert_array_equal(mw, ck["adam"][which]["lin3.weight"][0])
        np.testing.assert_array_equal(vw, ck["adam"][which]["lin3.weight"][1])
    # partial loads: enc.lin1 (item-major on the device, its bias a tensor of its own) and a hidden layer
    rng = np.random.default_rng(0)
    for n, layer in ((0, 1), (1, 1), (2, 3)):
        key = f"{NETS[n]}.lin{layer}"
        w2 = rng.standard_normal(ck["params"][key + ".weight"].shape).astype(np.float32)
        b2 = rng.standard_normal(ck["params"][key + ".bias"].shape).astype(np.float32)
        dev.load_linear(n, layer, weight=w2)
        w, b = dev.store_linear(n, layer)
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, ck["params"][key + ".bias"])
        dev.load_linear(n, layer, bias=b2)
        w, b = dev.store_linear(n, layer)
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    # moments with step = -1 leave the count alone; a step alone leaves the moments alone
    for which in OPTS:
        oid = _hip._OPTIM_ID[which]
        old = dev.store_adam(oid, 1)
        new = [rng.random(a.shape).astype(np.float32) for a in old[:4]]
        dev.load_adam(oid, 1, *new, step=-1)
        got = dev.store_adam(oid, 1)
        for a, b in zip(got[:4], new):
            np.testing.assert_array_equal(a, b)
        assert got[4] == old[4]
        dev.load_adam(oid, 1, step=old[4] + 5)
        got = dev.store_adam(oid, 1)
        for a, b in zip(got[:4], new):
            np.testing.assert_array_equal(a, b)
        assert got[4] == old[4] + 5


# ---- (b) restore into a new handle --------------------------------------------------------------------------------------
K, J = 20, 150
PLANTED = ((880, (1, K + J - 1)), (881, (K - 1, K + 1)))


def resume_case(N, h, c, B, kind, k, j, seed, planted, rng_mode, prefetch, with_oracle):
    """Run A: k steps, stored through the ABI, j more.  Handle B: the same configuration and seed, loaded through
    aae_load_linear / aae_load_adam (all four optimisers with their counts), the same j batches.  Losses after every one
    of the j steps, then every parameter, every moment pair and every count: equal bits.  B against the oracle's k + j
    eager steps as well - A and B could be wrong the same way."""
    inject = rng_mode == "inject"
    bs = batches_of(N, h, c, B, k + j, seed, cond_inc(kind), planted)

    def run(dev, lo, hi):
        out = []
        for s in range(lo, hi):
            if prefetch and s + 1 < k + j:
                dev.prefetch(bs[s + 1].csr, 0, B)      # every batch named one step ahead, across the checkpoint as well
            out.append(step(dev, kind, bs[s], inject))
        return out
    a = make(N, h, c, B, kind, rng_mode)
    la = run(a, 0, k)
    ck = abi_store(a)
    assert_store_equals_python_views(a, ck)
    if with_oracle:
        snaps, want = oracle_run(N, h, c, B, kind, seed, planted, (k, k + j))
        assert_close_to_oracle(ck, snaps[k], kind, f"{kind} A at step {k}", k)
    la = run(a, k, k + j)
    end_a = abi_store(a)
    b = make(N, h, c, B, kind, rng_mode, load=False)
    abi_load(b, ck)
    assert_same_checkpoint(abi_store(b), ck, "what was loaded comes back")
    lb = run(b, k, k + j)
    for s, (x, y) in enumerate(zip(la, lb)):
        assert x == y, f"losses of step {k + s} (the {s + 1}. after the checkpoint): unbroken run {x}, resumed run {y}"
    end_b = abi_store(b)
    assert_same_checkpoint(end_a, end_b, "unbroken run vs resumed run")
    assert all(end_b["adam"][w]["step"] == k + j for w in OPTS)
    if with_oracle:
        for s in list(range(0, j, 20)) + [j - 1]:
            np.testing.assert_allclose(oracle_loss_view(kind, lb[s], B), want[k + s], err_msg=f"step {k + s}", **LOSS_TOL)
        assert_close_to_oracle(end_b, snaps[k + j], kind, f"{kind} B at step {k + j}", k + j)
    return ck, end_b


@pytest.mark.parametrize("prefetch", [False, "early"])
@pytest.mark.parametrize("rng_mode", ["inject", "device"])
def test_resumed_run_equals_the_unbroken_one(rng_mode, prefetch, monkeypatch):
    """(900, 12, 6, 6), k = 20, j = 150, the deferred-Adam test's batches with two planted items: 880 is seen at step 1
    and again at step k + j - 1 only - its gap crosses the checkpoint and exceeds kLazyReplay = 128 after it, so its
    catch-up ends in the closed-form tail -, 881 at steps k - 1 and k + 1.  Both runs flush the deferred first-layer
    updates at step k - A by storing, B by loading (which sets every row's sync step to k) -, so every later catch-up
    starts from the same step in both and they agree even where the closed-form tail is used.
    inject: masks and z_real are given, and B is held to the oracle.  device: dropout (.2, .2) from the counter generator,
    keyed by the step count - a restored count that did not reach the host's own would draw step 1's masks for step
    k + 1; the device draws are pinned to nothing, so bit equality of A and B is the assertion.
    prefetch = 'early': every batch is named a step ahead (AAE_EARLY_ANY: the early form at this batch size), so the
    step-opening gather and the early catch-up take their step number from the host's count."""
    if prefetch == "early":
        monkeypatch.setenv("AAE_EARLY_ANY", "1")
    resume_case(900, 12, 6, 6, "aae", K, J, 5, PLANTED, rng_mode, bool(prefetch), with_oracle=rng_mode == "inject")


# ---- (c) restore into a handle that has already run -----------------------------------------------------------------------
def rollback_case(N, h, c, B, k, j, seed, prefetch):
    """k steps, store, then three passes over the same j steps with a load of the stored state between them.  The first
    load meets everything a running handle can have pending (no call has joined or flushed since the last step: the
    deferred dec_optim launch, the catch-up of a batch named ahead, the list built for it), the second follows a store.
    With prefetch the last step of a pass names the batch that comes first after the load - the list built ahead then
    matches it - and a batch is named immediately before the store and before each load."""
    bs = batches_of(N, h, c, B, k + j, seed)
    dev = make(N, h, c, B, "aae", "device")

    def run(lo, hi, then):
        out = []
        for s in range(lo, hi):
            if prefetch:
                dev.prefetch(bs[s + 1 if s + 1 < hi else then].csr, 0, B)
            out.append(step(dev, "aae", bs[s], inject=False))
        return out
    run(0, k, k)
    if prefetch:
        dev.prefetch(bs[k + 1].csr, 0, B)
    ck = abi_store(dev)
    first = run(k, k + j, k)
    if prefetch:
        dev.prefetch(bs[k + 1].csr, 0, B)
    abi_load(dev, ck)
    second = run(k, k + j, k)
    if prefetch:
        dev.prefetch(bs[k + 1].csr, 0, B)
    end2 = abi_store(dev)
    abi_load(dev, ck)
    assert_same_checkpoint(abi_store(dev), ck, "rolled back")
    third = run(k, k + j, k)
    end3 = abi_store(dev)
    for name, again in (("second", second), ("third", third)):
        for s, (x, y) in enumerate(zip(first, again)):
            assert x == y, f"losses of step {k + s} ({s + 1}. after the checkpoint): first pass {x}, {name} pass {y}"
    assert_same_checkpoint(end2, end3, "second vs third pass")
    assert all(end3["adam"][w]["step"] == k + j for w in OPTS)


@pytest.mark.parametrize("path,env,prefetch", [
    ("default", {}, False),
    ("split_output_layer", {"AAE_SPLIT_ANY": "1"}, False),
    ("wide_batch_chain", {"AAE_X16_ROWS": "1"}, False),
    ("prefetch", {}, True),
    ("prefetch_split_output_layer", {"AAE_SPLIT_ANY": "1"}, True),
    ("early_prefetch", {"AAE_EARLY_ANY": "1"}, True)])
def test_rolled_back_handle_repeats_itself(path, env, prefetch, monkeypatch):
    """Device generator, dropout (.2, .2), on the execution paths the parity suite forces (its switches as they are): the
    single-launch output layer; its split form, whose deferred launch is pending when store and load are called; the
    wide-batch chain kernel, which reads the split bf16 weight copies a load must invalidate; a batch named ahead in both
    forms of the prefetch."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    rollback_case(900, 12, 6, 6, 20, 40, 5, prefetch)


def test_rolled_back_handle_repeats_itself_at_headline_width():
    """(5000, 200, 50, 100): the benchmark's layer widths and batch size - the output layer in its split form by the
    library's own choice, the late join, a batch named ahead."""
    rollback_case(5000, 200, 50, 100, 3, 4, 9, True)


# ---- (d) the other kinds of handle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ae_only", "vae", "sgd", "bf16", "cond"])
def test_other_handle_kinds_store_and_resume(kind):
    """(a) and (b) at (33, 8, 4, 2) with k = 5, j = 8 for the plain autoencoder, the VAE (enc.lin3 = [fc21; fc22]: 2c rows
    in the stored layout), SGD, bf16 arithmetic and a constant condition block (dec.lin1 takes n_code + cond_inc columns).
    SGD: the handle carries the moment tensors of an Adam handle and never reads or writes them - storing gives what was
    last loaded (zeros on a new handle), loading is a plain round trip, the step counts count (include/aaerec_hip.h)."""
    N, h, c, B, k, j = 33, 8, 4, 2, 5, 8
    ck, end = resume_case(N, h, c, B, kind, k, j, 21, (), "inject", False, with_oracle=True)
    want = {"enc.lin1.weight": (h, N), "enc.lin3.weight": (2 * c if kind == "vae" else c, h), "enc.lin3.bias": (2 * c if kind == "vae" else c,),
            "dec.lin1.weight": (h, c + cond_inc(kind)), "dec.lin3.weight": (N, h), "disc.lin1.weight": (h, c), "disc.lin3.bias": (1,)}
    for key, shape in want.items():
        assert ck["params"][key].shape == shape, (key, ck["params"][key].shape)
    assert ck["adam"]["enc"]["lin3.weight"][0].shape == want["enc.lin3.weight"]
    if kind != "sgd":
        return
    for c_ in (ck, end):
        for which in OPTS:
            for key, mv in c_["adam"][which].items():
                if key != "step":
                    assert not mv[0].any() and not mv[1].any(), (which, key)
    # moments loaded into an SGD handle: kept, returned, and without effect on the steps
    rng = np.random.default_rng(1)
    junk = {w: {key: (rng.random(mv[0].shape).astype(np.float32), rng.random(mv[1].shape).astype(np.float32)) if key != "step" else mv
                for key, mv in ck["adam"][w].items()} for w in OPTS}
    dev = make(N, h, c, B, kind, load=False)
    abi_load(dev, {"params": ck["params"], "adam": junk})
    for b in batches_of(N, h, c, B, k + j, 21)[k:]:
        step(dev, kind, b)
    got = abi_store(dev)
    for key in end["params"]:
        np.testing.assert_array_equal(got["params"][key], end["params"][key], err_msg=key)
    for w in OPTS:
        assert got["adam"][w]["step"] == k + j
        for key, mv in junk[w].items():
            if key != "step":
                np.testing.assert_array_equal(got["adam"][w][key][0], mv[0], err_msg=f"{w} {key}")
                np.testing.assert_array_equal(got["adam"][w][key][1], mv[1], err_msg=f"{w} {key}")


# ---- (e) rejections, and the count enc_optim and gen_optim share ------------------------------------------------------------
def test_bad_ids_are_rejected_and_leave_the_state_alone():
    N, h, c, B = 33, 8, 4, 2
    dev = make(N, h, c, B)
    for b in batches_of(N, h, c, B, 3, 31):
        step(dev, "aae", b)
    before = abi_store(dev)
    lib, hd = dev.lib, dev.handle
    buf = [np.full(N * (h + 1) + 64, 7.0, dtype=np.float32) for _ in range(4)]
    p = [a.ctypes.data_as(C.c_void_p) for a in buf]
    step_out = C.c_int64(-77)
    for net, layer in ((3, 1), (-1, 1), (0, 0), (0, 4), (2, -1)):
        assert lib.aae_load_linear(hd, net, layer, p[0], p[1]) == EINVAL, (net, layer)
        assert lib.aae_store_linear(hd, net, layer, p[0], p[1]) == EINVAL, (net, layer)
    for which, layer in ((4, 1), (-1, 1), (0, 0), (1, 4), (3, -2)):
        assert lib.aae_load_adam(hd, which, layer, p[0], p[1], p[2], p[3], 9) == EINVAL, (which, layer)
        assert lib.aae_store_adam(hd, which, layer, p[0], p[1], p[2], p[3], C.byref(step_out)) == EINVAL, (which, layer)
    assert lib.aae_load_adam(hd, 0, 1, None, None, None, None, 2 ** 31) == EINVAL       # a count the per-item sync steps cannot hold
    assert lib.aae_load_linear(None, 0, 1, p[0], p[1]) == EINVAL
    assert lib.aae_store_linear(None, 0, 1, p[0], p[1]) == EINVAL
    assert lib.aae_load_adam(None, 0, 1, p[0], p[1], p[2], p[3], 9) == EINVAL
    assert lib.aae_store_adam(None, 0, 1, p[0], p[1], p[2], p[3], C.byref(step_out)) == EINVAL
    assert step_out.value == -77 and all((a == 7.0).all() for a in buf)
    assert_same_checkpoint(abi_store(dev), before, "after the rejected calls")


def test_enc_optim_and_gen_optim_share_one_step_count():
    """advance_step_body files a step's -lr / bc1 of enc_optim under enc_optim's count and gen_optim's under gen_optim's,
    in the one ring the deferred catch-up reads by the step counter: the two counts cannot differ.  The contract
    (include/aaerec_hip.h): a count loaded for either is the count of both, of the step counter and of every item's sync
    step; dec_optim and disc_optim keep counts of their own.  A handle given enc_optim's count alone must therefore carry
    on exactly as one given both."""
    from aaerec import _hip
    N, h, c, B = 900, 12, 6, 6
    bs = batches_of(N, h, c, B, 12, 5)
    x, y = make(N, h, c, B), make(N, h, c, B)
    for b in bs[:3]:
        step(x, "aae", b)
        step(y, "aae", b)
    x.load_adam(_hip.O_ENC, 2, step=11)
    assert [x.store_adam(o, 1, weight=False, bias=False)[4] for o in (_hip.O_ENC, _hip.O_DEC, _hip.O_GEN, _hip.O_DISC)] == [11, 3, 11, 3]
    x.load_adam(_hip.O_GEN, 3, step=7)
    assert [x.store_adam(o, 1, weight=False, bias=False)[4] for o in (_hip.O_ENC, _hip.O_DEC, _hip.O_GEN, _hip.O_DISC)] == [7, 3, 7, 3]
    y.load_adam(_hip.O_ENC, 1, step=7)
    y.load_adam(_hip.O_GEN, 1, step=7)
    for b in bs[3:]:
        assert step(x, "aae", b) == step(y, "aae", b)
    ex, ey = abi_store(x), abi_store(y)
    assert_same_checkpoint(ex, ey, "count loaded for enc_optim alone vs for both")
    assert [ex["adam"][w]["step"] for w in OPTS] == [16, 12, 16, 12]
