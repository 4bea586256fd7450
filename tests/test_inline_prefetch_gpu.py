"""The batch named ahead (aae_prefetch_batch): its distinct-item list and deferred-Adam catch-up built by workgroups of the running
step's own layer-chain launches (the default where aae_step runs a batch of one fused launch) against the side stream's two
launches (AAE_NO_INLINE_PREFETCH=1, the route every other handle keeps).  Twin handles from the same seeds and draws run the
same calls and must agree in EVERY BYTE of every parameter, every Adam moment, tsync and the loss series: a row's replay is the
same fp32 operations in the same order on either route, rows are independent, and the order of the distinct-item list - arbitrary
on both routes - may show in nothing.

Which route ran is read from the library's launch counters (K_UNIQ_ITEMS / K_W1_CATCHUP count uniq_items_kernel /
w1_catchup_kernel as launches of their own; a list built inside a chain launch is no launch), never from a clock.

Handles are created with AAE_SPLIT_ANY=1 - the output layer as critical + deferred launch, the form bench.py's shape runs, and
the one whose reconstruction loss is reproducible from run to run at shapes this small (tests/test_w1_item_lists_gpu.py says why)."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

C = 4
WRAP = 65536          # kLazyTabCap: the ring of per-step optimiser scalars


def _corpus(N, rows, seed, per_row=6, lo=0):
    r = np.random.default_rng(seed)
    rr, cc = [], []
    for b in range(rows):
        items = r.choice(np.arange(lo, N), size=per_row, replace=False)
        rr += [b] * per_row
        cc += sorted(int(i) for i in items)
    return sp.csr_matrix((np.ones(len(rr), dtype=np.float32), (rr, cc)), shape=(rows, N))


def _handle(monkeypatch, side, N, h, B, max_nnz, c=C, params_seed=4, **kw):
    from aaerec._hip import HipAAE, K_UNIQ_ITEMS, K_W1_CATCHUP
    from oracle.dense_torch_port import init_params
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    if side:
        monkeypatch.setenv("AAE_NO_INLINE_PREFETCH", "1")
    else:
        monkeypatch.delenv("AAE_NO_INLINE_PREFETCH", raising=False)
    kw.setdefault("rng_mode", "device")
    kw.setdefault("dropout", (0.2, 0.2))
    m = HipAAE(N, h, c, max_batch=B, max_nnz=max_nnz, seed=11, **kw)
    if params_seed is not None:
        m.load_params(init_params(N, h, c, seed=params_seed))
    m.profile_enable(True, kernels=(K_UNIQ_ITEMS, K_W1_CATCHUP))
    return m


def _launches(m):
    from aaerec._hip import K_UNIQ_ITEMS, K_W1_CATCHUP
    return m.profile_read(K_UNIQ_ITEMS)[1], m.profile_read(K_W1_CATCHUP)[1]


def _tsync(m):
    import torch
    from aaerec._hip import T_W1_TSYNC
    m.join()
    torch.cuda.synchronize()
    return m.tensor(T_W1_TSYNC).view(torch.int32).cpu().numpy().copy()


def _outputs(m, losses, extra=None):
    """tsync as the steps left it, then (state_dict and adam_state bring every row up to date) all parameters and moments."""
    out = {"losses": np.asarray(losses, dtype=np.float32), "tsync": _tsync(m)}
    out.update(extra or {})
    for k, v in m.state_dict().items():
        out["p." + k] = np.asarray(v)
    for which in ("enc", "gen", "dec", "disc"):
        for name, mv in m.adam_state(which).items():
            if name == "step":
                out[f"{which}.step"] = np.asarray([mv])
            else:
                for tag, a in zip("mv", mv):
                    if a is not None:
                        out[f"{which}.{name}.{tag}"] = np.asarray(a)
    return out


def _assert_same(got, want):
    assert got.keys() == want.keys()
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k in want:
        if want[k].dtype == np.float32:
            assert np.all(np.isfinite(want[k])), k
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)


def _twins(monkeypatch, drive, N, h, B, max_nnz, want_inline, want_side, **kw):
    """drive(m) -> (losses, extra arrays); -> the two routes' outputs after asserting them equal and the launch counts."""
    outs = []
    for side, want in ((False, want_inline), (True, want_side)):
        m = _handle(monkeypatch, side, N, h, B, max_nnz, **kw)
        losses, extra = drive(m)
        counts = _launches(m)
        if want is not None:
            assert counts == want, f"{'side-stream' if side else 'inline'} route: (uniq_items, w1_catchup) launches {counts}, expected {want}"
        outs.append(_outputs(m, losses, extra))
        m.close()
    _assert_same(outs[0], outs[1])
    assert np.any(outs[1]["enc.lin1.weight.m"] != 0) and np.any(outs[1]["gen.lin1.weight.m"] != 0)
    return outs


def _steps(csr_of, B, steps, named=lambda s: True, before=None, after=None):
    """Step s runs rows [s B, (s + 1) B) of csr_of(m); named(s): step s names the batch of step s + 1 first."""
    def drive(m):
        csr = csr_of(m)
        losses, extra = [], {}
        for s in range(steps):
            if before:
                before(m, csr, s)
            if named(s) and s + 1 < steps:
                m.prefetch(csr, (s + 1) * B, B)
            m.step(csr, s * B, B)
            losses.append(m.losses())
            if after:
                after(m, csr, s, extra)
        return losses, extra
    return drive


def _device_csr(X):
    from aaerec._hip import DeviceCSR
    return lambda m: DeviceCSR(X, m.device)


def test_headline_shape_with_injected_draws(monkeypatch):
    """(a) tests/golden/step_headline.npz's shape and draws, 12 steps alternating its two batches, each named a step ahead."""
    from aaerec._hip import DeviceCSR
    from golden_util import Fixture
    fx = Fixture("step_headline")
    N, h, c, B = fx.cfg["N"], fx.cfg["h"], fx.cfg["c"], fx.cfg["B"]
    kw = fx.model_kwargs()

    def drive(m):
        m.load_params(fx.init_params())
        _launches(m)              # (loading flushes every row: the counters start at the first step)
        csrs =[DeviceCSR.from_arrays(*fx.batch(s), N, m.device) for s in range(fx.steps)]
        losses = []
        for s in range(12):
            k = s % fx.steps
            if s < 11:
                m.prefetch(csrs[(s + 1) % fx.steps], 0, B)
            m.step(csrs[k], 0, B, masks=fx.masks(k), z_real=fx.z[f"step{k}.z_real"])
            losses.append(m.losses())
        return losses, {}
    nnz = B * max(int(np.diff(fx.batch(s)[0]).max()) for s in range(fx.steps))
    _twins(monkeypatch, drive, N, h, B, nnz, (1, 1), (12, 12), c=c, params_seed=None, rng_mode="inject", **kw)


def test_gaps_table_wrap_and_lr_change(monkeypatch):
    """(b) 8 rows x 400 items (the smallest the fused output layer and the item lists take), 300 steps from 140 steps short of
    the table's wrap, the rates changed twice on the way; probe items return after gaps of 0, 1, 127, 128, 129 and 274 steps
    (kLazyReplay = 128 replayed steps, the rest in closed form), the other items after whatever 6 of 340 per row gives."""
    N, B, S = 400, 8, 300
    X = _corpus(N, S * B, seed=21, per_row=6, lo=60).tolil()
    at = {0: (20, 21), 1: (20, 22), 2: (20, 148), 3: (20, 149), 4: (20, 150), 5: (5, 280)}
    for item, steps in at.items():
        for s in steps:
            X[s * B + item % B, item] = 1.0
    X = X.tocsr()
    for item, (s0, s1) in at.items():
        hit = np.unique(X[:, item].nonzero()[0] // B)
        assert list(hit) == [s0, s1], (item, hit)

    def before(m, csr, s):
        from aaerec._hip import O_ENC, O_GEN
        if s == 0:
            m.load_adam(O_ENC, 1, step=WRAP - 140)
            m.load_adam(O_GEN, 1, step=WRAP - 140)
            _launches(m)          # (loading flushes every row: the counters start at the first step)
        if s in (100, 201):       # (with the next batch's list already built, as fit_steps would meet a scheduler)
            m.set_lr(0.002 if s == 100 else 0.0005, 0.003 if s == 100 else 0.001)
    outs = _twins(monkeypatch, _steps(_device_csr(X), B, S, before=before), N, 8, B, B * 7, (1, 1), (S, S))
    assert outs[0]["enc.step"][0] == WRAP - 140 + S
    # (as the last step left it: the last batch's rows at the last step, rows no batch ever named where load_adam put them)
    assert outs[0]["tsync"].max() == WRAP - 140 + S and outs[0]["tsync"].min() == WRAP - 140


def test_widest_batch_of_one_fused_launch(monkeypatch):
    """(c) 112 rows."""
    N, B = 4500, 112
    X = _corpus(N, 4 * B, seed=22, per_row=12)
    _twins(monkeypatch, _steps(_device_csr(X), B, 4), N, 12, B, B * 12, (1, 1), (4, 4))


def test_empty_and_full_intersection(monkeypatch):
    """(d) the next batch shares no item with the running one (every row of its list is caught up), then every item (every row is
    the running batch's: all skipped), then none again."""
    N, B = 4500, 100
    r = np.random.default_rng(24)
    rows = np.repeat(np.arange(B), 10)
    lowc = np.concatenate([np.sort(r.choice(2000, size=10, replace=False)) for _ in range(B)])
    highc = np.concatenate([np.sort(r.choice(np.arange(2000, N), size=10, replace=False)) for _ in range(B)])
    ones = np.ones(len(rows), dtype=np.float32)
    low = sp.csr_matrix((ones, (rows, lowc)), shape=(B, N))
    high = sp.csr_matrix((ones, (rows, highc)), shape=(B, N))
    perm = r.permutation(B)
    same_items = low[perm]                                   # the same item set as `low`, in other rows
    X = sp.vstack([low, high, low, same_items, high, low]).tocsr()
    assert low.multiply(high).nnz == 0 and set(same_items.indices) == set(low.indices)
    _twins(monkeypatch, _steps(_device_csr(X), B, 6), N, 8, B, B * 10, (1, 1), (6, 6))


def test_named_batch_not_run(monkeypatch):
    """(e) a batch named ahead and then not run: another batch runs instead, or the same rows under a new generation id - the
    step builds its own list in place (one launch of each kernel), and the rows caught up for nothing are simply up to date."""
    N, B = 4500, 100
    X = _corpus(N, 6 * B, seed=25, per_row=10)

    def drive(m):
        from aaerec._hip import DeviceCSR
        csr = DeviceCSR(X, m.device)
        losses = []
        m.prefetch(csr, 1 * B, B); m.step(csr, 0, B); losses.append(m.losses())          # builds batch 1's list
        m.prefetch(csr, 3 * B, B); m.step(csr, 2 * B, B); losses.append(m.losses())      # batch 2 runs instead: in place
        csr.touch()
        m.prefetch(csr, 4 * B, B); m.step(csr, 3 * B, B); losses.append(m.losses())      # batch 3 under a new id: in place
        m.step(csr, 4 * B, B); losses.append(m.losses())                                  # batch 4 as named: taken
        return losses, {}
    # in place: steps 0, 2 and 3; the side route adds one pair per prefetch that went out (3)
    _twins(monkeypatch, drive, N, 8, B, B * 10, (3, 3), (6, 6))


def test_a_step_with_nothing_named(monkeypatch):
    """(f) steps 0, 1, 3, 4 name their successor, step 2 does not: step 3 builds in place, nothing is left pending or half built."""
    N, B = 4500, 100
    X = _corpus(N, 6 * B, seed=26, per_row=10)
    _twins(monkeypatch, _steps(_device_csr(X), B, 6, named=lambda s: s != 2), N, 8, B, B * 10, (2, 2), (6, 6))


def test_epoch_boundary_through_fit_steps(monkeypatch):
    """(g) fit_steps() itself over two epochs of 5 batches, the last of 60 rows: the short batch named from a full one, and the
    first batch of the next epoch - other row ids, another generation - named from the short one."""
    import torch
    from aaerec._hip import K_UNIQ_ITEMS, K_W1_CATCHUP
    from aaerec.aae import AdversarialAutoEncoder
    N, B = 4500, 100
    X = _corpus(N, 4 * B + 60, seed=27, per_row=10)
    outs = []
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    for side in (False, True):
        if side:
            monkeypatch.setenv("AAE_NO_INLINE_PREFETCH", "1")
        else:
            monkeypatch.delenv("AAE_NO_INLINE_PREFETCH", raising=False)
        np.random.seed(5)
        torch.manual_seed(5)
        m = AdversarialAutoEncoder(n_hidden=8, n_code=C, batch_size=B, n_epochs=2, verbose=False, seed=3)
        it = m.fit_steps(X)
        losses = []
        for n, _ in zip(range(10), it):
            if n == 0:
                m.hip.profile_enable(True, kernels=(K_UNIQ_ITEMS, K_W1_CATCHUP))
            losses.append(m.hip.losses())
        assert len(losses) == 10
        counts = _launches(m.hip)
        outs.append((_outputs(m.hip, losses), counts))
        m.hip.close()
    _assert_same(outs[0][0], outs[1][0])
    # counted from the second step on (the first ran before the counters were on): fit_steps names every batch of an epoch but
    # its first, so the second epoch's first step builds in place on both routes; the side route adds the 3 + 4 batches named
    assert outs[0][1] == (1, 1) and outs[1][1] == (8, 8), (outs[0][1], outs[1][1])


def test_predict_and_export_straight_after_a_step(monkeypatch):
    """(h) predict and state_dict right behind a step that named its successor: both catch rows up themselves (every row of the
    predicted batch / of the matrix), on top of what the catch-up of the named batch did - and the step after still takes its list."""
    N, B = 4500, 100
    X = _corpus(N, 5 * B, seed=28, per_row=10)

    def after(m, csr, s, extra):
        if s == 1:
            extra["pred"] = m.predict(csr, 4 * B, B).cpu().numpy().copy()
            extra["tsync.after_predict"] = _tsync(m)
        if s == 2:
            extra["sd.mid"] = np.asarray(m.state_dict()["enc.lin1.weight"]).copy()
    _twins(monkeypatch, _steps(_device_csr(X), B, 5, after=after), N, 8, B, B * 10, None, None)


@pytest.mark.parametrize("kind", ["wide", "wide_bf16", "vae"])
def test_ineligible_handles_keep_the_side_stream(kind, monkeypatch):
    """(i) a batch beyond one fused launch (fp32, and bf16: row-blocked) and a VAE: the default handle launches exactly what the
    handle with the switch does."""
    N, B = 4500, (128 if kind != "vae" else 100)
    X = _corpus(N, 3 * B, seed=29, per_row=8)
    counts, outs = [], []
    for side in (False, True):
        kw = dict(dtype="bf16") if kind == "wide_bf16" else dict(vae=True, dropout=(0.0, 0.0)) if kind == "vae" else {}
        m = _handle(monkeypatch, side, N, 8, B, B * 8, params_seed=None if kind == "vae" else 4, **kw)
        from aaerec._hip import DeviceCSR
        csr = DeviceCSR(X, m.device)
        losses = []
        for s in range(3):
            if s < 2:
                m.prefetch(csr, (s + 1) * B, B)
            if kind == "vae":
                m.vae_step(csr, s * B, B)
            else:
                m.step(csr, s * B, B)
            losses.append(m.losses())
        counts.append(_launches(m))
        import torch
        torch.cuda.synchronize()
        outs.append({"losses": np.asarray(losses, dtype=np.float32), "w": np.asarray(m.state_dict()["enc.lin1.weight"])})
        m.close()
    assert counts[0] == counts[1] == (3, 3), counts
    if kind != "vae":       # (the VAE's loss series is held to its own reordering bound elsewhere; the route is the point here)
        np.testing.assert_array_equal(outs[0]["losses"], outs[1]["losses"])
        np.testing.assert_array_equal(outs[0]["w"].view(np.uint32), outs[1]["w"].view(np.uint32))
