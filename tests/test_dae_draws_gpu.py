"""DenoisingAutoEncoder(corrupt_draws='step'): both kinds of corruption drawn from the device generator (csrc/dae_corrupt.h;
stream 13 thins a CSR matrix, stream 14 is the Gauss noise of a step's dense input) against tests/device_rng.py, the NumPy
restatement of that generator, fed through the arguments the suite already pins to the reference (`keep=` / `noise=` of
partial_fit: tests/test_host_gpu.py).

Tolerances.  Zero corruption through partial_fit: the two models run the same kernels on the same values - equal bits.  Through
fit(): atol 2e-5, what tests/test_device_rng_gpu.py holds a step to (the gathered-rows path of fit() and the uploaded-batch path
of partial_fit may sum in another order).  Gauss corruption: atol 2e-5 - the restated Gaussian is within 5e-6 of the kernel's
(device_rng.py) and is scaled by noise_factor = 0.05, and the L1 norm is summed in another order (chunk sums + a correction per
entry instead of one sum over the row).  One wrong stream or step moves a weight by O(lr) = 2e-3, a hundred times the tolerance:
every comparison comes with a restatement off in one place that must miss."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import device_rng as R

pytestmark = pytest.mark.gpu

ZERO_STREAM, GAUSS_STREAM = 13, 14
SEED = 1234
ATOL = 2e-5                     # test_device_rng_gpu.py
N, H, C = 1000, 50, 20
LR = 2e-3
DROP = (0.2, 0.2)
P_ZERO = 0.3
ESTATE = "error -4"


@functools.lru_cache(maxsize=None)
def params(n_items):
    from oracle.dense_torch_port import init_params
    return init_params(n_items, H, C, seed=9)


def entry_keep(seed, step, rows, cols, n_rows, n_cols, p, sid=ZERO_STREAM):
    """The restated keep flag of every entry (rows[e], cols[e]) of a matrix [n_rows, n_cols] thinned for step `step`."""
    w = R.hash_cell(R.stream_key(seed, step, sid), np.arange(n_rows, dtype=np.int64), np.arange(n_cols, dtype=np.int64))
    return R.keep(w[rows, cols], p)


def csr_keep(seed, step, X, p, sid=ZERO_STREAM):
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return entry_keep(seed, step, rows, X.indices, X.shape[0], X.shape[1], p, sid)


@functools.lru_cache(maxsize=None)
def batches(n_items, rows, steps, seed=0, empty_row=3):
    """`steps` batches of `rows` documents of 1-9 items (ones), row `empty_row` of each empty."""
    r = np.random.default_rng(200 + seed)
    out = []
    for _ in range(steps):
        docs = [np.sort(r.choice(n_items, size=int(r.integers(1, 10)), replace=False)) if i != empty_row else np.zeros(0, dtype=np.int64)
                for i in range(rows)]
        ip = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
        idx = np.concatenate(docs).astype(np.int32)
        out.append(sp.csr_matrix((np.ones(len(idx), dtype=np.float32), idx, ip), shape=(rows, n_items)))
    return tuple(out)


def dae(n_items, batch_size, corrupt_draws="torch", seed=SEED, load=True, **kw):
    from aaerec.dae import DenoisingAutoEncoder
    m = DenoisingAutoEncoder(n_hidden=H, n_code=C, lr=LR, batch_size=batch_size, dropout=DROP, verbose=False, rng_mode="device",
                             seed=seed, corrupt_draws=corrupt_draws, **kw)
    m._build(n_items, 0)
    if load:
        m.hip.load_params(params(n_items))
    return m


def deviation(a, b):
    sa, sb = a.hip.state_dict(), b.hip.state_dict()
    assert sa.keys() == sb.keys()
    worst = max(sa, key=lambda k: float(np.abs(sa[k] - sb[k]).max()))
    return float(np.abs(sa[worst] - sb[worst]).max()), worst


def assert_same_bits(a, b, what):
    sa, sb = a.hip.state_dict(), b.hip.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{what}: {k}")


# ---- 1. aae_dae_thin against the restatement ----------------------------------------------------------------------------------
def test_dae_thin_equals_the_restatement_bit_for_bit():
    """Rows of 0, 1, 63, 64, 65 and 1 300 entries over 1 500 items (an empty row, one entry, either side of a wavefront, a row
    longer than any group's stride), values in [0.25, 1): a kept value passes unchanged, a dropped one is +0.  On a fresh handle
    the flags are those of step 1; after two training steps those of step 3."""
    from aaerec import _hip
    n_items, lens = 1500, (0, 1, 63, 64, 65, 1300)
    r = np.random.default_rng(1)
    docs = [np.sort(r.choice(n_items, size=n, replace=False)) for n in lens]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(docs).astype(np.int32)
    val = r.uniform(0.25, 1.0, len(idx)).astype(np.float32)
    rows = np.repeat(np.arange(len(lens)), lens)
    dev = _hip.HipAAE(n_items, H, C, max_batch=len(lens), rng_mode="device", seed=SEED, ae_only=True, dropout=DROP, gen_lr=LR, reg_lr=LR)
    dev.load_params(params(n_items))
    csr = _hip.DeviceCSR.from_arrays(ip, idx, val, n_items, dev.device)

    def check(step):
        want = val * entry_keep(SEED, step, rows, idx, len(lens), n_items, P_ZERO).astype(np.float32)
        assert 0 < np.count_nonzero(want) < len(want)
        thin = dev.dae_thin(csr, P_ZERO)
        assert thin.values is not csr.values and thin.indptr is csr.indptr and thin.indices is csr.indices
        assert thin.generation != csr.generation and thin.shape == csr.shape and thin.nnz_per_row_max == csr.nnz_per_row_max
        got = thin.values.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"step value {step}")
        np.testing.assert_array_equal(csr.values.cpu().numpy(), val)                      # the source is untouched
        np.testing.assert_array_equal(dev.dae_thin(csr, 0.0).values.cpu().numpy().view(np.uint32), val.view(np.uint32))
        scratch = _hip.DeviceCSR.from_arrays(ip, idx, val, n_items, dev.device)
        same = dev.dae_thin(scratch, P_ZERO, out=scratch.values)                          # in place
        assert same.values is scratch.values
        np.testing.assert_array_equal(scratch.values.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=f"in place, step value {step}")
        # off by one stream or one step: other flags
        for other in (entry_keep(SEED, step, rows, idx, len(lens), n_items, P_ZERO, sid=12), entry_keep(SEED, step + 1, rows, idx, len(lens), n_items, P_ZERO)):
            assert (val * other != want).sum() > 100
    check(1)
    for _ in range(2):
        dev.step(csr, 0, len(lens))
    check(3)


def test_calls_that_need_the_device_generator_are_refused_without_it():
    from aaerec import _hip
    csr = _hip.DeviceCSR(batches(N, 5, 1)[0], torch.device("cuda:0"))
    inj = _hip.HipAAE(N, H, C, max_batch=5, rng_mode="inject", ae_only=True, dense_noise=True)
    with pytest.raises(_hip.AaeHipError, match=ESTATE):
        inj.dae_thin(csr, P_ZERO)
    with pytest.raises(_hip.AaeHipError, match=ESTATE):
        inj.set_input_noise_gen(0.05)
    sparse = _hip.HipAAE(N, H, C, max_batch=5, rng_mode="device", seed=SEED, ae_only=True)      # no room for a dense input
    with pytest.raises(_hip.AaeHipError, match=ESTATE):
        sparse.set_input_noise_gen(0.05)
    with pytest.raises(_hip.AaeHipError):
        sparse.dae_thin(csr, 1.5)
    with pytest.raises(ValueError):
        sparse.dae_thin(csr, P_ZERO, out=torch.empty(3, device=csr.values.device))


# ---- 2. zero corruption through partial_fit -----------------------------------------------------------------------------------
def run_zero(steps, keep_of=None):
    """`steps` partial_fit steps on 37 rows (one empty): corrupt_draws='step', or the default fed keep_of(n, X) -> (model, losses)."""
    m = dae(N, 37, "torch" if keep_of else "step", noise_factor=P_ZERO)
    losses = []
    for n, X in enumerate(batches(N, 37, steps), start=1):
        m.partial_fit(X, keep=keep_of(n, X) if keep_of else None)
        losses.append(m.hip.losses()[0])
    assert np.isfinite(losses).all()
    return m, losses


def test_zero_corruption_of_partial_fit_is_stream_13_keyed_by_batch_row_and_opening_step():
    a, la = run_zero(3)
    b, lb = run_zero(3, lambda n, X: csr_keep(SEED, n, X, P_ZERO))
    assert la == lb, (la, lb)
    assert_same_bits(a, b, "corrupt_draws='step' vs the restated flags")
    for what, keep_of in (("stream 12", lambda n, X: csr_keep(SEED, n, X, P_ZERO, sid=12)),
                          ("step + 1", lambda n, X: csr_keep(SEED, n + 1, X, P_ZERO))):
        w, lw = run_zero(3, keep_of)
        dl, (dp, worst) = float(np.abs(np.subtract(la, lw)).max()), deviation(a, w)
        print(f"restatement off ({what}): losses differ by {dl:.3g}, parameters by {dp:.3g} ({worst})")
        assert dl > ATOL and dp > ATOL, (what, dl, dp)


# ---- 3. zero corruption through fit() -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus():
    return sp.vstack(batches(N, 30, 3, seed=5)).tocsr()            # 90 x 1 000, three empty rows


def fit_step_mode(torch_seed, seed=SEED):
    """fit() with corrupt_draws='step' from params(N): two epochs of three batches (40, 40, 10 rows)."""
    from aaerec.dae import DenoisingAutoEncoder
    m = DenoisingAutoEncoder(n_hidden=H, n_code=C, lr=LR, batch_size=40, n_epochs=2, dropout=DROP, verbose=False, rng_mode="device",
                             seed=seed, corrupt_draws="step", noise_factor=P_ZERO)
    build = m._build

    def build_and_load(*a, **kw):
        build(*a, **kw)
        m.hip.load_params(params(N))
    m._build = build_and_load
    torch.manual_seed(torch_seed)
    np.random.seed(11)
    m.fit(corpus())
    return m


def test_zero_corruption_of_fit_thins_the_corpus_once_per_epoch_by_the_seed_alone():
    X = corpus()
    a = fit_step_mode(1)
    # the same permutations through partial_fit: row = corpus row, step = the epoch's first step (1, then 4)
    b = dae(N, 40, "torch", noise_factor=P_ZERO)
    np.random.seed(11)
    for first_step in (1, 4):
        perm = np.arange(X.shape[0])
        np.random.shuffle(perm)
        for start in range(0, X.shape[0], 40):
            idx = perm[start:start + 40]
            Xb = X[idx].tocsr()
            Xb.sort_indices()
            rows = np.repeat(idx, np.diff(Xb.indptr))
            b.partial_fit(Xb, keep=entry_keep(SEED, first_step, rows, Xb.indices, X.shape[0], N, P_ZERO))
    dp, worst = deviation(a, b)
    print(f"fit() vs the replay through partial_fit(keep=): parameters differ by {dp:.3g} ({worst})")
    assert dp <= ATOL, (dp, worst)
    assert_same_bits(a, fit_step_mode(2), "the same seed under another torch.manual_seed")
    dq, worst = deviation(a, fit_step_mode(1, seed=SEED + 1))
    assert dq > ATOL, (dq, worst)


# ---- 4. Gauss corruption ---------------------------------------------------------------------------------------------------------
NG, BG, NF = 1500, 5, 0.05      # past one 1 024-thread stride, no multiple of 64; 5 rows -> 6 column chunks of 256 a row


def run_gauss(normalize, rng_rows, noise_of=None, tail=False):
    """Three corrupt='gauss' steps on 5 rows (one empty): corrupt_draws='step', or the default fed noise_of(n) -> (model, losses).
    tail: one more step of the handle without a request (the sparse path)."""
    m = dae(NG, BG, "torch" if noise_of else "step", corrupt="gauss", noise_factor=NF, normalize_inputs=normalize)
    if rng_rows:
        m.hip.set_rng_rows(*rng_rows)
    bs = batches(NG, BG, 4, seed=2, empty_row=1)
    losses = []
    for n, X in enumerate(bs[:3], start=1):
        if n == 2:       # a request of the other kind is pending: the later call (partial_fit's) wins
            if noise_of:
                m.hip.set_input_noise_gen(3.0)
            else:
                m.hip.set_input_noise(torch.full((BG, NG), 9.0))
        m.partial_fit(X, noise=noise_of(n) if noise_of else None)
        losses.append(m.hip.losses()[0])
    if tail:
        from aaerec import _hip
        m.hip.step(_hip.DeviceCSR(bs[3], m.hip.device), 0, BG)
        losses.append(m.hip.losses()[0])
    assert np.isfinite(losses).all()
    return m, losses


def restated_noise(step, row0=0, sid=GAUSS_STREAM):
    return R.gauss(SEED, step, sid, BG, NG, row0).astype(np.float32) * np.float32(NF)


@pytest.mark.parametrize("normalize,rng_rows", [(True, None), (False, None), (True, (7, 20))])
def test_gauss_corruption_is_stream_14_keyed_by_global_row_and_the_opened_step(normalize, rng_rows):
    row0 = rng_rows[0] if rng_rows else 0
    a, la = run_gauss(normalize, rng_rows, tail=True)
    b, lb = run_gauss(normalize, rng_rows, lambda n: restated_noise(n, row0), tail=True)
    dl, (dp, worst) = float(np.abs(np.subtract(la, lb)).max()), deviation(a, b)
    print(f"normalize {normalize}, rows {rng_rows}: losses differ by {dl:.3g}, parameters by {dp:.3g} ({worst})")
    assert dl <= ATOL and dp <= ATOL, (dl, dp, worst)
    if rng_rows:
        return
    a, la = run_gauss(normalize, None)
    for what, noise_of in (("stream 12", lambda n: restated_noise(n, sid=12)), ("step + 1", lambda n: restated_noise(n + 1)),
                           ("row + 1", lambda n: restated_noise(n, row0=1))):
        w, lw = run_gauss(normalize, None, noise_of)
        dl, (dp, worst) = float(np.abs(np.subtract(la, lw)).max()), deviation(a, w)
        print(f"restatement off ({what}): losses differ by {dl:.3g}, parameters by {dp:.3g} ({worst})")
        assert dp > ATOL, (what, dl, dp)


# ---- 5. resume -------------------------------------------------------------------------------------------------------------------
def test_resumed_dae_equals_the_unbroken_run():
    """Four partial_fit steps in 'step' mode, zero corruption; stored after two (the calls of tests/test_checkpoint_gpu.py) into a
    second model that runs the last two: the restored step counter keys steps 3 and 4 of both - equal bits."""
    from test_checkpoint_gpu import abi_store, abi_load, assert_same_checkpoint
    bs = batches(N, 37, 4)
    a = dae(N, 37, "step", noise_factor=P_ZERO)
    for X in bs[:2]:
        a.partial_fit(X)
    ck = abi_store(a.hip)
    la = [a.partial_fit(X).hip.losses()[0] for X in bs[2:]]
    b = dae(N, 37, "step", noise_factor=P_ZERO, load=False)
    abi_load(b.hip, ck)
    lb = [b.partial_fit(X).hip.losses()[0] for X in bs[2:]]
    assert la == lb, (la, lb)
    assert_same_checkpoint(abi_store(a.hip), abi_store(b.hip), "unbroken run vs resumed run")
    assert_same_bits(a, b, "unbroken run vs resumed run")
