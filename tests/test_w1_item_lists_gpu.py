"""The first layer's update from the per-batch item row lists (csrc/w1_lists.h) against the path that collects every item's
rows itself (AAE_NO_ITEM_LISTS=1): two handles from the same seed run the same full steps, a different batch each step, and
every bit of enc.lin1 (weight, bias), of both Adam moment sets of each, of every other parameter and of the three losses
must agree - the lists change where the row lists are derived, never the order of a sum.

Shapes: the smallest that still reach every branch (the hybrid form of the update needs n_items >= 40 x rows); hidden 8 or
12, code 4.  The "row counts" case of 640 items x 16 rows cannot hold an item in 17 rows, so it runs twice: 640 x 16 with
items in exactly 1, 2 and 16 rows, and 720 x 18 with items in exactly 1, 2, 16 and 17 rows.

Every handle here is created with AAE_SPLIT_ANY=1 - the output layer as critical + deferred launch, the form bench.py's shape
runs - and the two handles of a test differ in AAE_NO_ITEM_LISTS alone.  Measured, the reason: in the single-launch form that
shapes this small take by default the RECONSTRUCTION loss is not reproducible from run to run on the path without lists either.
csrc/dec_fused.h's BCE phase adds each entry's correction of the loss to the thread that holds the entry's position in its tile
bucket, and the order inside a bucket is whatever the counting sort's atomics left (csrc/buckets.h): one step's value flips by one ulp
(5.96e-8 at 0.7) where the sum lies near an fp32 rounding boundary; no gradient does - every parameter and moment agreed in every run.
Forty runs of the named-ahead scenario against the first, single-launch form: 10 and 11 differ on the library before this change
(without | with the switch, which is no path there), 18 to 28 on this one, and in three of six runs of this file one of its thirteen
tests failed on that value.  With the split form: none of 80 runs differs and four runs of the file passed.  The adversarial losses
and everything else are asserted first, the reconstruction loss - the same bit equality - last."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

C = 4


def _corpus(N, B, steps, seed, per_row=12, head=8, fixed=None, values=False):
    """steps x B documents: `per_row` random items each + each of `head` head items with probability 1/2 (items in many rows:
    the overflow slots) + the (item -> rows of every batch) pairs of `fixed`."""
    r = np.random.default_rng(seed)
    rows, cols = [], []
    fixed = fixed or {}
    for s in range(steps):
        for b in range(B):
            items = set(int(i) for i in r.choice(np.arange(head + 64, N), size=min(per_row, N - head - 64), replace=False))
            items |= {i for i in range(head) if r.random() < 0.5}
            items |= {it for it, rr in fixed.items() if b in rr}
            items -= {it for it, rr in fixed.items() if b not in rr}
            rows += [s * B + b] * len(items)
            cols += sorted(items)
    data = np.ones(len(rows), dtype=np.float32)
    if values:
        data = r.choice(np.asarray([0.25, 0.5, 1.0], dtype=np.float32), size=len(rows))
    return sp.csr_matrix((data, (rows, cols)), shape=(steps * B, N))


def _outputs(m, losses):
    import torch
    torch.cuda.synchronize()
    out = {"losses": np.asarray(losses)}
    for k, v in m.state_dict().items():
        out["p." + k] = np.asarray(v)
    for which in ("enc", "gen"):
        st = m.adam_state(which)
        for name in ("lin1.weight", "lin1.bias"):
            out[f"{which}.{name}.m"], out[f"{which}.{name}.v"] = np.asarray(st[name][0]), np.asarray(st[name][1])
    return out


def _run(monkeypatch, no_lists, N, h, B, X, steps, drive=None, max_nnz=None, **kw):
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle.dense_torch_port import init_params
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")       # (the module's docstring says why)
    if no_lists:
        monkeypatch.setenv("AAE_NO_ITEM_LISTS", "1")
    else:
        monkeypatch.delenv("AAE_NO_ITEM_LISTS", raising=False)
    per_row = int(np.diff(X.indptr).max())
    m = HipAAE(N, h, C, max_batch=B, max_nnz=max_nnz if max_nnz is not None else B * per_row, rng_mode="device", seed=11,
               dropout=(0.2, 0.2), **kw)
    m.load_params(init_params(N, h, C, seed=4))
    csr = DeviceCSR(X, m.device)
    losses = []
    for s in range(steps):
        if drive is not None:
            drive(m, csr, s, B)
        else:
            m.step(csr, s * B, B)
        losses.append(m.losses())
    out = _outputs(m, losses)
    m.close()
    return out


def _assert_same(got, want):
    assert got.keys() == want.keys()
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k in want:
        if k != "losses":
            assert np.all(np.isfinite(want[k])), k
            np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    np.testing.assert_array_equal(got["losses"][:, 1:], want["losses"][:, 1:], err_msg="disc / gen loss")
    np.testing.assert_array_equal(got["losses"][:, 0], want["losses"][:, 0],
                                  err_msg="reconstruction loss (all else agreed)")


def _both(monkeypatch, *a, **kw):
    got, want = _run(monkeypatch, False, *a, **kw), _run(monkeypatch, True, *a, **kw)
    _assert_same(got, want)
    # the steps trained the first layer at all: its rows moved away from their start
    assert np.any(want["enc.lin1.weight.m"] != 0) and np.any(want["gen.lin1.weight.m"] != 0)


@pytest.mark.parametrize("N,B,counts", [(640, 16, (1, 2, 16)), (720, 18, (1, 2, 16, 17))])
def test_row_counts_around_a_record(N, B, counts, monkeypatch):
    """Named items in exactly 1, 2, 16 (a full record) and 17 (the first overflow) rows of every batch."""
    fixed = {100 + 40 * i: set(range(B - n, B)) for i, n in enumerate(counts)}
    X = _corpus(N, B, 3, seed=1, per_row=6, head=0, fixed=fixed, values=True)
    for it, rr in fixed.items():
        assert all(X[s * B:(s + 1) * B, it].nnz == len(rr) for s in range(3))
    _both(monkeypatch, N, 8, B, X, 3)


def test_an_item_in_every_row(monkeypatch):
    N, B = 4500, 112
    X = _corpus(N, B, 3, seed=2, fixed={77: set(range(B))})
    assert X[:B, 77].nnz == 112
    _both(monkeypatch, N, 12, B, X, 3)


def test_popular_tile(monkeypatch):
    """Every row holds the same 32 items of one tile (3 200 entries: more than 256 and more than 1 024 in the tile, 32 overflow
    slots) beside a few others."""
    N, B = 4500, 100
    X = _corpus(N, B, 3, seed=3, per_row=3, head=0, fixed={i: set(range(B)) for i in range(64, 96)})
    assert X[:B, 64:96].nnz == 3200
    _both(monkeypatch, N, 8, B, X, 3)


def test_ragged_last_tile(monkeypatch):
    N, B = 4001, 100
    X = _corpus(N, B, 3, seed=4, fixed={4000: set(range(0, B, 3)), 3999: {5}, 3970: set(range(40))})
    assert N % 32 != 0 and X[:B, 4000].nnz == 34
    _both(monkeypatch, N, 8, B, X, 3)


def test_odd_row_count(monkeypatch):
    N, B = 4500, 5
    X = _corpus(N, B, 4, seed=5, head=3)
    _both(monkeypatch, N, 12, B, X, 4)


def test_stale_records(monkeypatch):
    """Many distinct items, then few, then many again: records and overflow slots of an earlier batch lie behind the count."""
    N, B = 4500, 100
    many = _corpus(N, B, 1, seed=6, per_row=30)
    few = _corpus(N, B, 1, seed=7, per_row=0, head=0, fixed={9: set(range(B)), 200: set(range(3)), 4100: {50}})
    many2 = _corpus(N, B, 1, seed=8, per_row=30)
    X = sp.vstack([many, few, many2, few]).tocsr()
    _both(monkeypatch, N, 8, B, X, 4, max_nnz=B * 40)


def test_item_count_at_the_cap(monkeypatch):
    """Every entry of the batch is an item of its own: the distinct-item count reaches max_nnz."""
    N, B, L = 4500, 100, 40
    r = np.random.default_rng(9)
    cols = np.concatenate([r.permutation(N)[:B * L] for _ in range(3)])
    rows = np.repeat(np.arange(3 * B), L)
    X = sp.csr_matrix((np.ones(len(cols), dtype=np.float32), (rows, cols)), shape=(3 * B, N))
    _both(monkeypatch, N, 8, B, X, 3, max_nnz=B * L)


def test_batches_named_ahead(monkeypatch):
    """The step after a prefetch takes its item list from the second list set (what fit_steps does for every batch of an epoch
    but the last): every step names the batch after it."""
    N, B = 4500, 100
    X = _corpus(N, B, 5, seed=10)

    def drive(m, csr, s, B):
        m.prefetch(csr, (s + 1) * B, B)
        m.step(csr, s * B, B)
    _both(monkeypatch, N, 8, B, X, 4, drive=drive)


def test_fit_steps(monkeypatch):
    """fit_steps() itself: shuffled row ids, every batch named a step ahead - four steps of an epoch of five."""
    import torch
    from aaerec.aae import AdversarialAutoEncoder
    N, B = 4500, 100
    X = _corpus(N, B, 5, seed=12)
    outs = []
    monkeypatch.setenv("AAE_SPLIT_ANY", "1")
    for no_lists in (False, True):
        if no_lists:
            monkeypatch.setenv("AAE_NO_ITEM_LISTS", "1")
        else:
            monkeypatch.delenv("AAE_NO_ITEM_LISTS", raising=False)
        np.random.seed(5)
        torch.manual_seed(5)
        m = AdversarialAutoEncoder(n_hidden=8, n_code=C, batch_size=B, n_epochs=1, verbose=False, seed=3)
        losses = [m.hip.losses() for _ in zip(range(4), m.fit_steps(X))]
        assert len(losses) == 4
        outs.append(_outputs(m.hip, losses))
        m.hip.close()
    _assert_same(outs[0], outs[1])
    assert np.any(outs[1]["gen.lin1.weight.m"] != 0)


def test_sgd_with_an_lr_change(monkeypatch):
    N, B = 4500, 100
    X = _corpus(N, B, 4, seed=13)

    def drive(m, csr, s, B):
        if s == 2:
            m.set_lr(0.02, 0.005)
        m.step(csr, s * B, B)
    got, want = (_run(monkeypatch, nl, N, 8, B, X, 4, drive=drive, optimizer="sgd", gen_lr=0.05, reg_lr=0.01) for nl in (False, True))
    _assert_same(got, want)
    from oracle.dense_torch_port import init_params
    assert np.any(want["p.enc.lin1.weight"] != np.asarray(init_params(N, 8, C, seed=4)["enc.lin1.weight"]))


def test_bf16(monkeypatch):
    N, B = 4500, 100
    X = _corpus(N, B, 3, seed=14)
    _both(monkeypatch, N, 8, B, X, 3, dtype="bf16")


def test_split_api_takes_the_fallback(monkeypatch):
    """The phases called one by one (aae_ae_encode, aae_ae_decode_backward, aae_ae_encoder_backward, aae_disc_gen): no launch in
    front of the update carries the builder there, so a default handle runs the path of AAE_NO_ITEM_LISTS=1 - also in the
    step after a fused step that did build lists."""
    N, B = 4500, 100
    X = _corpus(N, B, 4, seed=15)

    def drive(m, csr, s, B):
        if s == 1:
            m.step(csr, s * B, B)
            return
        z = m.ae_encode(csr, s * B, B)
        m.ae_encoder_backward(m.ae_decode_backward(z))
        m.disc_gen()
    _both(monkeypatch, N, 8, B, X, 4, drive=drive)
