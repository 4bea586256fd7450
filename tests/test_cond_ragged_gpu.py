"""aae_bag_csr_encode / aae_bag_csr_update (csrc/cond_csr.h) on the device: the kernels against the padded kernels on the same
lists (bit for bit), every fixed capacity of the new kernels crossed by one, per-sample weights against the restatement and
torch, and the models - a fit whose trainable conditions read resident bags against the same fit on the padded route."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bag_cases as BC
import ragged_cases as RC

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---- 1. the kernels against the padded kernels ---------------------------------------------------------------------------------
def _blocks(dout):
    """(NaN-filled encode block, its column slice; NaN-filled gradient block holding dout, its column slice)."""
    dev = torch.device("cuda")
    rows, dim = dout.shape
    block = torch.full((rows, dim + 5), float("nan"), device=dev)
    dblock = torch.full((rows, dim + 3), float("nan"), device=dev)
    dblock[:, 2:2 + dim] = torch.from_numpy(dout).to(dev)
    return block, block[:, 3:3 + dim], dblock[:, 2:2 + dim]


def _finish(block, dim, table, m, v, scratch):
    block = block.cpu().numpy()
    assert np.isnan(block[:, :3]).all() and np.isnan(block[:, 3 + dim:]).all(), "the encode wrote outside its columns"
    assert not scratch.any(), "the gradient scratch is left zero"
    return block[:, 3:3 + dim], table.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def _padded_step(table, lists, dout, reduce, pad, sparse, lr=1e-2, step=1):
    from aaerec import _hip
    dev = torch.device("cuda")
    table = torch.from_numpy(table).to(dev)
    m, v, scratch = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    idx = torch.from_numpy(RC.padded(lists, pad).astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(dev)
    block, out, d = _blocks(dout)
    _hip.bag_encode(table, idx, out, reduce=reduce, padding_idx=pad)
    _hip.bag_update(table, m, v, idx, d, lr, step, reduce=reduce, padding_idx=pad, grad_scratch=scratch, sparse=sparse)
    return _finish(block, dout.shape[1], table, m, v, scratch)


def _csr_step(table, lists, dout, reduce, pad, sparse, lr=1e-2, step=1, permute=None, weights=None):
    """The same step from a resident CSR.  permute (a seed): the lists are scattered over a larger corpus and the step names
    them by a row_ids window; None: the contiguous rows 0 .. rows of a corpus that holds exactly them."""
    from aaerec import _hip
    dev = torch.device("cuda")
    table = torch.from_numpy(table).to(dev)
    m, v, scratch = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    if permute is None:
        bags = _hip.DeviceBags(lists, dev, weights=None if weights is None else RC.flat(lists, weights)[2])
        view = bags.window(row0=0, rows=len(lists))
    else:
        rng = np.random.default_rng(permute)
        n = len(lists) + 5
        ids = rng.permutation(n)[:len(lists)]
        corpus = [[int(j) for j in rng.integers(0, table.shape[0], size=3)] for _ in range(n)]
        for r, i in enumerate(ids):
            corpus[i] = lists[r]
        bags = _hip.DeviceBags(corpus, dev)
        view = bags.window(torch.from_numpy(ids.astype(np.int32)).to(dev))
    block, out, d = _blocks(dout)
    _hip.bag_csr_encode(table, view, out, reduce=reduce, padding_idx=pad)
    _hip.bag_csr_update(table, m, v, view, d, lr, step, reduce=reduce, padding_idx=pad, grad_scratch=scratch, sparse=sparse)
    return _finish(block, dout.shape[1], table, m, v, scratch)


def _off_grid(seed, rows, dim, vocab, pad, lists=None):
    """Table and dout OFF the grid - every sum rounds, so a different order of the additions shows in the bits - and the lists
    of ragged_cases.make_lists."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((vocab, dim)).astype(f32)
    if pad >= 0:
        table[pad] = 0
    lists = RC.make_lists(rng, rows, vocab, pad) if lists is None else lists
    return table, lists, rng.standard_normal((len(lists), dim)).astype(f32)


def _same(got, want, tag):
    for name, a, b in zip(("encode", "table", "exp_avg", "exp_avg_sq"), got, want):
        assert np.array_equal(a, b, equal_nan=True), f"{tag}: {name} differs"


@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
@pytest.mark.parametrize("reduce", list(BC.NAMES), ids=list(BC.NAMES.values()))
def test_kernels_equal_the_padded_kernels_bit_for_bit(reduce, sparse):
    """rows {1, 3, 65} x dim {1, 7, 64, 65, 256} x vocab {2, 40} x padding_idx {-1, 0}, lists of 0-5 values plus one of 130:
    an empty list, an all-out-of-vocabulary list, a table row named three times in one list and again in two others, the
    indices -3, vocab and 2^30 (ragged_cases.make_lists).  Encode, table, moments: the padded kernels' bits, from the
    contiguous rows and from a permuted row_ids window; blocks are column slices of NaN-filled wider ones; twice."""
    for rows in (1, 3, 65):
        for dim in (1, 7, 64, 65, 256):
            for vocab in (2, 40):
                for pad in (-1, 0):
                    tag = f"{BC.NAMES[reduce]} rows {rows} dim {dim} vocab {vocab} pad {pad}"
                    table, lists, dout = _off_grid(1000 * reduce + rows + dim + vocab + pad, rows, dim, vocab, pad)
                    if rows == 65:
                        flat = [j for row in lists for j in row]
                        assert [] in lists and [vocab, -3, 2 ** 30] in lists and -3 in flat and 2 ** 30 in flat
                        assert max(len(row) for row in lists) == 130
                        assert lists[3].count(lists[3][0]) >= 3 and lists[3][0] in lists[5] and lists[3][0] in lists[7]
                    want = _padded_step(table, lists, dout, reduce, pad, sparse)
                    got = _csr_step(table, lists, dout, reduce, pad, sparse)
                    _same(got, want, tag)
                    _same(_csr_step(table, lists, dout, reduce, pad, sparse), got, tag + " (second run)")
                    _same(_csr_step(table, lists, dout, reduce, pad, sparse, permute=rows + dim), want, tag + " (row_ids window)")


def test_kernels_equal_the_restatement_on_the_grid():
    """On the 1/8 grid (exact sums, tie-free) the encodes equal ragged_cases' bit for bit in every mode, and a step lands on
    the restatement's table and moments at test_cond_bag_gpu.py's tolerances."""
    for reduce in BC.NAMES:
        for sparse in (False, True):
            c = RC.make_case(40 + reduce, 65, 7, 40, reduce, 0)
            p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
            want = RC.step(p, m, v, c["lists"], reduce, 0, c["dout"], 1e-2, 1, sparse)
            out, gp, gm, gv = _csr_step(c["table"], c["lists"], c["dout"], reduce, 0, sparse)
            if reduce in (BC.SUM, BC.MAX_PAD0, BC.MAX):
                assert np.array_equal(out, want), BC.NAMES[reduce]
            else:
                assert (np.abs(out - want) <= 2 * np.spacing(np.abs(want))).all(), BC.NAMES[reduce]
            np.testing.assert_allclose(gm, m, atol=2e-8, rtol=2e-4)
            np.testing.assert_allclose(gv, v, atol=1e-12, rtol=2e-4)
            np.testing.assert_allclose(gp, p, atol=1e-5, rtol=0)


# ---- 2. capacities ---------------------------------------------------------------------------------------------------------------
def _lists_of(rng, lengths, vocab):
    return [[int(j) for j in rng.integers(0, vocab, size=n)] for n in lengths]


def _capacity_cases():
    from aaerec import _hip
    rng = np.random.default_rng(11)
    sort, scan, waves = _hip.BAG_CSR_SORT, _hip.BAG_CSR_SCAN, _hip.BAG_CSR_UPDATE_WAVES
    assert (sort, scan, waves) == (4096, 1024, 16384)
    return {
        # one key more than a workgroup sorts in LDS: two runs and one merge pass
        "BAG_CSR_SORT + 1": (_lists_of(rng, [sort - 100, 94, 7], 40), 40),
        # one row more than the row scan takes in a round
        "BAG_CSR_SCAN + 1": (_lists_of(rng, rng.integers(0, 3, size=scan + 1), 40), 40),
        # one sorted position more than the update launch's grid covers in a round (and three merge passes)
        "BAG_CSR_UPDATE_WAVES + 1": (_lists_of(rng, [4000, 4000, 4000, 4000, waves + 1 - 16000], 40), 40),
        # one table row named by more entries than the largest capacity
        "hot row": ([[1] * (waves + 6), [0, 1, 1], [1] * 70 + [0]], 2),
    }


@pytest.mark.parametrize("name", ["BAG_CSR_SORT + 1", "BAG_CSR_SCAN + 1", "BAG_CSR_UPDATE_WAVES + 1", "hot row"])
def test_capacities_crossed_by_one(name):
    """Each fixed capacity of cond_csr.h (exported by _hip as BAG_CSR_*) crossed by one entry or row, and one table row named
    by more entries than the largest of them; dim 7, against the padded kernels, bit for bit.  The hot row runs in sum and
    mean mode under both optimisers, the others in a sum, a mean and a max mode."""
    from aaerec import _hip
    lists, vocab = _capacity_cases()[name]
    entries = sum(len(row) for row in lists)
    if name == "BAG_CSR_SORT + 1":
        assert entries == _hip.BAG_CSR_SORT + 1
    elif name == "BAG_CSR_SCAN + 1":
        assert len(lists) == _hip.BAG_CSR_SCAN + 1
    elif name == "BAG_CSR_UPDATE_WAVES + 1":
        assert entries == _hip.BAG_CSR_UPDATE_WAVES + 1
    else:
        assert sum(row.count(1) for row in lists) > max(_hip.BAG_CSR_SORT, _hip.BAG_CSR_SCAN, _hip.BAG_CSR_UPDATE_WAVES)
    modes = [(BC.SUM, -1, True), (BC.MEAN_WIDTH, 0, False)] if name == "hot row" else \
        [(BC.SUM, -1, True), (BC.MEAN_COUNT, 0, False), (BC.MAX_PAD0, 0, True)]
    for reduce, pad, sparse in modes:
        table, _, dout = _off_grid(7 + reduce, len(lists), 7, vocab, pad, lists=lists)
        want = _padded_step(table, lists, dout, reduce, pad, sparse)
        got = _csr_step(table, lists, dout, reduce, pad, sparse)
        _same(got, want, f"{name} {BC.NAMES[reduce]}")


# ---- 3. per-sample weights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
def test_per_sample_weights_in_sum_mode(sparse):
    """Weights, table and dout on the 1/8 grid (every product and sum exact): the encode equals ragged_cases' bit for bit and
    torch's nn.EmbeddingBag(input, offsets, per_sample_weights) bit for bit; table and moments at test_cond_bag_gpu.py's
    tolerances against both (the optimisers' arithmetic is held to torch at those, never bit for bit)."""
    for pad in (-1, 0):
        for rows, dim, vocab in ((3, 7, 40), (65, 65, 40), (65, 256, 2)):
            rng = np.random.default_rng(rows + dim)
            c = RC.make_case(9 + rows + pad, rows, dim, vocab, BC.SUM, pad, outside=False)
            wts = RC.make_weights(rng, c["lists"])
            p, m, v = c["table"].copy(), np.zeros_like(c["table"]), np.zeros_like(c["table"])
            want = RC.step(p, m, v, c["lists"], BC.SUM, pad, c["dout"], 1e-2, 1, sparse, wts)
            outs, tp, tm, tv = RC.torch_steps(c["table"], [c["lists"]], BC.SUM, pad, [c["dout"]], 1e-2, sparse, [wts])
            got = _csr_step(c["table"], c["lists"], c["dout"], BC.SUM, pad, sparse, weights=wts)
            _same(_csr_step(c["table"], c["lists"], c["dout"], BC.SUM, pad, sparse, weights=wts), got, "second run")
            out, gp, gm, gv = got
            assert np.array_equal(out, want) and np.array_equal(out, outs[0])
            for wm, wv, wp in ((m, v, p), (tm, tv, tp)):
                np.testing.assert_allclose(gm, wm, atol=2e-8, rtol=2e-4)
                np.testing.assert_allclose(gv, wv, atol=1e-12, rtol=2e-4)
                np.testing.assert_allclose(gp, wp, atol=1e-5, rtol=0)


# ---- 4. the models ---------------------------------------------------------------------------------------------------------------
N_DOCS, N_ITEMS, BATCH, HIDDEN = 40, 120, 16, 20


def _corpus(seed=0):
    rng = np.random.default_rng(seed)
    X = sp.random(N_DOCS, N_ITEMS, density=0.08, format="csr", random_state=3, dtype=np.float32)
    X.data[:] = 1
    names = ["a%d" % i for i in range(12)]
    authors = [[names[j] for j in rng.integers(0, 12, size=int(rng.integers(0, 5)))] for _ in range(N_DOCS)]
    authors[0] = [names[3]] * 3 + [names[1]]
    authors[1] = []
    return X, authors


def _fit(kind, resident, cond_of, data_of=None, stop_after=None, hook=None):
    """One seeded fit of two epochs; returns (model, condition, condition data, test-time condition data)."""
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec.condition import ConditionList
    from aaerec.dae import DenoisingAutoEncoder
    from aaerec.vae import VAE
    X, authors = _corpus()
    torch.manual_seed(7)
    np.random.seed(7)
    cond = cond_of()
    data = cond.fit_transform(authors) if data_of is None else data_of(cond, authors)
    conds = ConditionList([("author", cond)])
    kw = dict(n_hidden=HIDDEN, n_code=10, n_epochs=2, batch_size=BATCH, conditions=conds, verbose=False, rng_mode="reference")
    if kind == "aae":
        m = AdversarialAutoEncoder(**kw)
    elif kind == "dae":
        m = DenoisingAutoEncoder(**kw)
    else:
        m = VAE(N_ITEMS, N_ITEMS, **kw)
    m.resident_conditions = resident
    if hook is not None:
        hook(m)
    m.fit(X, condition_data=[data])
    return m, cond, X, data


def _weights_of(m):
    sd = m.state_dict() if hasattr(m, "state_dict") else m.hip.state_dict()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}


def _table_state(cond):
    w = cond.embedding.weight if hasattr(cond, "embedding") else cond.embedding_bag.weight
    st = cond.optimizer.state[w]
    return w.detach().cpu().numpy(), float(st["step"]), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


def _assert_same_fit(a, b, tag):
    (ma, ca, X, da), (mb, cb, _, db) = a, b
    wa, wb = _weights_of(ma), _weights_of(mb)
    assert wa.keys() == wb.keys()
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), f"{tag}: {k}"
    for name, x, y in zip(("table", "step", "exp_avg", "exp_avg_sq"), _table_state(ca), _table_state(cb)):
        assert np.array_equal(x, y), f"{tag}: condition {name}"
    torch.manual_seed(11)                       # (rng_mode='reference': the VAE draws its eps from torch's generator)
    ids_a, vals_a = ma.predict_topk(X, k=10, condition_data=[da])
    torch.manual_seed(11)
    ids_b, vals_b = mb.predict_topk(X, k=10, condition_data=[db])
    assert np.array_equal(ids_a, ids_b) and np.array_equal(vals_a, vals_b), f"{tag}: predict_topk"


@pytest.mark.parametrize("sparse", [True, False], ids=["sparse_adam", "adam"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_aae_fit_with_resident_conditions_equals_the_padded_route(reduce, sparse):
    from aaerec.condition import CategoricalCondition
    mk = lambda: CategoricalCondition(8, reduce=reduce, sparse=sparse)          # noqa: E731
    a, b = _fit("aae", True, mk), _fit("aae", False, mk)
    assert a[0]._is_device_native() and float(_table_state(a[1])[1]) == 6.0
    _assert_same_fit(a, b, f"{reduce} sparse {sparse}")


@pytest.mark.parametrize("kind", ["vae", "dae"])
def test_vae_and_dae_fit_with_resident_conditions_equal_the_padded_route(kind):
    from aaerec.condition import CategoricalCondition
    mk = lambda: CategoricalCondition(8, reduce="mean", sparse=True)           # noqa: E731
    _assert_same_fit(_fit(kind, True, mk), _fit(kind, False, mk), kind)


def test_a_one_value_condition_takes_its_window_on_the_device():
    """reduce=None: the column is resident as an int32 tensor, a step selects its rows there and hands aae_bag_* a block of width 1."""
    from aaerec.condition import CategoricalCondition
    mk = lambda: CategoricalCondition(8, reduce=None, sparse=True)             # noqa: E731
    one = lambda cond, authors: cond.fit_transform([row[0] if row else "nobody" for row in authors])      # noqa: E731
    _assert_same_fit(_fit("aae", True, mk, one), _fit("aae", False, mk, one), "reduce None")


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_embedding_bag_condition_with_offsets_equals_its_padded_2d_form(mode):
    """(input, offsets) condition data through AdversarialAutoEncoder.fit against the same bags as a 2-D block padded with a
    padding_idx row (row 12 of a 13-row table; both modules hold the same weights)."""
    from aaerec.condition import EmbeddingBagCondition

    def mk():
        return EmbeddingBagCondition(13, 8, mode=mode, padding_idx=12, device="cuda")

    def ids(authors):
        return [[int(a[1:]) for a in row] for row in authors]

    def offsets_form(cond, authors):
        idx, offsets, _ = RC.flat(ids(authors))
        return (idx, offsets)

    def padded_form(cond, authors):
        return RC.padded(ids(authors), 12)

    a, b = _fit("aae", True, mk, offsets_form), _fit("aae", False, mk, padded_form)
    assert isinstance(a[3], tuple) and a[0]._is_device_native()
    _assert_same_fit(a, b, mode)


def test_checkpoint_in_the_middle_of_a_resident_fit(tmp_path):
    """An unbroken resident fit of two epochs (six steps) against one that, after its second step, is overwritten with the
    first run's checkpoint of that moment (parameters, Adam state, table, the condition's optimizer.state_dict(), both host
    generators) and goes on: test_cond_bag_gpu.py's checkpoint tolerances."""
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec.condition import CategoricalCondition, ConditionList
    X, authors = _corpus()

    def run(seed, load=None):
        torch.manual_seed(seed)
        np.random.seed(7)
        cond = CategoricalCondition(8, reduce="sum", sparse=True)
        data = cond.fit_transform(authors)
        m = AdversarialAutoEncoder(n_hidden=HIDDEN, n_code=10, n_epochs=2, batch_size=BATCH, verbose=False, rng_mode="reference",
                                   conditions=ConditionList([("author", cond)]))
        m.resident_conditions = True
        for step in m.fit_steps(X, condition_data=[data]):
            if step != 2:
                continue
            if load is None:
                torch.save({"params": m.hip.state_dict(), "adam": {w: m.hip.adam_state(w) for w in ("enc", "dec", "gen", "disc")},
                            "table": cond.embedding.state_dict(), "optim": cond.optimizer.state_dict(),
                            "torch_rng": torch.get_rng_state(), "np_rng": np.random.get_state()}, tmp_path / "ck.pt")
            else:
                ck = torch.load(load, weights_only=False)
                m.hip.load_params(ck["params"])
                for w, st in ck["adam"].items():
                    m.hip.load_adam_state(w, st)
                cond.embedding.load_state_dict(ck["table"])
                cond.optimizer.load_state_dict(ck["optim"])
                torch.set_rng_state(ck["torch_rng"])
                np.random.set_state(ck["np_rng"])
        return m, cond

    (ma, ca), (mb, cb) = run(1), run(2, load=tmp_path / "ck.pt")
    a, b = ma.hip.state_dict(), mb.hip.state_dict()
    for k in a:
        np.testing.assert_allclose(b[k], a[k], atol=1e-7, rtol=0, err_msg=k)
    (ta, sa, ma_, va), (tb, sb, mb_, vb) = _table_state(ca), _table_state(cb)
    assert sa == sb == 6.0
    np.testing.assert_allclose(tb, ta, atol=1e-7, rtol=0)
    np.testing.assert_allclose(mb_, ma_, atol=1e-9, rtol=1e-6)
    np.testing.assert_allclose(vb, va, atol=1e-13, rtol=1e-6)


def test_no_upload_for_the_condition_inside_the_epoch_loop(monkeypatch):
    """During a resident fit _hip.upload moves nothing from the host between the first and the last step: the lists went up
    once, before the epoch loop.  (rng_mode='device': the reference mode uploads its host-drawn masks by design.)  On the padded route
    the same spy sees the index block of every step."""
    from aaerec import _hip
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec.condition import CategoricalCondition, ConditionList
    X, authors = _corpus()
    real = _hip.upload
    for resident in (True, False):
        calls, in_loop = [], []
        cond = CategoricalCondition(8, reduce="sum", sparse=True)
        data = cond.fit_transform(authors)
        m = AdversarialAutoEncoder(n_hidden=HIDDEN, n_code=10, n_epochs=2, batch_size=BATCH, verbose=False, seed=3,
                                   conditions=ConditionList([("author", cond)]))
        m.resident_conditions = resident

        def spy(x, device, dtype=None):
            if not (torch.is_tensor(x) and x.is_cuda):          # (a device tensor passes through upload: nothing crosses)
                calls.append(1)
            return real(x, device, dtype)
        monkeypatch.setattr(_hip, "upload", spy)
        steps = 0
        for step in m.fit_steps(X, condition_data=[data]):
            if step == 1:
                del calls[:]                 # (everything up to the first step's launches: the corpus, the lists)
            steps, in_loop = step, list(calls)
        monkeypatch.setattr(_hip, "upload", real)
        assert steps == 6
        assert len(in_loop) == (0 if resident else 5), (resident, len(in_loop))
