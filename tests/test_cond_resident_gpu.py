"""resident_conditions = True for constant condition blocks and for DecodingRecommender: the condition data is uploaded once
per fit() / ranking call, a step's rows reach the condition block by one aae_cond_gather launch, and - a gather is a copy - every
result equals the default route's bit for bit.  Sizes: 64 items, 40 documents, batches of 16 (the last one has 8 rows), hidden
16, code 8, constant blocks of 5 and 12 columns."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from golden_util import Fixture

pytestmark = pytest.mark.gpu
N_ITEMS, N_DOCS, BATCH, HIDDEN, CODE = 64, 40, 16, 16, 8


def _data():
    rng = np.random.default_rng(17)
    X = sp.csr_matrix((rng.random((N_DOCS, N_ITEMS)) < 0.12).astype(np.float32))
    Y = sp.csr_matrix(((rng.random((N_DOCS, N_ITEMS)) < 0.08) & (X.toarray() == 0)).astype(np.float32))
    a = rng.standard_normal((N_DOCS, 5)).astype(np.float32)
    b = rng.standard_normal((N_DOCS, 12))                              # float64, as a host vectoriser may hand it over
    cats = [["a%d" % v for v in rng.integers(0, 9, size=rng.integers(1, 5))] for _ in range(N_DOCS)]
    return X, Y, a, b, cats


X, Y, BLOCK_A, BLOCK_B, CATS = _data()


class _Vect:
    """A vectoriser whose documents already are their vectors: PretrainedWordEmbeddingCondition's own transform / encode /
    resident run on them."""

    def __init__(self, width):
        self.embedding = np.zeros((1, width), dtype=np.float32)

    def fit(self, raw):
        return self

    def transform(self, raw):
        return np.asarray(raw)

    def fit_transform(self, raw):
        return np.asarray(raw)


def _conditions(kind):
    """(ConditionList, raw condition data): 'const' = [constant block]; 'mixed' = [constant, CategoricalCondition(8, sum),
    constant]; 'two' = two constant blocks."""
    from aaerec import condition as C
    const = lambda w: C.PretrainedWordEmbeddingCondition(_Vect(w), use_cuda=True)            # noqa: E731
    if kind == "const":
        return C.ConditionList([("a", const(5))]), [BLOCK_A]
    if kind == "two":
        return C.ConditionList([("a", const(5)), ("b", const(12))]), [BLOCK_A, BLOCK_B]
    cat = C.CategoricalCondition(8, use_cuda=True, reduce="sum", lr=0.01)
    return C.ConditionList([("a", const(5)), ("cat", cat), ("b", const(12))]), [BLOCK_A, CATS, BLOCK_B]


def _model(name, conds):
    from aaerec.aae import AdversarialAutoEncoder, AutoEncoder
    from aaerec.dae import DenoisingAutoEncoder
    from aaerec.vae import VAE
    kw = dict(n_hidden=HIDDEN, n_code=CODE, n_epochs=2, batch_size=BATCH, conditions=conds, verbose=False, seed=3)
    if name == "AdversarialAutoEncoder":
        return AdversarialAutoEncoder(**kw)
    if name == "AutoEncoder":
        return AutoEncoder(**kw)
    if name == "DenoisingAutoEncoder":
        return DenoisingAutoEncoder(corrupt_draws="step", **kw)
    return VAE(N_ITEMS, N_ITEMS, **kw)


class _Uploads:
    """_hip.upload wrapped by a counter of the float matrices that cross from the host."""

    def __init__(self, monkeypatch):
        from aaerec import _hip
        self.shapes, real = [], _hip.upload

        def counting(x, device, dtype=None):
            t = x if torch.is_tensor(x) else np.asarray(x)
            on_device = torch.is_tensor(x) and x.is_cuda
            floating = t.is_floating_point() if torch.is_tensor(t) else t.dtype.kind == "f"
            if not on_device and floating and t.ndim == 2:
                self.shapes.append(tuple(t.shape))
            return real(x, device, dtype)
        monkeypatch.setattr(_hip, "upload", counting)


def _fit(name, kind, flag, uploads=None):
    """Two epochs of fit() under fixed seeds; every parameter, the trainable table and its optimiser state."""
    np.random.seed(5)
    torch.manual_seed(5)
    conds, raw = _conditions(kind)
    data = conds.fit_transform(raw)
    m = _model(name, conds)
    m.resident_conditions = flag
    if uploads is not None:
        uploads.shapes.clear()
    m.fit(X, condition_data=data)
    state = {k: np.asarray(v) for k, v in m.hip.state_dict().items()}
    if "cat" in conds:
        cat = conds["cat"]
        state["cat.weight"] = cat.embedding.weight.detach().cpu().numpy()
        for k, v in cat.optimizer.state[cat.embedding.weight].items():
            state["cat." + k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return m, data, state


def _same_bits(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{tag}: {k}"


@pytest.mark.parametrize("kind", ["const", "mixed"])
@pytest.mark.parametrize("name", ["AdversarialAutoEncoder", "AutoEncoder", "DenoisingAutoEncoder", "VAE"])
def test_fit_equals_the_unset_flag_bit_for_bit_and_uploads_no_block_inside_the_loop(name, kind, monkeypatch):
    from aaerec import _hip
    from aaerec.aae import resident_condition_data
    uploads = _Uploads(monkeypatch)
    _, _, want = _fit(name, kind, False)
    m, data, got = _fit(name, kind, True, uploads)
    _same_bits(got, want, f"{name} {kind}")
    assert len(want) >= 8 and any(np.any(v != 0) for v in want.values())
    # the route is really taken: under the flag a float matrix crosses the host once per constant block - the whole corpus,
    # at the head of fit() - and never a batch's rows inside the step loop
    n_const = 1 if kind == "const" else 2
    assert sorted(uploads.shapes) == sorted([(N_DOCS, 5), (N_DOCS, 12)][:n_const]), uploads.shapes
    res = resident_condition_data(m, data)
    for cond, c in zip(m.conditions.values(), res):
        assert isinstance(c, _hip.DeviceBlock if getattr(cond, "constant_concat", False) else _hip.DeviceBags)
    assert [c.width for c in res if isinstance(c, _hip.DeviceBlock)] == [5, 12][:n_const]
    m.resident_conditions = False
    assert all(a is b for a, b in zip(resident_condition_data(m, data), data))


def _forward(m, data):
    """predict, predict_topk, predict_ranks and eval_loss of a trained model, each from the same torch seed (the VAE in
    rng_mode='reference' draws its eps from it)."""
    out = {}
    for name, call in (("predict", lambda: m.predict(X, condition_data=data)),
                       ("topk", lambda: m.predict_topk(X, k=7, condition_data=data)),
                       ("ranks", lambda: m.predict_ranks(X, Y, condition_data=data)),
                       ("loss", lambda: m.eval_loss(X, condition_data=data, per_row=True))):
        torch.manual_seed(11)
        r = call()
        if sp.issparse(r):
            r = (r.indptr, r.indices, r.data)
        for i, part in enumerate(r if isinstance(r, tuple) else (r,)):
            out[f"{name}.{i}"] = np.asarray(part)
    return out


@pytest.mark.parametrize("kind", ["two", "mixed"])
@pytest.mark.parametrize("name", ["AdversarialAutoEncoder", "VAE"])
def test_forward_calls_agree_exactly_with_the_default_route(name, kind, monkeypatch):
    from aaerec.vae import VAE
    np.random.seed(5)
    torch.manual_seed(5)
    conds, raw = _conditions(kind)
    data = conds.fit_transform(raw)
    if name == "VAE":
        m = VAE(N_ITEMS, N_ITEMS, n_hidden=HIDDEN, n_code=CODE, n_epochs=1, batch_size=BATCH, conditions=conds, verbose=False,
                rng_mode="reference")
    else:
        m = _model(name, conds)
    m.fit(X, condition_data=data)
    m.batch_size = 12                                  # ragged chunks: 12, 12, 12, 4 rows
    want = _forward(m, data)
    uploads = _Uploads(monkeypatch)
    m.resident_conditions = True
    got = _forward(m, data)
    _same_bits(got, want, f"{name} {kind}")
    assert want["predict.0"].shape == (N_DOCS, N_ITEMS) and want["topk.0"].shape == (N_DOCS, 7)
    # four calls, each uploads every constant block once, whole
    assert sorted(s for s in uploads.shapes if s[1] in (5, 12)) == sorted([(N_DOCS, 5), (N_DOCS, 12)] * 4), uploads.shapes


# ---- keep_on_device through AAERecommender.train -----------------------------------------------------------------------------
class _Set:
    def __init__(self, M, attrs):
        self.M, self.attrs = M, attrs

    def tocsr(self):
        return self.M

    def size(self, dim=0):
        return self.M.shape[dim]

    def get_attributes(self, keys):
        return [self.attrs for _ in keys]


WORDS = ["graph", "neural", "network", "matrix", "sparse", "kernel", "ranking", "citation", "music", "playlist"]


def _titles():
    rng = np.random.default_rng(23)
    return [" ".join(rng.choice(WORDS, size=rng.integers(1, 6))) for _ in range(N_DOCS)]


def test_keep_on_device_through_recommender_train(monkeypatch):
    from aaerec import _hip, condition as C
    from aaerec.aae import AAERecommender, AdversarialAutoEncoder, resident_condition_data
    from aaerec.ub import EmbeddedVectorizer
    emb = np.random.default_rng(29).standard_normal((len(WORDS), 6)).astype(np.float32)
    titles = _titles()
    vect = EmbeddedVectorizer(emb, WORDS).fit(titles)
    host, dev = vect.transform(titles), vect.transform_device(titles)
    assert dev.is_cuda and dev.dtype == torch.float32 and dev.shape == (N_DOCS, 6) and host.dtype == np.float32
    assert dev.cpu().numpy().tobytes() == host.tobytes()

    def train(keep, flag):
        np.random.seed(7)
        torch.manual_seed(7)
        monkeypatch.setattr(AdversarialAutoEncoder, "resident_conditions", flag)
        cond = C.PretrainedWordEmbeddingCondition(EmbeddedVectorizer(emb, WORDS), use_cuda=True, keep_on_device=keep)
        rec = AAERecommender(conditions=C.ConditionList([("title", cond)]), n_hidden=HIDDEN, n_code=CODE, n_epochs=2,
                             batch_size=BATCH, verbose=False, seed=3)
        rec.train(_Set(X, titles))
        data = rec.conditions.transform([titles])
        res = resident_condition_data(rec.model, data)[0]
        return {k: np.asarray(v) for k, v in rec.model.hip.state_dict().items()}, data[0], res, rec

    want, data, res, _ = train(False, False)
    assert isinstance(data, np.ndarray) and res is data
    got, data, res, _ = train(False, True)
    _same_bits(got, want, "host-fed, resident")
    assert isinstance(res, _hip.DeviceBlock)
    got, data, res, rec = train(True, True)
    _same_bits(got, want, "keep_on_device, resident")
    # the tensor of the product itself is the resident block: wrapped, not copied
    assert torch.is_tensor(data) and data.is_cuda and isinstance(res, _hip.DeviceBlock) and res.data.data_ptr() == data.data_ptr()
    np.testing.assert_array_equal(rec.predict(_Set(X, titles)), rec.model.predict(X, condition_data=[host]))


# ---- DecodingRecommender -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["step_decoding", "step_decoding_trainable"])
def test_decoding_recommender_native_route_tracks_reference(name):
    """test_host_gpu.py::test_decoding_recommender_tracks_reference's replay of the reference fixtures, through the kernels'
    route: resident_conditions = True, constant_concat = True blocks, the trainable table on the GPU (encode_into /
    update_from instead of autograd).  Tolerances: that test's - losses rtol 1e-5 / atol 1e-6, parameters and embedding
    atol 1e-5."""
    from aaerec.aae import DecodingRecommender
    from aaerec import condition as C
    fx = Fixture(name)
    cfg = fx.cfg
    incs = cfg["incs"]

    def const_concat(inc):
        class ConstConcat(C.ConcatenationBasedConditioning):
            constant_concat = True

            def size_increment(self):
                return inc

            def encode(self, inputs):
                return torch.as_tensor(np.asarray(inputs), dtype=torch.float32, device="cuda")
        return ConstConcat()
    items, cat = [], None
    if cfg["trainable"]:
        cat = C.CategoricalCondition(incs[0], sparse=False, use_cuda=True, reduce="sum", lr=1e-2)
        V = fx.z["init.cond.embedding"].shape[0]
        cat.vocab = {"a%d" % i: i for i in range(1, V)}           # indices are given pre-transformed
        cat.embedding = torch.nn.Embedding(V, incs[0], padding_idx=0)
        with torch.no_grad():
            cat.embedding.weight.copy_(torch.from_numpy(fx.z["init.cond.embedding"]))
        cat.embedding = cat.embedding.cuda()
        cat.optimizer = torch.optim.Adam(cat.embedding.parameters(), lr=1e-2)
        items.append(("authors", cat))
    else:
        items.append(("title", const_concat(incs[0])))
    items += [(f"c{j}", const_concat(inc)) for j, inc in enumerate(incs[1:])]
    conds = C.ConditionList(items)
    m = DecodingRecommender(conds, n_epochs=1, batch_size=cfg["B"], n_hidden=cfg["h"], lr=cfg["gen_lr"], verbose=True,
                            rng_mode="reference", dropout=tuple(cfg["dropout"]))
    m.resident_conditions = True
    m._build(cfg["N"])
    m.hip.load_params(fx.init_params())
    assert m._native_route()

    def cin_of(prefix, s=0):
        cin = fx.cond_inputs(s, prefix=prefix)
        if cfg["trainable"]:
            cin[0] = [[int(j) for j in row if j != 0] or [0] for row in cin[0]]
        return cin
    for s in range(fx.steps):
        ip, idx, val = fx.batch(s)
        Yb = sp.csr_matrix((val, idx, ip), shape=(len(ip) - 1, cfg["N"]))
        masks = [torch.from_numpy(k) for k in fx.masks(s)]
        m._masks = lambda B, masks=masks: masks                  # the fixture's randomness instead of a fresh draw
        m.partial_fit(cin_of(None, s), torch.FloatTensor(Yb.toarray()), step=s)
        np.testing.assert_allclose(m.last_loss, fx.z[f"step{s}.losses"][0], rtol=1e-5, atol=1e-6)
        got = m.mlp.state_dict()
        for k in ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"):
            np.testing.assert_allclose(got[k].numpy(), fx.z[f"step{s}.dec.{k}"], atol=1e-5, rtol=0,
                                       err_msg=f"{name} step {s} {k}")
        if cat is not None:
            np.testing.assert_allclose(cat.embedding.weight.detach().cpu().numpy(), fx.z[f"step{s}.cond.embedding"],
                                       atol=1e-5)
            st = cat.optimizer.state[cat.embedding.weight]       # torch's own layout, as on the AAE
            assert float(st["step"]) == s + 1 and st["exp_avg"].shape == cat.embedding.weight.shape
    m.batch_size = 7                                             # ragged predict batches
    out = m._predict_conditions(cin_of("predict"), cfg["B"])
    np.testing.assert_allclose(out, fx.z["predict.out"], atol=1e-5)


def _decoding(kind, flag, uploads=None, plain=False):
    from aaerec import condition as C
    from aaerec.aae import DecodingRecommender
    np.random.seed(5)
    torch.manual_seed(5)
    conds, raw = _conditions(kind)
    if plain:
        # a concatenating condition the kernels do not know: no constant_concat, no device_native
        class Plain(C.ConcatenationBasedConditioning):
            def size_increment(self):
                return 12

            def encode(self, inputs):
                return torch.as_tensor(np.asarray(inputs), dtype=torch.float32, device="cuda")
        conds = C.ConditionList([("a", conds["a"]), ("b", Plain())])
    data = conds.fit_transform(raw)
    m = DecodingRecommender(conds, n_epochs=2, batch_size=BATCH, n_hidden=HIDDEN, verbose=False, seed=3)
    m.resident_conditions = flag
    if uploads is not None:
        uploads.shapes.clear()
    m.fit(data, X)
    return m, raw, {k: v.numpy() for k, v in m.mlp.state_dict().items()}


def test_decoding_recommender_fit_over_resident_constant_blocks_equals_the_default_route(monkeypatch):
    uploads = _Uploads(monkeypatch)
    _, _, want = _decoding("two", False)
    m, raw, got = _decoding("two", True, uploads)
    _same_bits(got, want, "DecodingRecommender fit")
    assert m._native_route() and sorted(uploads.shapes) == [(N_DOCS, 5), (N_DOCS, 12)], uploads.shapes
    # the forward calls: exact agreement with the default route, on ragged chunks
    m.batch_size = 12
    test_set = _Set(X, None)
    test_set.get_attributes = lambda keys: list(raw)
    calls = (("predict", lambda: m.predict(test_set)), ("topk", lambda: m.predict_topk(test_set, k=7)),
             ("ranks", lambda: m.predict_ranks(test_set, Y)), ("loss", lambda: m.eval_loss(test_set, per_row=True)))

    def forward():
        out = {}
        for name, call in calls:
            r = call()
            if sp.issparse(r):
                r = (r.indptr, r.indices, r.data)
            for i, part in enumerate(r if isinstance(r, tuple) else (r,)):
                out[f"{name}.{i}"] = np.asarray(part)
        return out
    under_flag = forward()
    m.resident_conditions = False
    _same_bits(under_flag, forward(), "DecodingRecommender forward calls")
    assert under_flag["predict.0"].shape == (N_DOCS, N_ITEMS)


def test_decoding_recommender_trains_a_resident_table_without_uploads_in_the_loop(monkeypatch):
    """[constant, CategoricalCondition(8, sum), constant] under the flag: the value lists and both blocks are resident, the table
    learns through update_from (its optimiser state is torch's own), and nothing but the two whole blocks is uploaded."""
    from aaerec import condition as C
    uploads = _Uploads(monkeypatch)
    np.random.seed(5)
    torch.manual_seed(5)
    conds, raw = _conditions("mixed")
    conds.fit_transform(raw)
    before = conds["cat"].embedding.weight.detach().cpu().numpy().copy()
    m, _, got = _decoding("mixed", True, uploads)
    cat = m.conditions["cat"]
    assert isinstance(cat, C.CategoricalCondition) and m._native_route()
    assert sorted(uploads.shapes) == [(N_DOCS, 5), (N_DOCS, 12)], uploads.shapes
    after = cat.embedding.weight.detach().cpu().numpy()
    assert after.shape == before.shape and np.isfinite(after).all() and np.array_equal(after[0], before[0])
    assert (after[1:] != before[1:]).any()
    steps = 2 * -(-N_DOCS // BATCH)
    assert int(cat.optimizer.state[cat.embedding.weight]["step"]) == steps
    assert all(np.isfinite(v).all() for v in got.values())


def test_decoding_recommender_keeps_the_parents_route_for_a_list_that_is_not_device_native():
    _, _, want = _decoding("two", False, plain=True)
    m, _, got = _decoding("two", True, plain=True)
    assert not m._native_route()
    _same_bits(got, want, "DecodingRecommender, a condition that is not device-native")
