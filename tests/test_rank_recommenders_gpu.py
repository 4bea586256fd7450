"""Evaluation ranks the VAE, DAE and decoder-only recommenders on the device: with bounded metrics it takes their
predict_topk, with mrr / map their predict_ranks (it discovers both by hasattr), and the numbers are those of the reference's
dense pipeline on the recommender's own predict() - remove_non_missing, then the project's tie rule imposed on the dense
scores (an id tie-breaker far below the near-tie bound; known items pushed below everything, among themselves by id).
Rows where another item's scaled score lies within 2e-6 of a held-out item's are left out (the two paths' summation orders
may order such a pair either way); they are counted and may be 2 % of the rows at most."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

NEAR_TIE, NEAR_TIE_CAP = 2e-6, 0.02


def _bags():
    from aaerec.datasets import Bags
    rng = np.random.RandomState(0)
    protos = [rng.choice(300, size=8, replace=False) for _ in range(30)]
    data, owners, years, venue = [], [], {}, {}
    for i in range(600):
        k = rng.randint(30)
        data.append(["i%d" % t for t in rng.choice(protos[k], size=rng.randint(4, 8), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // 600
        venue["d%d" % i] = k
    return Bags(data, owners, {"year": years, "venue": venue})


def _vec_condition():
    """The condition the DecodingRecommender's own tests use (tests/test_host_gpu.py::test_decoding_recommender_learns_from_
    conditions): a constant concatenated vector per document - here the one-hot of its 'venue' attribute."""
    from aaerec import condition as C

    class Vec(C.ConcatenationBasedConditioning):
        def fit(self, raw):
            return self

        def transform(self, raw):
            return np.eye(30, dtype=np.float32)[np.asarray([int(v) for v in raw])]

        def fit_transform(self, raw):
            return self.transform(raw)

        def size_increment(self):
            return 30

        def encode(self, inputs):
            return torch.as_tensor(np.asarray(inputs), dtype=torch.float32, device="cuda")
    return C.ConditionList([("venue", Vec())])


def _make(kind):
    if kind == "vae":       # (rng_mode='reference': predict() and the rank calls draw the same eps from the same torch seed)
        from aaerec.vae import VAERecommender
        return VAERecommender(n_hidden=40, n_code=16, n_epochs=8, batch_size=50, lr=0.01, verbose=False, rng_mode="reference")
    if kind == "dae":
        from aaerec.dae import DAERecommender
        return DAERecommender(n_hidden=40, n_code=16, n_epochs=8, batch_size=50, lr=0.01, verbose=False, seed=11)
    from aaerec.aae import DecodingRecommender
    return DecodingRecommender(_vec_condition(), n_epochs=8, batch_size=50, n_hidden=40, lr=0.01, verbose=False, seed=11)


def _dense_with_tie_rule(rec, ev):
    """rec.predict -> remove_non_missing (the reference's pipeline) in float64, the project's order imposed: equal scores go
    to the smaller id, known items sit below every rankable one, among themselves by id.  Also: per row, whether another
    rankable item's score lies within NEAR_TIE of a held-out item's."""
    from aaerec.evaluation import remove_non_missing
    torch.manual_seed(77)
    y = np.asarray(rec.predict(ev.test_set.clone()))
    y = remove_non_missing(y, ev.x_test, copy=True).astype(np.float64)
    n, N = y.shape
    known = np.asarray(ev.x_test.todense()) != 0
    near = np.zeros(n, dtype=bool)
    Y = ev.y_test.tocsr()
    for b in range(n):
        for t in Y.indices[Y.indptr[b]:Y.indptr[b + 1]]:
            if known[b, t]:
                continue
            d = np.abs(y[b] - y[b, t])
            d[t] = np.inf
            d[known[b]] = np.inf
            near[b] = near[b] or bool((d <= NEAR_TIE).any())
    tie = np.arange(N, dtype=np.float64) / N * 1e-8
    adj = y - tie[None, :]
    adj[known] = (-1.0 - tie[None, :] * np.ones((n, 1)))[known]
    return adj, near


@pytest.mark.parametrize("kind", ["vae", "dae", "decoder"])
def test_evaluation_ranks_the_recommender_on_the_device(kind):
    from aaerec.evaluation import Evaluation, evaluate, evaluate_topk, evaluate_ranks
    bags = _bags()
    for metrics, method in ((["mrr@10", "map@10", "p@5", "P@1"], "predict_topk"), (["mrr", "map", "mrr@10"], "predict_ranks")):
        np.random.seed(3)
        torch.manual_seed(3)
        ev = Evaluation(bags, 2009, metrics=metrics, logfile=None, topk=True).setup(min_elements=2, drop=1)
        rec = _make(kind)
        calls, dense_calls = [], []
        real, real_predict = getattr(rec, method), rec.predict

        def spy(*a, _real=real, **kw):
            torch.manual_seed(77)            # (the VAE in rng_mode='reference': the eps of the dense run below)
            out = _real(*a, **kw)
            calls.append(out)
            return out

        def spy_predict(*a, **kw):
            dense_calls.append(1)
            return real_predict(*a, **kw)
        setattr(rec, method, spy)
        rec.predict = spy_predict
        res = ev([rec])[0]
        assert len(calls) == 1 and not dense_calls, (kind, method, len(calls), len(dense_calls))
        rec.predict = real_predict
        adj, near = _dense_with_tie_rule(rec, ev)
        share = float(near.mean())
        print(f"{kind} {method}: {len(near)} test rows, {int(near.sum())} left out as near-ties ({share:.2%})")
        assert share <= NEAR_TIE_CAP, share
        keep = np.nonzero(~near)[0]
        y_keep = ev.y_test.tocsr()[keep]
        want = evaluate(y_keep, adj[keep], metrics=metrics)
        if method == "predict_topk":
            top_ids = np.asarray(calls[0][0])
            assert top_ids.shape == (len(near), 10)
            np.testing.assert_allclose(np.asarray(res), np.asarray(evaluate_topk(ev.y_test, top_ids, metrics)), atol=0)
            got = evaluate_topk(y_keep, top_ids[keep], metrics)
        else:
            ranks = calls[0]
            assert sp.issparse(ranks) and ranks.shape == ev.y_test.shape
            np.testing.assert_allclose(np.asarray(res), np.asarray(evaluate_ranks(ranks, metrics)), atol=0)
            got = evaluate_ranks(ranks.tocsr()[keep], metrics)
        print("   device:", np.asarray(got).ravel().tolist(), "\n   dense: ", np.asarray(want).ravel().tolist())
        np.testing.assert_allclose(np.asarray(got), np.asarray(want), atol=1e-12, rtol=0)
        # topk=False keeps the reference's dense pipeline for the same recommender
        ev_dense = Evaluation(bags, 2009, metrics=metrics, logfile=None, topk=False).setup(min_elements=2, drop=1)
        rec2 = _make(kind)
        took = []
        real2 = getattr(rec2, method)
        setattr(rec2, method, lambda *a, **kw: took.append(1) or real2(*a, **kw))
        ev_dense([rec2])
        assert not took


class _NoRows:
    """A test set without rows over n_items items (what AAERecommender reads of one: tocsr())."""

    def __init__(self, n_items):
        self._X = sp.csr_matrix((0, n_items), dtype=np.float32)

    def tocsr(self):
        return self._X


@pytest.mark.parametrize("adversarial", [True, False])
def test_a_test_set_without_rows_gives_empty_lists_and_ranks(adversarial):
    """predict_topk of a test set without rows returns [0, k] arrays, as the other four recommenders do (it used to raise:
    torch.cat of no parts), and predict_ranks the empty CSR."""
    from aaerec.aae import AAERecommender
    train_set = _bags().build_vocab(apply=True)
    rec = AAERecommender(adversarial=adversarial, n_hidden=40, n_code=16, n_epochs=1, batch_size=50, verbose=False, seed=11)
    rec.train(train_set)
    n_items = train_set.size(1)
    ids, val = rec.predict_topk(_NoRows(n_items), k=10)
    assert ids.shape == (0, 10) and ids.dtype == np.int32
    assert val.shape == (0, 10) and val.dtype == np.float32
    ranks = rec.predict_ranks(_NoRows(n_items), sp.csr_matrix((0, n_items)))
    assert sp.issparse(ranks) and ranks.shape == (0, n_items) and ranks.nnz == 0 and ranks.dtype == np.int32
