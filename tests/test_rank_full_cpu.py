"""What the full-ranking path (csrc/rank_full.h: the rank of every held-out item, for 'mrr' / 'map') needs no device for:
evaluate_ranks against evaluate() on dense matrices, the evaluation harness handing unbounded metrics to predict_ranks, and
the library's / the custom ops' surface."""
import numpy as np
import pytest
import scipy.sparse as sp


def _ranks_of(y_scaled, truth):
    """CSR with truth's pattern: 1 + the number of items of the row that score higher (remove_non_missing's output: the
    known items sit at 0).  Asserts that no other item of the row ties with a held-out one - the ranks are then what ANY
    sort of the row gives."""
    T = sp.csr_matrix(truth)
    T.sort_indices()
    data = np.zeros(T.nnz, dtype=np.int32)
    for b in range(T.shape[0]):
        for e in range(T.indptr[b], T.indptr[b + 1]):
            t = T.indices[e]
            assert np.count_nonzero(y_scaled[b] == y_scaled[b, t]) == 1, "a held-out item's score ties with another item's"
            data[e] = 1 + np.count_nonzero(y_scaled[b] > y_scaled[b, t])
    return sp.csr_matrix((data, T.indices.copy(), T.indptr.copy()), shape=T.shape)


def _case(seed, n=60, N=400):
    """float64 scores without ties; known items x; truth rows with 0, 1 and many held-out items (none of them known, none
    the row's minimum: those sit at 0 with the known items after remove_non_missing)."""
    r = np.random.default_rng(seed)
    scores = r.random((n, N))
    assert all(np.unique(row).size == N for row in scores)
    x = sp.random(n, N, density=0.03, format="csr", random_state=seed + 1)
    x.data[:] = 1
    xd = x.toarray() > 0
    lens = np.concatenate([[0, 0, 1, 1, 1, 40], r.integers(0, 12, size=n - 6)])
    y = sp.lil_matrix((n, N))
    for b in range(n):
        free = np.flatnonzero(~xd[b] & (np.arange(N) != scores[b].argmin()))
        for t in r.choice(free, size=int(lens[b]), replace=False):
            y[b, t] = 1
    y = y.tocsr()
    assert {0, 1, 40} <= set(np.diff(y.indptr).tolist())
    return scores, x, y


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_evaluate_ranks_equals_evaluate_on_dense_matrices(seed):
    from aaerec import evaluation as E
    scores, x, y = _case(seed)
    scaled = E.remove_non_missing(scores, x, copy=True)
    ranks = _ranks_of(scaled, y)
    names = list(E.METRICS)
    assert len(names) == 12 and "mrr" in names and "map" in names and "P@1" in names
    want = E.evaluate(y, scaled, metrics=names)
    got = E.evaluate_ranks(ranks, names)
    for name, g, w in zip(names, got, want):
        np.testing.assert_allclose(np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64), rtol=0, atol=1e-12, err_msg=name)
    # the batched form of evaluate (per-row values, then mean / std) agrees as well
    want_b = E.evaluate(y, scaled, metrics=names, batch_size=7)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want_b, dtype=np.float64), rtol=0, atol=1e-12)


def test_evaluate_ranks_on_the_known_answer_vectors():
    """The relevance vectors of rank_metrics_with_std's doctests, as ranks."""
    from aaerec import evaluation as E

    def ranks(rs):
        return sp.csr_matrix(np.asarray([[j + 1 if v else 0 for j, v in enumerate(r)] for r in rs], dtype=np.int32))

    mrr = E.evaluate_ranks(ranks([[0, 0, 1], [0, 1, 0], [1, 0, 0]]), ["mrr"])[0]
    assert round(mrr[0], 4) == 0.6111
    assert E.evaluate_ranks(ranks([[0, 0, 0], [0, 1, 0], [1, 0, 0]]), ["mrr"])[0][0] == 0.5
    ap = E.evaluate_ranks(ranks([[1, 1, 0, 1, 0, 1, 0, 0, 0, 1]]), ["map"])[0]
    assert round(ap[0], 4) == 0.7833 and ap[1] == 0.0
    # bounded: the same vector cut at 5 -> hits at 1, 2, 4: AP = (1 + 1 + 3/4) / 3, P@5 = 3/5, RR = 1
    got = E.evaluate_ranks(ranks([[1, 1, 0, 1, 0, 1, 0, 0, 0, 1]]), ["map@5", "p@5", "mrr@5", "P@1"])
    np.testing.assert_allclose([g[0] for g in got], [(1 + 1 + 0.75) / 3, 0.6, 1.0, 1.0], atol=1e-15)
    # a row without held-out items, and one whose only item lies beyond k
    got = E.evaluate_ranks(ranks([[0] * 30, [0] * 29 + [1]]), ["mrr", "map", "mrr@10", "map@10", "p@10"])
    np.testing.assert_allclose([g[0] for g in got], [0.5 / 30, 0.5 / 30, 0.0, 0.0, 0.0], atol=1e-15)


@pytest.mark.parametrize("case,N,h,c,rows,excl", [(0, 5000, 200, 50, 64, True), (5, 2000, 61, 20, 100, False), (21, 5000, 200, 50, 113, True)])
def test_oracle_intervals_are_narrow_for_the_chosen_truths(case, N, h, c, rows, excl):
    """tests/test_rank_full_gpu.py bounds every device rank by the interval a tolerance of 2e-6 on the scaled scores leaves
    open, and asks that at most 10 % of the intervals be wider than one rank on its fp32 cases with N <= 5000.  Here the same
    share on the ORACLE's predict for those cases' parameters (tools/synth.init_params, dec.lin3 scaled by 8, untrained; the
    condition of case 5 left out) and held-out items drawn as that file draws them: it must stay within the 10 % as well."""
    from oracle import aae_oracle as O
    from tools.synth import init_params
    from test_rank_full_gpu import _corpus, _intervals, _truths
    params = init_params(N, h, c, cond_inc=0, seed=case)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * 8.0
    ora = O.OracleAAE(params, dropout=(0.2, 0.2), gen_lr=1e-3, reg_lr=1e-3, activation="ReLU")
    ip, idx, val, docs = _corpus(np.random.default_rng(100 + case), N, rows, 30)
    full = np.asarray(ora.predict(ip, idx, val), dtype=np.float32)
    one, mixed = _truths(np.random.default_rng(700 + case), N, docs)
    for name, tr in (("one per row", one), ("mixed", mixed)):
        lo, hi, known = _intervals(full, docs, tr, excl, 2e-6)
        wide = float(np.mean(hi[~known] > lo[~known]))
        print(f"oracle, case {case}, {name}: wide intervals {100 * wide:.2f} % of {int((~known).sum())}")
        assert wide <= 0.10, (name, wide)


class _StandIn:
    """A recommender that ranks a fixed score matrix (tests/test_rank_long_cpu.py::_StandIn) and offers predict_ranks as
    the device path answers it: known items not rankable, better score first."""

    def __init__(self, scores, x_test):
        self.scores, self.x_test, self.asked = scores, x_test, []

    def train(self, train_set):
        pass

    def predict(self, test_set):
        self.asked.append("predict")
        return self.scores

    def predict_topk(self, test_set, k=10):
        self.asked.append(("predict_topk", k))
        from aaerec.evaluation import remove_non_missing
        y = remove_non_missing(self.scores, self.x_test, copy=True)
        ids = np.stack([np.lexsort((np.arange(y.shape[1]), -row))[:k] for row in y])
        return ids, np.take_along_axis(y, ids, axis=1)

    def predict_ranks(self, test_set, y_true):
        self.asked.append("predict_ranks")
        from aaerec.evaluation import remove_non_missing
        return _ranks_of(remove_non_missing(self.scores, self.x_test, copy=True), y_true)


class _Set:
    index2token = ["a", "b"]         # (what a prediction dump writes as vocab.txt)

    def clone(self):
        return self


def _evaluation(E, metrics, x, y, log, **kw):
    ev = E.Evaluation(None, None, metrics=metrics, logfile=log, **kw)
    ev.train_set = ev.test_set = _Set()
    ev.x_test, ev.y_test = x, y
    return ev


def test_evaluation_hands_unbounded_metrics_to_predict_ranks(tmp_path):
    from aaerec import evaluation as E
    scores, x, y = _case(5)
    metrics = ["mrr", "map", "mrr@10"]
    log = str(tmp_path / "log.txt")
    dense = E.evaluate(y, E.remove_non_missing(scores, x, copy=True), metrics=metrics)
    ev = _evaluation(E, metrics, x, y, log)
    assert ev._bounded_k() is None
    rec = _StandIn(scores, x)
    got = ev([rec])[0]
    assert rec.asked == ["predict_ranks"]
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(dense, dtype=np.float64), rtol=0, atol=1e-12)
    # topk=False and a prediction dump keep the dense route
    rec = _StandIn(scores, x)
    got = _evaluation(E, metrics, x, y, log, topk=False)([rec])[0]
    assert rec.asked == ["predict"]
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(dense, dtype=np.float64), rtol=0, atol=1e-12)
    rec = _StandIn(scores, x)
    _evaluation(E, metrics, x, y, log, logdir=str(tmp_path / "dump"))([rec])
    assert rec.asked == ["predict"]
    # all-bounded metrics stay on predict_topk; a metric object (not a name) stays dense
    rec = _StandIn(scores, x)
    _evaluation(E, ["mrr@10", "p@5"], x, y, log)([rec])
    assert rec.asked == [("predict_topk", 10)]
    rec = _StandIn(scores, x)
    _evaluation(E, ["mrr", E.MAP(7)], x, y, log)([rec])
    assert rec.asked == ["predict"]


def test_library_exports_the_rank_calls_and_the_op_is_registered():
    import torch
    from aaerec import _hip, ops  # noqa: F401
    lib = _hip.load_library()
    for name in ("aae_predict_ranks", "aae_decode_ranks", "aae_rank_full_max_rows"):
        assert getattr(lib, name) is not None, name
    assert lib.aae_abi_version() == 4
    assert hasattr(torch.ops.aaerec, "predict_ranks")
    schema = str(torch.ops.aaerec.predict_ranks.default._schema)
    assert "truth_indptr" in schema and "exclude_known" in schema
    from aaerec.aae import AdversarialAutoEncoder, AutoEncoder, AAERecommender
    from aaerec.dae import DenoisingAutoEncoder
    for cls in (AdversarialAutoEncoder, AutoEncoder, DenoisingAutoEncoder, AAERecommender, _hip.HipAAE):
        assert callable(getattr(cls, "predict_ranks")), cls
    assert callable(_hip.HipAAE.decode_ranks)
