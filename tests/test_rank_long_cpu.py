"""What the long-list ranking path (k up to 1024: csrc/rank_long.h) needs no device for: its entry in the options table, and
the evaluation harness handing metrics bounded beyond 32 to predict_topk."""
import numpy as np
import scipy.sparse as sp


def test_rank_collect_cap_is_an_option_and_refuses_nonsense():
    from aaerec import _hip
    import pytest
    lib = _hip.load_library()
    assert lib.aae_set_option(b"RANK_COLLECT_CAP", b"8") == 0
    assert lib.aae_set_option(b"RANK_COLLECT_CAP", b"4096") == 0
    for bad in (b"0", b"-3", b"4097", b"many", b"12x", b""):
        assert lib.aae_set_option(b"RANK_COLLECT_CAP", bad) == -1, bad
        assert b"RANK_COLLECT_CAP" in lib.aae_last_error()
    assert lib.aae_set_option(b"RANK_COLLECT_CAP", None) == 0
    _hip.set_option("RANK_COLLECT_CAP", 16)
    _hip.set_option("RANK_COLLECT_CAP", None)
    with pytest.raises(_hip.AaeHipError):
        _hip.set_option("RANK_COLLECT_CAP", "none")
    assert _hip.RANK_K_MAX == 1024


class _StandIn:
    """A recommender that ranks a fixed score matrix: predict_topk as the device path answers (min-max scaled scores, known
    items dropped, k best, smaller id at ties), predict the dense matrix."""

    def __init__(self, scores, x_test):
        self.scores, self.x_test, self.asked = scores, x_test, []

    def train(self, train_set):
        pass

    def predict(self, test_set):
        return self.scores

    def predict_topk(self, test_set, k=10):
        self.asked.append(k)
        from aaerec.evaluation import remove_non_missing
        y = remove_non_missing(self.scores, self.x_test, copy=True)
        ids = np.stack([np.lexsort((np.arange(y.shape[1]), -row))[:k] for row in y])
        return ids, np.take_along_axis(y, ids, axis=1)


class _Set:
    def clone(self):
        return self


def test_evaluation_hands_metrics_bounded_beyond_32_to_predict_topk(monkeypatch, tmp_path):
    """A metric bounded at 100 (the package's tables stay the reference's: the entry exists for this test only) takes the
    predict_topk route, and its results equal evaluate() on the dense matrix."""
    from aaerec import evaluation as E
    monkeypatch.setitem(E.BOUNDED_METRICS, "map@100", E.MAP(100))
    monkeypatch.setitem(E.METRICS, "map@100", E.BOUNDED_METRICS["map@100"])
    r = np.random.default_rng(0)
    n, N = 40, 700
    scores = r.random((n, N)).astype(np.float32)
    x = sp.random(n, N, density=0.02, format="csr", random_state=1)
    x.data[:] = 1
    y = sp.random(n, N, density=0.01, format="csr", random_state=2)
    y.data[:] = 1
    y = y - y.multiply(x)
    y = sp.csr_matrix(y)
    y.eliminate_zeros()
    metrics = ["map@100", "mrr@10", "p@5"]
    ev = E.Evaluation(None, None, metrics=metrics, logfile=str(tmp_path / "log.txt"))
    ev.train_set = ev.test_set = _Set()
    ev.x_test, ev.y_test = x, y
    assert ev._bounded_k() == 100
    rec = _StandIn(scores, x)
    got = ev([rec])[0]
    assert rec.asked == [100]
    dense = E.evaluate(y, E.remove_non_missing(scores, x, copy=True), metrics=metrics)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(dense, dtype=np.float64), rtol=1e-12, atol=1e-12)
    monkeypatch.setitem(E.BOUNDED_METRICS, "map@2000", E.MAP(2000))      # beyond the library's limit: the dense route
    ev2 = E.Evaluation(None, None, metrics=["map@2000"], logfile=str(tmp_path / "log.txt"))
    assert ev2._bounded_k() is None
