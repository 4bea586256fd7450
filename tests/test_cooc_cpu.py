"""What the item co-occurrence baseline (aaerec/cooc.py, csrc/cooc.h, csrc/abi_cooc.h) needs no device for: the library's
surface and its argument checks, the exactness guard, predict() and the host route of predict_topk / predict_ranks against the
definition  S = X_test @ (X^T X),  order by (-S, id) with the input row's items removed."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp


class _Rows:
    """The slice of the Bags interface Countbased reads: tocsr()."""

    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()


def _corpus(seed=0, docs=60, N=23, n_test=14):
    r = np.random.default_rng(seed)
    X = sp.lil_matrix((docs, N))
    for d in range(docs):
        for i in r.choice(N - 2, size=int(r.integers(2, 6)), replace=False):      # (the last two items never occur)
            X[d, i] = 1
    T = sp.lil_matrix((n_test, N))
    for d in range(n_test - 2):
        for i in r.choice(N, size=int(r.integers(1, 5)), replace=False):
            T[d, i] = 1
    T[0, 3] = 3                                   # a multiplicity
    T[n_test - 2, N - 1] = 1                      # only an item that never occurred: all scores 0; the last row stays empty
    return sp.csr_matrix(X), sp.csr_matrix(T)


def _definition(X, T, k):
    """ids [n, k] (-1 padded), scaled fp32 scores and the int64 score matrix, from the definition."""
    S = np.asarray((T.astype(np.int64) @ (X.T.astype(np.int64) @ X.astype(np.int64))).toarray(), dtype=np.int64)
    n, N = S.shape
    ids = np.full((n, k), -1, dtype=np.int64)
    val = np.zeros((n, k), dtype=np.float64)
    for r in range(n):
        known = set(T.indices[T.indptr[r]:T.indptr[r + 1]].tolist())
        order = [i for i in sorted(range(N), key=lambda i: (-S[r, i], i)) if i not in known][:k]
        span = S[r].max() - S[r].min()
        ids[r, :len(order)] = order
        val[r, :len(order)] = [(S[r, i] - S[r].min()) / span if span else 0.0 for i in order]
    return ids, val, S


def _ranks_definition(S, T, Y):
    Y = sp.csr_matrix(Y)
    Y.sort_indices()
    N = S.shape[1]
    out = np.zeros(Y.nnz, dtype=np.int64)
    for r in range(Y.shape[0]):
        known = set(T.indices[T.indptr[r]:T.indptr[r + 1]].tolist())
        key = lambda i: (1 if i in known else 0, -S[r, i] if i not in known else 0, i)      # noqa: E731
        order = sorted(range(N), key=key)
        for e in range(Y.indptr[r], Y.indptr[r + 1]):
            out[e] = 1 + order.index(Y.indices[e])
    return out


def test_library_exports_the_cooc_calls_and_the_abi_version_stands():
    from aaerec import _hip
    lib = _hip.load_library()
    for name in ("aae_cooc_scores", "aae_cooc_topk", "aae_cooc_ranks"):
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    assert _hip.COOC_TILE == 16384
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "aaerec_hip.h")) as fh:
        assert "#define AAE_COOC_TILE %d" % _hip.COOC_TILE in fh.read()


def _args(lib, **over):
    """A well-formed aae_cooc_topk / _ranks / _scores call over pointers nothing may dereference, one argument replaced."""
    from aaerec import _hip
    p = 0x1000
    cooc, batch, truth = _hip.AaeCooc(), _hip.AaeBatch(), _hip.AaeBatch()
    cooc.indptr_dev = cooc.indices_dev = cooc.values_dev = p
    cooc.n_rows = 50
    for b in (batch, truth):
        b.indptr_dev = b.indices_dev = b.values_dev = p
        b.n_rows = 4
    a = dict(cooc=cooc, batch=batch, truth=truth, n_items=50, k=10, scratch=p, ld=52, idx=p, val=p, ranks=p)
    a.update(over)
    return a


def _call(lib, which, a):
    ref = lambda s: None if s is None else C.byref(s)      # noqa: E731
    if which == "scores":
        return lib.aae_cooc_scores(ref(a["cooc"]), a["n_items"], ref(a["batch"]), a["scratch"], a["ld"], None)
    if which == "topk":
        return lib.aae_cooc_topk(ref(a["cooc"]), a["n_items"], ref(a["batch"]), a["k"], 1, a["scratch"], a["ld"], a["idx"], a["val"], None)
    return lib.aae_cooc_ranks(ref(a["cooc"]), a["n_items"], ref(a["batch"]), ref(a["truth"]), 1, a["scratch"], a["ld"], a["ranks"], None)


def _null_field(kind, field):
    def make(lib):
        a = _args(lib)
        setattr(a[kind], field, None)
        return a
    return make


_BAD = [
    ("scores", lambda lib: _args(lib, cooc=None)),
    ("scores", _null_field("cooc", "indptr_dev")),
    ("topk", _null_field("cooc", "indices_dev")),
    ("ranks", _null_field("cooc", "values_dev")),
    ("scores", lambda lib: _args(lib, batch=None)),
    ("topk", _null_field("batch", "indptr_dev")),
    ("ranks", _null_field("batch", "values_dev")),
    ("scores", lambda lib: _args(lib, scratch=None)),
    ("topk", lambda lib: _args(lib, scratch=None)),
    ("ranks", lambda lib: _args(lib, scratch=None)),
    ("topk", lambda lib: _args(lib, idx=None)),
    ("topk", lambda lib: _args(lib, val=None)),
    ("ranks", lambda lib: _args(lib, ranks=None)),
    ("ranks", lambda lib: _args(lib, truth=None)),
    ("ranks", _null_field("truth", "indices_dev")),
    ("topk", lambda lib: _args(lib, k=0)),
    ("topk", lambda lib: _args(lib, k=51)),                               # k > n_items
    ("topk", lambda lib: _args(lib, k=1025, n_items=5000, ld=5000)),      # k > 1024
    ("scores", lambda lib: _args(lib, ld=49)),
    ("topk", lambda lib: _args(lib, ld=49)),
    ("ranks", lambda lib: _args(lib, ld=49)),
    ("scores", lambda lib: _args(lib, n_items=0)),
    ("topk", lambda lib: _args(lib, n_items=-3)),
    ("ranks", lambda lib: _args(lib, n_items=0)),
]


@pytest.mark.parametrize("case", range(len(_BAD)))
def test_invalid_arguments_are_refused_before_the_device(case):
    from aaerec import _hip
    lib = _hip.load_library()
    which, make = _BAD[case]
    assert _call(lib, which, make(lib)) == -1                  # AAE_EINVAL
    msg = lib.aae_last_error().decode()
    assert msg.startswith("aae_cooc_" + which) and len(msg) > len("aae_cooc_" + which) + 4, msg


def test_a_call_without_rows_launches_nothing():
    from aaerec import _hip
    lib = _hip.load_library()
    for which in ("scores", "topk", "ranks"):
        a = _args(lib)
        a["batch"].n_rows = a["truth"].n_rows = 0
        assert _call(lib, which, a) == 0, which
    a = _args(lib)
    a["truth"].n_rows = 3                                      # truth names another number of rows
    assert _call(lib, "ranks", a) == -1


def test_guard_on_both_sides_of_2_to_the_24():
    from aaerec.cooc import device_route_ok
    Cm = sp.csr_matrix(np.array([[4096, 1], [1, 2]], dtype=np.float64))
    ok = sp.csr_matrix(np.array([[4095, 0], [1, 1]], dtype=np.float64))         # 4095 * 4096 = 2^24 - 4096
    edge = sp.csr_matrix(np.array([[4095, 1], [1, 1]], dtype=np.float64))       # 4096 * 4096 = 2^24: not below it
    assert device_route_ok(ok, Cm)
    assert not device_route_ok(edge, Cm)
    assert not device_route_ok(sp.csr_matrix(np.array([[2048, 2048], [0, 0]], dtype=np.float64)), Cm)      # the row SUM counts
    assert device_route_ok(sp.csr_matrix((2, 2)), Cm) and device_route_ok(ok, sp.csr_matrix((2, 2)))
    # whole numbers only, in X and in C
    assert not device_route_ok(sp.csr_matrix(np.array([[0.5, 0], [1, 1]])), Cm)
    assert not device_route_ok(ok, sp.csr_matrix(np.array([[1.25, 1], [1, 2]])))
    # C has to fit int32 whatever X holds
    big = sp.csr_matrix(np.array([[2.0 ** 31, 0], [0, 1]]))
    assert not device_route_ok(sp.csr_matrix((2, 2)), big)
    assert device_route_ok(sp.csr_matrix((2, 2)), sp.csr_matrix(np.array([[2.0 ** 31 - 1, 0], [0, 1]])))


def test_guard_follows_the_growth_of_order_2():
    from aaerec.cooc import Countbased, device_route_ok
    X = sp.csr_matrix(np.ones((400, 12)))
    rows = sp.csr_matrix(np.ones((3, 12)))
    one, two = Countbased(1, device=None), Countbased(2, device=None)
    one.train(_Rows(X))
    two.train(_Rows(X))
    assert one.cooccurences.max() == 400 and two.cooccurences.max() == 12 * 400 * 400
    np.testing.assert_array_equal(two.cooccurences.toarray(), (one.cooccurences.T @ one.cooccurences).toarray())
    assert 12 * 400 < 2 ** 24 and device_route_ok(rows, one.cooccurences)
    assert 12 * (12 * 400 * 400) >= 2 ** 24 and not device_route_ok(rows, two.cooccurences)
    assert not two.on_device(rows, 5) and not two.on_device(rows)
    assert 12 * 400 * 400 < 2 ** 24 and device_route_ok(sp.csr_matrix(np.eye(3, 12)), two.cooccurences)      # one item a row still fits


def test_str_is_the_references_text():
    from aaerec.cooc import Countbased
    from aaerec.base import Recommender
    assert str(Countbased(2, device=None)) == "Count-based Predictor (order 2)"
    assert str(Countbased(device=None)) == "Count-based Predictor (order 1)"
    assert isinstance(Countbased(device=None), Recommender)
    for name in ("train", "predict", "predict_topk", "predict_ranks"):
        assert callable(getattr(Countbased, name))


def test_predict_is_the_scipy_product():
    from aaerec.cooc import Countbased
    X, T = _corpus(1)
    rec = Countbased(device=None)
    rec.train(_Rows(X))
    got = rec.predict(_Rows(T))
    assert sp.issparse(got)
    np.testing.assert_array_equal(got.toarray(), (T @ (X.T @ X)).toarray())
    rec3 = Countbased(3, device=None)
    rec3.train(_Rows(X))
    C1 = (X.T @ X)
    C2 = C1.T @ C1
    np.testing.assert_array_equal(rec3.predict(_Rows(T)).toarray(), (T @ (C2.T @ C2)).toarray())


@pytest.mark.parametrize("k", [1, 5, 23])
def test_host_route_topk_equals_the_definition_ties_to_the_smaller_id(k):
    from aaerec.cooc import Countbased
    X, T = _corpus(2)
    rec = Countbased(device=None)
    rec.train(_Rows(X))
    assert not rec.on_device(T, k)
    ids, val = rec.predict_topk(_Rows(T), k=k)
    want_ids, want_val, S = _definition(X, T, k)
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == val.shape == (T.shape[0], k)
    np.testing.assert_array_equal(ids, want_ids)
    # (v - min) * (1 / span) in fp32: the difference is exact, the reciprocal and the product round once each
    np.testing.assert_allclose(val, want_val, rtol=2.0 ** -23, atol=0)
    # the corpus does tie: some row's list holds equal scores, in ascending id order
    tied = 0
    for r in range(ids.shape[0]):
        for a, b in zip(ids[r, :-1], ids[r, 1:]):
            if a >= 0 and b >= 0 and S[r, a] == S[r, b]:
                assert a < b
                tied += 1
    assert tied > 0 or k == 1
    if k == 23:      # fewer rankable items than k: -1 / 0 behind them; the all-zero row lists every other item by id
        assert (ids[:-1, -1] == -1).all() and (val[ids < 0] == 0).all()
        z = T.shape[0] - 2
        assert S[z].max() == 0 and ids[z, :22].tolist() == list(range(22)) and (val[z] == 0).all()
        assert ids[-1].tolist() == list(range(23))               # the empty row: nothing known, every score 0


def test_host_route_ranks_equal_the_definition():
    from aaerec.cooc import Countbased
    X, T = _corpus(3)
    n, N = T.shape
    r = np.random.default_rng(9)
    Y = sp.lil_matrix((n, N))
    for d in range(n - 1):
        for i in r.choice(N, size=int(r.integers(0, 10)), replace=False):
            Y[d, i] = 1
    Y[0, T[0].indices[0]] = 1                      # a held-out item that is a known item
    Y = sp.csr_matrix(Y)
    rec = Countbased(device=None)
    rec.train(_Rows(X))
    got = rec.predict_ranks(_Rows(T), Y)
    _, _, S = _definition(X, T, 1)
    assert got.dtype == np.int32 and got.shape == Y.shape
    Yc = Y.copy()
    Yc.sort_indices()
    np.testing.assert_array_equal(got.indices, Yc.indices)
    np.testing.assert_array_equal(got.indptr, Yc.indptr)
    np.testing.assert_array_equal(got.data, _ranks_definition(S, T, Y))
    # a rank <= k is that item's place in the list of k
    ids, _ = rec.predict_topk(_Rows(T), k=N)
    for d in range(n):
        for e in range(got.indptr[d], got.indptr[d + 1]):
            rank = got.data[e]
            if ids[d, rank - 1] >= 0:
                assert ids[d, rank - 1] == got.indices[e]
            else:
                assert got.indices[e] in T[d].indices
    with pytest.raises(ValueError):
        rec.predict_ranks(_Rows(T), Y[:, :N - 1])


def test_non_integer_inputs_take_the_host_route_with_the_same_rule():
    from aaerec.cooc import Countbased
    X, T = _corpus(4)
    half = T.copy()
    half.data = half.data * 0.5
    rec = Countbased(device=None)
    rec.train(_Rows(X))
    a, _ = rec.predict_topk(_Rows(T), k=7)
    b, _ = rec.predict_topk(_Rows(half), k=7)
    np.testing.assert_array_equal(a, b)           # halving every score changes no order and no tie
