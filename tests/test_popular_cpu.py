"""What the most-popular baseline (aaerec/popular.py, csrc/popular.h, csrc/abi_popular.h) needs no device for: the reference's
train / predict against the fixture, the library's surface and its argument checks, the guards, and the host route of
predict_topk / predict_ranks against the definition of tests/popular_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import popular_cases as PC


# ---- the reference's train / predict -------------------------------------------------------------------------------------
def _fixture():
    z = np.load(PC.GOLDEN)
    n = int(z["n_items"])
    X = sp.csr_matrix((z["train_data"], z["train_indices"], z["train_indptr"]), shape=(z["train_indptr"].size - 1, n))
    T = sp.csr_matrix((z["test_data"], z["test_indices"], z["test_indptr"]), shape=(z["test_indptr"].size - 1, n))
    return z, X, T


def test_train_and_predict_equal_the_reference():
    from aaerec.base import Recommender
    from aaerec.popular import MostPopular
    z, X, T = _fixture()
    assert X.shape == (200, 120) and T.shape == (9, 120)
    rec = MostPopular(device=None)
    assert str(rec) == str(z["model_str"]) == "Most Popular baseline" and isinstance(rec, Recommender)
    assert rec.most_popular is None
    rec.train(PC.Rows(X))
    mp = rec.most_popular
    assert isinstance(mp, np.matrix) and mp.shape == z["most_popular"].shape == (1, 120) and mp.dtype == z["most_popular"].dtype
    np.testing.assert_array_equal(np.asarray(mp), z["most_popular"])
    pred = rec.predict(PC.Rows(T))
    assert isinstance(pred, np.matrix) == bool(z["pred_is_matrix"])
    assert pred.shape == z["pred"].shape == (9, 120) and pred.dtype == z["pred"].dtype
    np.testing.assert_array_equal(np.asarray(pred), z["pred"])
    assert rec.counted_on == "host"


def test_most_popular_keeps_scipys_dtype_for_integer_matrices():
    from aaerec.popular import MostPopular
    X = PC.training_set(PC.counts_300())
    for dt in (np.int32, np.int64, np.float32, np.float64):
        rec = MostPopular(device=None)
        rec.train(PC.Rows(X.astype(dt)))
        want = X.astype(dt).sum(0)
        assert rec.most_popular.dtype == want.dtype and rec._dtype == want.dtype, dt
        np.testing.assert_array_equal(np.asarray(rec.most_popular), np.asarray(want))


# ---- the library's surface -----------------------------------------------------------------------------------------------
def test_library_exports_the_pop_calls_and_the_abi_version_stands():
    from aaerec import _hip
    lib = _hip.load_library()
    for name in ("aae_pop_counts", "aae_pop_topk", "aae_pop_ranks"):
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    with open(os.path.join(PC.ROOT, "include", "aaerec_hip.h")) as fh:
        text = fh.read()
    assert "#define AAE_ABI_VERSION 4" in text
    for name in ("aae_pop_counts(", "aae_pop_topk(", "aae_pop_ranks(", "typedef struct aae_popular {"):
        assert name in text, name
    for name in ("DevicePopular", "pop_counts", "pop_topk", "pop_ranks"):
        assert callable(getattr(_hip, name)), name


def _args(**over):
    """A well-formed aae_pop_* call over pointers nothing may dereference, one argument replaced."""
    from aaerec import _hip
    p = 0x1000
    X, pop, batch, truth = _hip.AaeCooc(), _hip.AaePopular(), _hip.AaeBatch(), _hip.AaeBatch()
    X.indptr_dev = X.indices_dev = X.values_dev = p
    X.n_rows = 7
    pop.counts_dev = pop.order_dev = pop.pos_dev = p
    pop.n_items = 50
    for b in (batch, truth):
        b.indptr_dev = b.indices_dev = b.values_dev = p
        b.n_rows = 4
    a = dict(X=X, pop=pop, batch=batch, truth=truth, n_items=50, k=10, counts=p, idx=p, val=p, ranks=p)
    a.update(over)
    return a


def _call(lib, which, a):
    ref = lambda s: None if s is None else C.byref(s)      # noqa: E731
    if which == "counts":
        return lib.aae_pop_counts(ref(a["X"]), a["n_items"], a["counts"], None)
    if which == "topk":
        return lib.aae_pop_topk(ref(a["pop"]), ref(a["batch"]), a["k"], 1, a["idx"], a["val"], None)
    return lib.aae_pop_ranks(ref(a["pop"]), ref(a["batch"]), ref(a["truth"]), 1, a["ranks"], None)


def _with(kind, field, value):
    def make():
        a = _args()
        setattr(a[kind], field, value)
        return a
    return make


_BAD = [
    ("counts", lambda: _args(X=None)),
    ("counts", _with("X", "indptr_dev", None)),
    ("counts", _with("X", "indices_dev", None)),
    ("counts", _with("X", "values_dev", None)),
    ("counts", lambda: _args(counts=None)),
    ("counts", lambda: _args(n_items=0)),
    ("counts", lambda: _args(n_items=-2)),
    ("counts", _with("X", "n_rows", -1)),
    ("topk", lambda: _args(pop=None)),
    ("topk", _with("pop", "counts_dev", None)),
    ("topk", _with("pop", "order_dev", None)),
    ("ranks", _with("pop", "pos_dev", None)),
    ("topk", _with("pop", "n_items", 0)),
    ("ranks", _with("pop", "n_items", -5)),
    ("topk", lambda: _args(batch=None)),
    ("ranks", lambda: _args(batch=None)),
    ("topk", _with("batch", "indptr_dev", None)),
    ("ranks", _with("batch", "indices_dev", None)),
    ("topk", _with("batch", "n_rows", -1)),
    ("ranks", _with("batch", "n_rows", -1)),
    ("topk", lambda: _args(idx=None)),
    ("topk", lambda: _args(val=None)),
    ("topk", lambda: _args(k=0)),
    ("topk", lambda: _args(k=-1)),
    ("topk", lambda: _args(k=51)),                               # k > n_items
    ("ranks", lambda: _args(truth=None)),
    ("ranks", _with("truth", "indptr_dev", None)),
    ("ranks", _with("truth", "indices_dev", None)),
    ("ranks", _with("truth", "n_rows", 3)),                      # truth names another number of rows
    ("ranks", _with("truth", "n_rows", -4)),
    ("ranks", lambda: _args(ranks=None)),
]


@pytest.mark.parametrize("case", range(len(_BAD)))
def test_invalid_arguments_are_refused_before_the_device(case):
    from aaerec import _hip
    lib = _hip.load_library()
    which, make = _BAD[case]
    assert _call(lib, which, make()) == -1                     # AAE_EINVAL
    msg = lib.aae_last_error().decode()
    assert msg.startswith("aae_pop_" + which) and len(msg) > len("aae_pop_" + which) + 4, msg


def test_a_ranking_call_without_rows_launches_nothing_and_k_may_reach_the_items():
    from aaerec import _hip
    lib = _hip.load_library()
    for which in ("topk", "ranks"):
        for k in (1, 50):                                      # no cap below n_items
            a = _args(k=k)
            a["batch"].n_rows = a["truth"].n_rows = 0
            assert _call(lib, which, a) == 0, (which, k)


# ---- the guards ----------------------------------------------------------------------------------------------------------
def test_device_count_ok_refuses_each_of_its_cases(monkeypatch):
    import torch
    from aaerec import popular
    X = PC.training_set(PC.counts_300())
    assert not popular.device_count_ok(X, None)                               # no device named
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert not popular.device_count_ok(X, "cuda:0")                           # none present
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)            # (only the matrix is looked at from here on)
    assert popular.device_count_ok(X, "cuda:0") and popular.device_count_ok(X.astype(np.int32), "cuda:0")
    assert popular.MostPopular(device="cuda:0").device_count_ok(X) and not popular.MostPopular(device=None).device_count_ok(X)
    assert not popular.device_count_ok(X.tocsc(), "cuda:0") and not popular.device_count_ok(X.toarray(), "cuda:0")
    unsorted = sp.csr_matrix((np.ones(3), np.array([2, 0, 1]), np.array([0, 3])), shape=(1, 4))
    dup = sp.csr_matrix((np.ones(3), np.array([0, 1, 1]), np.array([0, 3])), shape=(1, 4))
    assert not popular.device_count_ok(unsorted, "cuda:0") and not popular.device_count_ok(dup, "cuda:0")
    half = X.copy()
    half.data[5] = 1.5
    assert not popular.device_count_ok(half, "cuda:0")
    # a column whose absolute sum reaches 2^31 - also where the signed sum is small
    edge = sp.csr_matrix(np.array([[2.0 ** 30, 1.0], [2.0 ** 30 - 1, 0.0]]))
    over = sp.csr_matrix(np.array([[2.0 ** 30, 1.0], [2.0 ** 30, 0.0]]))
    cancel = sp.csr_matrix(np.array([[2.0 ** 30, 1.0], [-2.0 ** 30, 0.0]]))
    assert popular.device_count_ok(edge, "cuda:0")
    assert not popular.device_count_ok(over, "cuda:0") and not popular.device_count_ok(cancel, "cuda:0")
    assert popular.device_count_ok(sp.csr_matrix((3, 4)), "cuda:0")           # no entries: nothing to refuse
    with pytest.raises(ValueError):
        popular.MostPopular(device=None, count="device")
    with pytest.raises(ValueError):
        popular.MostPopular(count="gpu")
    rec = popular.MostPopular(device="cuda:0", count="device")
    with pytest.raises(ValueError):
        rec.train(PC.Rows(half))


def test_auto_counts_constant_is_a_bool_and_auto_without_a_device_counts_on_the_host():
    from aaerec import popular
    assert isinstance(popular.AUTO_COUNTS_ON_DEVICE, bool)
    rec = popular.MostPopular(device=None, count="auto")
    rec.train(PC.Rows(PC.training_set(PC.counts_300())))
    assert rec.counted_on == "host" and rec._dev is None


def test_route_is_none_without_a_device_for_fractional_counts_and_for_k_beyond_the_items():
    from aaerec.popular import MostPopular
    counts = PC.counts_300()
    X = PC.training_set(counts)
    T, _ = PC.test_rows(counts)
    rec = MostPopular(device=None)
    rec.train(PC.Rows(X))
    assert rec.route(PC.Rows(T)) is None and rec.route(PC.Rows(T), 10) is None
    # a model that does hold device counts still answers None where the device route is closed: stood in for by a marker,
    # route() only asks whether the object is there
    rec._dev = object()
    assert rec.route(PC.Rows(T), 10) == "device" and rec.route(PC.Rows(T)) == "device" and rec.route(PC.Rows(T), PC.N) == "device"
    assert rec.route(PC.Rows(T), PC.N + 1) is None and rec.route(PC.Rows(T), 0) is None
    half = X.copy()
    half.data = half.data * 0.5
    frac = MostPopular(device="cuda:0", count="host")
    frac.train(PC.Rows(half))                                                  # fractional counts: nothing is uploaded
    assert frac._dev is None and frac.route(PC.Rows(T), 10) is None and frac.route(PC.Rows(T)) is None
    with pytest.raises(ValueError):
        rec.route(PC.Rows(T[:, :PC.N - 1]), 5)


# ---- the host route against the definition -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    from aaerec.popular import MostPopular
    counts = PC.counts_300()
    X = PC.training_set(counts)
    T, Y = PC.test_rows(counts)
    rec = MostPopular(device=None)
    rec.train(PC.Rows(X))
    np.testing.assert_array_equal(np.asarray(rec.most_popular).ravel(), counts)
    # the shape does what it is meant to: ties, a zero block, five items at the maximum, the listed row kinds, mixed truth rows
    assert np.unique(counts).size < 15 and (counts == 0).sum() == 40 and (counts == counts.max()).sum() == 5
    assert np.diff(T.indptr).tolist() == list(PC.KNOWN) * 2
    order = PC.order_of(counts)
    for i, m in enumerate(PC.KNOWN):
        assert set(T[len(PC.KNOWN) + i].indices.tolist()) == set(order[:m].tolist())
    lens = np.diff(Y.indptr)
    assert (lens == 0).any() and (lens > 3).any()
    assert any(np.isin(Y[r].indices, T[r].indices).any() and not np.isin(Y[r].indices, T[r].indices).all() for r in range(T.shape[0]))
    counts.setflags(write=False)
    return dict(counts=counts, X=X, T=T, Y=Y, rec=rec)


@pytest.mark.parametrize("k", PC.KS)
def test_host_route_topk_equals_the_definition(case, k):
    ids, val = case["rec"].predict_topk(PC.Rows(case["T"]), k=k)
    want_ids, want_val = PC.want_topk(case["counts"], case["T"], k)
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == val.shape == (case["T"].shape[0], k)
    np.testing.assert_array_equal(ids, want_ids)
    PC.check_scaled(val, want_val)
    if k == PC.N:
        assert (np.sum(ids >= 0, axis=1) == PC.N - np.diff(case["T"].indptr)).all()        # padded behind the last rankable item


def test_host_route_ranks_equal_the_definition(case):
    got = case["rec"].predict_ranks(PC.Rows(case["T"]), case["Y"])
    assert got.dtype == np.int32 and got.shape == case["Y"].shape
    np.testing.assert_array_equal(got.indices, case["Y"].indices)
    np.testing.assert_array_equal(got.indptr, case["Y"].indptr)
    np.testing.assert_array_equal(got.data, PC.want_ranks(case["counts"], case["T"], case["Y"]))
    with pytest.raises(ValueError):
        case["rec"].predict_ranks(PC.Rows(case["T"]), case["Y"][:, :PC.N - 1])


def test_host_route_answers_k_beyond_the_items_and_all_equal_counts(case):
    ids, val = case["rec"].predict_topk(PC.Rows(case["T"]), k=PC.N + 7)
    want_ids, _ = PC.want_topk(case["counts"], case["T"], PC.N)
    np.testing.assert_array_equal(ids[:, :PC.N], want_ids)
    assert (ids[:, PC.N:] == -1).all() and (val[:, PC.N:] == 0).all()
    from aaerec.popular import MostPopular
    flat = MostPopular(device=None)
    flat.train(PC.Rows(sp.csr_matrix(np.ones((3, 70)))))
    T = PC.csr_of([[], [0, 1, 69], [5]], 70)
    ids, val = flat.predict_topk(PC.Rows(T), k=4)
    assert ids.tolist() == [[0, 1, 2, 3], [2, 3, 4, 5], [0, 1, 2, 3]] and (val == 0).all()


# ---- Evaluation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metrics,method", [(["mrr@5", "p@5"], "predict_topk"), (["mrr", "map"], "predict_ranks")])
def test_evaluation_asks_for_lists_or_ranks_and_gives_the_dense_numbers(metrics, method):
    from aaerec.popular import MostPopular
    rec = MostPopular(device=None)
    asked = PC.counting(rec)
    got = PC.evaluation_setup(metrics, topk=True)([rec])[0]
    assert asked == [method]
    dense_rec = MostPopular(device=None)
    dense_asked = PC.counting(dense_rec)
    dense = PC.evaluation_setup(metrics, topk=False)([dense_rec])[0]
    assert dense_asked == ["predict"]
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(dense, dtype=np.float64), rtol=1e-12, atol=0)
    assert all(0 < mean <= 1 for mean, _ in got)


def test_importing_popular_does_not_make_aaerec_baselines_importable():
    pkg = os.path.join(PC.ROOT, "aae-recommender_amd")
    code = (f"import sys\nsys.path.insert(0, {pkg!r})\nimport aaerec.popular\n"
            "try:\n    import aaerec.baselines\nexcept ModuleNotFoundError as e:\n    print('missing', e.name)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert out.returncode == 0 and out.stdout.strip() == "missing aaerec.baselines", (out.stdout, out.stderr[-2000:])
    assert not os.path.exists(os.path.join(pkg, "aaerec", "baselines.py"))
