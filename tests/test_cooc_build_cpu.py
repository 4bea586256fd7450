"""Where `aaerec.cooc.Countbased` builds its co-occurrence matrix (the `build` argument) and the guard of the device build
(`device_build_ok`), as far as they can be checked without a GPU: the guard is a pure function of X, and build="host" - and
build="auto" without a device - is the scipy product the class has always formed, compared here as the (indptr, indices, values)
triple against that product written out in this file."""
import numpy as np
import pytest
import scipy.sparse as sp

from aaerec.cooc import Countbased, device_build_ok


class _Rows:
    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()


def _corpus(seed=3, docs=300, items=90):
    r = np.random.default_rng(seed)
    lens = r.integers(1, 9, size=docs)
    rows = np.repeat(np.arange(docs), lens)
    cols = np.concatenate([r.choice(items, size=int(n), replace=False) for n in lens])
    X = sp.csr_matrix((r.integers(1, 4, size=cols.size).astype(np.float64), (rows, cols)), shape=(docs, items))
    X.sum_duplicates()
    X.sort_indices()
    return X


def _as_it_was(X, order):
    """train() of the class before it had a `build` argument."""
    X = X.tocsr()
    C = (X.T @ X).tocsr()
    for _ in range(order - 1):
        C = (C.T @ C).tocsr()
    C.sum_duplicates()
    C.sort_indices()
    return C


def _same_triple(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data)


def test_guard_accepts_zero_one_and_count_matrices():
    X = _corpus()
    ones = X.copy()
    ones.data[:] = 1.0
    assert device_build_ok(ones) and device_build_ok(X) and X.data.max() == 3
    assert device_build_ok(ones.astype(np.int32)) and device_build_ok(sp.csr_matrix((4, 7)))


def test_guard_rejects_what_scipy_would_treat_differently():
    X = _corpus()
    for bad in (0.5, -1.0, 0.0):                       # a fractional value, a negative one, an explicit stored zero
        Y = X.copy()
        Y.data[5] = bad
        assert Y.nnz == X.nnz and not device_build_ok(Y)
    dup = sp.csr_matrix((np.ones(3), np.array([2, 2, 4]), np.array([0, 3])), shape=(1, 6))
    assert dup.nnz == 3 and not device_build_ok(dup)                                                    # a duplicate column
    unsorted = sp.csr_matrix((np.ones(3), np.array([4, 1, 2]), np.array([0, 3])), shape=(1, 6))
    assert not device_build_ok(unsorted)
    two_rows = sp.csr_matrix((np.ones(4), np.array([3, 5, 0, 1]), np.array([0, 2, 4])), shape=(2, 6))   # descending only across a row end
    assert device_build_ok(two_rows)


def test_guard_bound_on_the_largest_diagonal_entry():
    # 46340^2 + 1984^2 = 2147395600 + 3936256 = 2151331856 >= 2^31; the edge itself: 2^31 = 32768^2 + 32768^2
    def col(a, b):
        return sp.csr_matrix((np.array([a, b], dtype=np.float64), (np.array([0, 1]), np.array([2, 2]))), shape=(2, 5))
    assert 32768 ** 2 + 32768 ** 2 == 2 ** 31 and not device_build_ok(col(32768, 32768))
    assert 32768 ** 2 + 32767 ** 2 == 2 ** 31 - 65535 and device_build_ok(col(32768, 32767))
    # the two sides of the bound itself: 2^31 - 1 and 2^31 as 32768^2 + 32767^2 + 65534 (65535) ones in one column
    for ones, ok in ((65534, True), (65535, False)):
        data = np.concatenate([[32768.0, 32767.0], np.ones(ones)])
        X = sp.csr_matrix((data, (np.arange(data.size), np.full(data.size, 3))), shape=(data.size, 5))
        assert int((data ** 2).sum()) == 2 ** 31 - 1 + (not ok) and device_build_ok(X) == ok
    assert not device_build_ok(col(46340, 1984)) and device_build_ok(col(46340, 1))
    assert not device_build_ok(col(46341, 1))                                                           # one entry alone is too large
    # the two large entries in different columns: each diagonal entry is below the bound
    apart = sp.csr_matrix((np.array([32768.0, 32768.0]), (np.array([0, 1]), np.array([1, 2]))), shape=(2, 5))
    assert device_build_ok(apart)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("build", ["host", "auto"])
def test_host_build_is_the_class_as_it_was(build, order):
    X = _corpus()
    rec = Countbased(order, device=None, build=build)
    rec.train(_Rows(X))
    assert rec.built_on == "host" and rec._dev is None
    want = _as_it_was(X, order)
    _same_triple(rec.cooccurences, want)
    T = _corpus(seed=9, docs=25)
    got = rec.predict(_Rows(T))
    _same_triple(sp.csr_matrix(got), sp.csr_matrix(T @ want))
    assert not rec.on_device(T, 10)


def test_default_build_is_auto_and_bad_arguments_raise():
    assert Countbased(device=None).build == "auto"
    with pytest.raises(ValueError):
        Countbased(device=None, build="device")
    with pytest.raises(ValueError):
        Countbased(device=None, build="gpu")
