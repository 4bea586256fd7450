"""The exact int32 sparse product on the device (csrc/spgemm.h, csrc/abi_spgemm.h, `_hip.spgemm_i32`) and the device build of
the co-occurrence matrix (`aaerec.cooc.Countbased(build="device")`) against scipy's product with int64 data on the CPU.

The arithmetic is whole numbers in int32 under a guard that keeps every sum below 2^31, so every comparison is EQUALITY of
indptr, indices and values - never a tolerance.  Shapes are the smallest that reach each branch: rows on either side of the
bin edge SPGEMM_HASH_PRODUCTS, columns that collide in the hash table at every capacity it takes, a result wider than one LDS
tile with entries at the tile's first and last cells, a row of A longer than one staging piece, empty rows everywhere."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class _Rows:
    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()


def _canon(M):
    M = sp.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return M


def _want(A, B):
    """scipy's product with int64 data, canonical."""
    C = _canon(sp.csr_matrix(A).astype(np.int64) @ sp.csr_matrix(B).astype(np.int64))
    assert C.nnz == 0 or (C.data.min() > 0 and C.data.max() < 2 ** 31)
    return C


def _same(got, want):
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data)


def _product(A, B):
    """(the device's A . B on the host, the product bound of every row)."""
    from aaerec import _hip
    a, b = _hip.DeviceCooc(_canon(A), DEV), _hip.DeviceCooc(_canon(B), DEV)
    u = _hip.spgemm_bound(a, b).cpu().numpy()
    C = _hip.spgemm_i32(a, b)
    assert C.indptr.dtype.is_floating_point is False and C.shape == (A.shape[0], B.shape[1]) and C.nnz == int(C.indptr[-1])
    got = C.to_scipy()
    assert got.data.dtype == np.int64 and got.has_canonical_format
    return got, u


def _docs(rng, docs, items, lo, hi, values=(1,)):
    lens = rng.integers(lo, hi + 1, size=docs)
    rows = np.repeat(np.arange(docs), lens)
    cols = np.concatenate([rng.choice(items, size=int(n), replace=False) for n in lens])
    return _canon(sp.csr_matrix((rng.choice(values, size=cols.size).astype(np.float64), (rows, cols)), shape=(docs, items)))


@pytest.fixture(scope="module")
def small():
    """40 x 300, rows of 1-6 items, 0/1: every row of X^T . X stays on the hash path.  Its C is the order-2 case's operand."""
    X = _docs(np.random.default_rng(1), 40, 300, 1, 6)
    return X, _want(X.T, X)


@pytest.fixture(scope="module")
def wide():
    """n = COOC_TILE + 5 items, 700 documents of about 20 with values in {1, 2, 3}; item `hot` is in every document, so its row
    of X^T is longer than one staging piece and its products are far beyond the hash bound; the tile's edge columns occur."""
    from aaerec import _hip
    tile = _hip.COOC_TILE
    n, hot = tile + 5, 4321
    X = _docs(np.random.default_rng(2), 700, n, 17, 22, values=(1, 2, 3)).tolil()
    X[:, hot] = 2
    for d, c in enumerate((0, tile - 1, tile, n - 1)):
        X[d, c] = 3
        X[d + 10, c] = 1
    X = _canon(X.tocsr())
    return X, hot, n, tile


def test_hash_path_alone(small):
    from aaerec import _hip
    X, want = small
    got, u = _product(X.T, X)
    assert u.max() <= _hip.SPGEMM_HASH_PRODUCTS and u.shape == (300,) and want.nnz > 300
    np.testing.assert_array_equal(u, np.asarray(X.T @ np.diff(X.indptr)).ravel())
    _same(got, want)


def test_order_2_is_the_product_with_itself(small):
    # X^T X is symmetric and so is every power of it: C^T C = C . C, which is what the device forms
    _, C = small
    assert (C != C.T).nnz == 0
    got, _ = _product(C, C)
    _same(got, _want(C.T, C))


def test_counts_not_just_zero_one():
    X = _docs(np.random.default_rng(3), 60, 200, 1, 8, values=(1, 2, 3))
    assert set(X.data.tolist()) == {1.0, 2.0, 3.0}
    got, _ = _product(X.T, X)
    want = _want(X.T, X)
    _same(got, want)
    D = X.toarray().astype(np.int64)
    np.testing.assert_array_equal(got.toarray(), D.T @ D)                   # the values are sum_d x_di x_dj


def test_probe_collisions():
    """Columns congruent modulo the table's largest capacity - and so modulo every smaller power of two a row's table takes:
    within a row of B every insert behind the first collides, and neighbouring rows' probe chains run into each other."""
    from aaerec import _hip
    cap = 2 * _hip.SPGEMM_HASH_PRODUCTS
    n = 3 * cap + 10
    rows = [[c + k * cap for k in range(4)] for c in range(6)] + [[7 + k * cap for k in range(3)] + [3 * cap + 9]]
    assert all(len({j % cap for j in r}) <= 2 for r in rows) and max(max(r) for r in rows) == n - 1
    B = sp.csr_matrix((np.arange(1, 29, dtype=np.float64), np.concatenate(rows), 4 * np.arange(8)), shape=(7, n))
    A = sp.csr_matrix(np.array([[1, 1, 1, 1, 1, 1, 1], [0, 2, 0, 3, 0, 1, 0], [5, 0, 0, 0, 0, 0, 0], [1, 2, 3, 1, 2, 3, 1]], dtype=np.float64))
    got, u = _product(A, B)
    assert u.tolist() == [28, 12, 4, 28]
    _same(got, _want(A, B))
    # the same columns many times over: a row of A with 300 entries into rows that all hold the colliding columns
    B2 = sp.vstack([B] * 50).tocsr()
    A2 = sp.csr_matrix(np.ones((2, 350)))
    got, u = _product(A2, B2)
    assert u.tolist() == [1400, 1400]
    _same(got, _want(A2, B2))


def test_bin_edge_rows_take_different_paths_and_both_are_right():
    from aaerec import _hip
    H = _hip.SPGEMM_HASH_PRODUCTS
    r = np.random.default_rng(4)
    per = 64
    assert H % per == 0
    k, n = H // per, 5000
    B = sp.vstack([_docs(r, k, n, per, per, values=(1, 2)), sp.csr_matrix(([1.0], ([0], [n - 1])), shape=(1, n))]).tocsr()
    A = sp.csr_matrix(np.vstack([np.r_[np.ones(k), 0], np.ones(k + 1)]))
    got, u = _product(A, B)
    assert u.tolist() == [H, H + 1]                                         # the last hash row, the first tile row
    _same(got, _want(A, B))


def test_tile_path(wide):
    from aaerec import _hip
    X, hot, n, tile = wide
    A = X.T.tocsr()
    got, u = _product(A, X)
    want = _want(A, X)
    assert n == tile + 5 and u[hot] > _hip.SPGEMM_HASH_PRODUCTS and A.indptr[hot + 1] - A.indptr[hot] == 700 > _hip.SPGEMM_STAGE
    assert (u > _hip.SPGEMM_HASH_PRODUCTS).sum() >= 1 and (u <= _hip.SPGEMM_HASH_PRODUCTS).sum() > 1000      # both paths
    row = want.indices[want.indptr[hot]:want.indptr[hot + 1]]
    assert {0, tile - 1, tile, n - 1} <= set(row.tolist()) and row.size > 5000
    _same(got, want)
    # the edge items' own rows end on either side of the tile boundary
    for c in (0, tile - 1, tile, n - 1):
        assert want.indptr[c + 1] - want.indptr[c] > 20


def test_same_bits_twice(wide):
    import torch
    from aaerec import _hip
    X = wide[0]
    a, b = _hip.DeviceCooc(X.T.tocsr(), DEV), _hip.DeviceCooc(X, DEV)
    one, two = _hip.spgemm_i32(a, b), _hip.spgemm_i32(a, b)
    assert one.nnz == two.nnz > 0
    for x, y in ((one.indptr, two.indptr), (one.indices[:one.nnz], two.indices[:two.nnz]), (one.values[:one.nnz], two.values[:two.nnz])):
        assert torch.equal(x, y)


def test_degenerate_operands():
    r = np.random.default_rng(5)
    X = _docs(r, 30, 50, 1, 5).tolil()
    X[7, :] = 0                                  # a document without items: an empty B row (and an empty column of X^T)
    X[:, 20] = 0                                 # an item no document holds: an empty A row, an empty C row in the middle
    X = _canon(X.tocsr())
    X.eliminate_zeros()
    assert X.indptr[8] == X.indptr[7] and X.T.tocsr().indptr[21] == X.T.tocsr().indptr[20]
    got, u = _product(X.T, X)
    want = _want(X.T, X)
    assert u[20] == 0 and want.indptr[21] == want.indptr[20] and 0 < want.indptr[20] < want.nnz
    _same(got, want)
    # m = 0
    got, u = _product(sp.csr_matrix((0, 30)), X)
    assert got.shape == (0, 50) and got.nnz == 0 and u.size == 0 and got.indptr.tolist() == [0]
    # a product with no entries at all: every entry of A meets an empty row of B
    A = sp.csr_matrix(([1.0, 2.0], ([0, 2], [7, 7])), shape=(3, 30))
    got, u = _product(A, X)
    assert got.shape == (3, 50) and got.nnz == 0 and u.tolist() == [0, 0, 0] and got.indptr.tolist() == [0, 0, 0, 0]
    # operands without any entry
    got, _ = _product(sp.csr_matrix((4, 30)), sp.csr_matrix((30, 9)))
    assert got.shape == (4, 9) and got.nnz == 0


def test_ids_outside_the_range_are_skipped(small):
    from aaerec import _hip
    X, _ = small
    A = X.T.tocsr()
    a, b = _hip.DeviceCooc(A, DEV), _hip.DeviceCooc(X, DEV)
    ra = int(np.flatnonzero(np.diff(A.indptr) >= 2)[0])
    rb = int(np.flatnonzero(np.diff(X.indptr) >= 2)[0])
    ea, eb = int(A.indptr[ra]), int(X.indptr[rb + 1] - 1)
    a.indices[ea] = X.shape[0] + 5               # written straight into the device CSR: beyond p, below 0, beyond n
    a.indices[ea + 1] = -1
    b.indices[eb] = X.shape[1] + 3               # (the last entry of its row: the row stays ascending)
    A2, B2 = A.copy(), X.copy()
    A2.data[ea:ea + 2] = 0
    B2.data[eb] = 0
    A2.eliminate_zeros()
    B2.eliminate_zeros()
    _same(_hip.spgemm_i32(a, b).to_scipy(), _want(A2, B2))


def test_bad_arguments_are_refused_before_the_device(small):
    import ctypes as C
    from aaerec import _hip
    X, _ = small
    a, b = _hip.DeviceCooc(X.T.tocsr(), DEV), _hip.DeviceCooc(X, DEV)
    with pytest.raises(ValueError):
        _hip.spgemm_i32(a, a)                    # [300 x 40] . [300 x 40]
    lib = _hip.load_library()
    sa, sb = a.struct(), b.struct()
    u = _hip.spgemm_bound(a, b)
    assert lib.aae_spgemm_i32_count(C.byref(sa), C.byref(sb), 300, _hip._ptr(u), None, None) != 0
    assert lib.aae_spgemm_i32_fill(C.byref(sa), C.byref(sb), -1, _hip._ptr(u), _hip._ptr(u), _hip._ptr(u), _hip._ptr(u), None) != 0
    sa.n_rows = -2
    assert lib.aae_spgemm_i32_bound(C.byref(sa), C.byref(sb), 40, _hip._ptr(u), None) != 0
    assert lib.aae_spgemm_i32_bound(None, C.byref(sb), 40, _hip._ptr(u), None) != 0


# ---- Countbased end to end ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """700 items, 400 documents of about 12 with item 5 in every one: its row of X^T is a tile row, the others hash rows; at
    order 2 most rows are tile rows and the rare items' rows hash rows."""
    r = np.random.default_rng(6)
    X = _docs(r, 400, 700, 8, 14).tolil()
    X[:, 5] = 1
    X = _canon(X.tocsr())
    T = _docs(r, 30, 700, 1, 6)
    Y = _docs(r, 30, 700, 1, 4)
    return X, T, Y


@pytest.mark.parametrize("order", [1, 2])
def test_device_build_equals_host_build(corpus, order):
    from aaerec import _hip
    from aaerec.cooc import Countbased
    X, T, Y = corpus
    host, dev = Countbased(order, device=DEV, build="host"), Countbased(order, device=DEV, build="device")
    host.train(_Rows(X))
    dev.train(_Rows(X))
    assert host.built_on == "host" and dev.built_on == "device" and dev._cooc is None
    # both kernels ran at this order
    A = _hip.DeviceCooc(X.T.tocsr(), DEV) if order == 1 else _hip.DeviceCooc(_want(X.T, X), DEV)
    u = _hip.spgemm_bound(A, _hip.DeviceCooc(X, DEV) if order == 1 else A).cpu().numpy()
    assert (u > _hip.SPGEMM_HASH_PRODUCTS).any() and (u <= _hip.SPGEMM_HASH_PRODUCTS).sum() > 5
    assert dev.on_device(T, 10) and host.on_device(T, 10)
    h_ids, h_val = host.predict_topk(_Rows(T), k=10)
    d_ids, d_val = dev.predict_topk(_Rows(T), k=10)
    np.testing.assert_array_equal(d_ids, h_ids)
    np.testing.assert_array_equal(d_val, h_val)
    h_r, d_r = host.predict_ranks(_Rows(T), Y), dev.predict_ranks(_Rows(T), Y)
    _same(d_r, h_r)
    assert dev._cooc is None                     # none of this downloaded C
    C = dev.cooccurences
    assert C.dtype == host.cooccurences.dtype and dev._cooc is C
    _same(C, host.cooccurences)
    _same(sp.csr_matrix(dev.predict(_Rows(T))), sp.csr_matrix(host.predict(_Rows(T))))


def test_order_2_beyond_the_int32_bound(monkeypatch):
    """400 identical documents of 10 items with the value 7: C = 19600 on a 10 x 10 block, sum_j C_ij^2 = 10 * 19600^2 >= 2^31
    while no single entry is too large - the device forms order 1 and must not form order 2."""
    from aaerec import _hip, cooc
    r = np.random.default_rng(7)
    block = sp.csr_matrix((np.full(4000, 7.0), (np.repeat(np.arange(400), 10), np.tile(np.arange(20, 30), 400))), shape=(400, 60))
    X = _canon(sp.vstack([block, _docs(r, 50, 60, 1, 4)]))
    assert cooc.device_build_ok(X) and 19600 ** 2 < 2 ** 31 <= 10 * 19600 ** 2
    host = cooc.Countbased(2, device=DEV, build="host")
    host.train(_Rows(X))
    with pytest.raises(ValueError):
        cooc.Countbased(2, device=DEV, build="device").train(_Rows(X))
    # "auto" with the device preferred: order 1 there, then scipy from the downloaded matrix - the host's result
    calls = []
    real = _hip.spgemm_i32
    monkeypatch.setattr(cooc, "AUTO_BUILDS_ON_DEVICE", True)
    monkeypatch.setattr(_hip, "spgemm_i32", lambda *a: (calls.append(1), real(*a))[1])
    auto = cooc.Countbased(2, device=DEV, build="auto")
    auto.train(_Rows(X))
    assert len(calls) == 1 and auto.built_on == "host"
    assert auto.cooccurences.dtype == host.cooccurences.dtype
    _same(auto.cooccurences, host.cooccurences)
    # and where the bound holds "auto" stays on the device
    calls.clear()
    fine = cooc.Countbased(2, device=DEV, build="auto")
    fine.train(_Rows(X[400:]))
    assert len(calls) == 2 and fine.built_on == "device"


def test_on_device_answers_without_downloading(corpus):
    from aaerec.cooc import Countbased
    X, T, _ = corpus
    host, dev = Countbased(device=DEV, build="host"), Countbased(device=DEV, build="device")
    host.train(_Rows(X))
    dev.train(_Rows(X))
    heavy = T.copy()
    heavy.data[:] = 2.0 ** 20                    # whole numbers, but the scores leave 2^24
    half = T.copy()
    half.data[0] = 0.5
    answers = [dev.on_device(M, k) for M in (T, heavy, half) for k in (None, 10, 5000)]
    assert dev._cooc is None
    assert answers == [host.on_device(M, k) for M in (T, heavy, half) for k in (None, 10, 5000)]
    assert answers[:3] == [True, True, False] and not any(answers[3:])
