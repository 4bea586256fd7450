"""The random baseline without a GPU (aaerec/randbase.py, csrc/abi_random.h): the NumPy restatement of the draws against an
independent build from tests/device_rng.py, their uniformity, the reference's behaviour without a seed, the host route against a
brute-force ranking, and every argument the entry points refuse before anything touches a device."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import device_rng as D
import random_cases as RC


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def _independent(seed, draw, row0, n_rows, n_items):
    key = D.rng_key(seed, draw, 0) ^ ((15 * D.STREAM_MUL) & D.M64)
    w = D.hash_cell(key, np.arange(n_rows, dtype=np.int64) + row0, np.arange(n_items, dtype=np.int64))
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


@pytest.mark.parametrize("row0", [0, 5])
def test_draw_scores_equal_the_generators_words_bit_for_bit(row0):
    from aaerec import randbase
    got = randbase.draw_scores(RC.SEED, 0, row0, 7, 70001)
    want = _independent(RC.SEED, 0, row0, 7, 70001)
    assert got.dtype == np.float32 and got.shape == (7, 70001)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert 0.0 <= got.min() and got.max() < 1.0


def test_a_block_of_rows_is_the_slice_of_the_whole_block():
    from aaerec import randbase
    whole = randbase.draw_scores(RC.SEED, 2, 0, 12, 70001)
    assert np.array_equal(randbase.draw_scores(RC.SEED, 2, 5, 7, 70001), whole[5:12])
    assert np.array_equal(randbase.draw_scores(RC.SEED, 2, 0, 5, 70001), whole[:5])
    assert randbase.draw_scores(RC.SEED, 2, 3, 0, 10).shape == (0, 10)


def test_fewer_bits_are_the_top_bits_of_the_same_words():
    from aaerec import randbase
    v24 = randbase.draw_values(RC.SEED, 0, 0, 3, 4097, 24)
    for bits in (1, 4, 10):
        assert np.array_equal(randbase.draw_values(RC.SEED, 0, 0, 3, 4097, bits), v24 >> np.uint32(24 - bits))
    for bad in (0, 25):
        with pytest.raises(ValueError):
            randbase.draw_values(RC.SEED, 0, 0, 1, 1, bad)


def test_draws_are_uniform():
    """10 x 100 000 cells: the mean of 10^6 uniform draws has standard deviation 0.2887 / 1000; 5 sigma = 0.0015."""
    from aaerec import randbase
    s = randbase.draw_scores(RC.SEED, 0, 0, 10, 100000).astype(np.float64)
    print("mean", s.mean())
    assert abs(s.mean() - 0.5) <= 0.0015


def test_another_draw_or_seed_is_another_block():
    from aaerec import randbase
    a = randbase.draw_scores(RC.SEED, 0, 0, 4, 1000)
    for other in (randbase.draw_scores(RC.SEED, 1, 0, 4, 1000), randbase.draw_scores(RC.SEED + 1, 0, 0, 4, 1000)):
        assert (a != other).mean() > 0.99
    assert np.array_equal(a, randbase.draw_scores(RC.SEED, 0, 0, 4, 1000))


# ---- the class -----------------------------------------------------------------------------------------------------------------
def test_without_a_seed_the_class_is_the_references():
    from aaerec.randbase import RandomBaseline
    from aaerec.base import Recommender
    rec = RandomBaseline()
    assert isinstance(rec, Recommender) and str(rec) == "RNDM baseline" and rec.seed is None and rec.train(None) is None
    X = RC.Rows(sp.random(13, 57, density=0.1, format="csr", random_state=1))
    np.random.seed(0)
    got = rec.predict(X)
    np.random.seed(0)
    want = np.random.rand(13, 57)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert rec.route(X, 10) is None and rec.route(X) is None
    ids, val = rec.predict_topk(X, k=5)
    assert ids.shape == (13, 5) and ids.dtype == np.int32 and (ids >= 0).all() and val.dtype == np.float32
    T = X.tocsr()
    for i in range(13):
        assert not np.isin(ids[i], T.indices[T.indptr[i]:T.indptr[i + 1]]).any()


def test_a_seeded_predict_on_the_host_is_draw_scores():
    from aaerec import randbase
    rec = randbase.RandomBaseline(seed=7, device=None)
    X = RC.Rows(sp.csr_matrix((9, 300)))
    assert np.array_equal(rec.predict(X), randbase.draw_scores(7, 0, 0, 9, 300))
    assert rec.route(X, 10) is None


@pytest.mark.parametrize("k", [1, 10, 33, 300, 310])
def test_the_host_route_lists_equal_a_brute_force_ranking_where_every_boundary_ties(k):
    from aaerec.randbase import RandomBaseline
    T, _, bits = RC.forced_tie_case()
    v = RC.values(7, 1, 0, T.shape[0], 300, bits)
    if k < 300:
        assert any(RC.boundary_ties(v[i], T.indices[T.indptr[i]:T.indptr[i + 1]], k) for i in range(T.shape[0]))
    rec = RandomBaseline(seed=7, device=None)
    rec.bits = bits
    ids, val = rec.predict_topk(RC.Rows(T), k=k, draw=1)
    want_ids, want_val = RC.want_topk(7, 1, 0, T, min(k, 300), bits=bits)
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == (T.shape[0], k)
    assert np.array_equal(ids[:, :300], want_ids) and np.array_equal(val[:, :300], want_val)
    assert (ids[:, 300:] == -1).all() and (val[:, 300:] == 0).all()


def test_the_host_route_ranks_equal_a_brute_force_ranking_with_ties():
    from aaerec.randbase import RandomBaseline
    T, Y, bits = RC.forced_tie_case()
    rec = RandomBaseline(seed=7, device=None)
    rec.bits = bits
    R = rec.predict_ranks(RC.Rows(T), Y, draw=1)
    assert R.dtype == np.int32 and np.array_equal(R.indptr, Y.indptr) and np.array_equal(R.indices, Y.indices)
    want = RC.want_ranks(7, 1, 0, T, Y, bits=bits)
    assert np.array_equal(R.data, want) and want.min() >= 1
    # the ranks of a row are the places of its held-out items in its full list
    ids, _ = rec.predict_topk(RC.Rows(T), k=300, draw=1)
    for i in range(T.shape[0]):
        for e in range(Y.indptr[i], Y.indptr[i + 1]):
            at = np.flatnonzero(ids[i] == Y.indices[e])
            assert at.size == 0 or R.data[e] == at[0] + 1
    means = rec.predict_ranks(RC.Rows(T), Y, metrics=["mrr", "map"], draw=1)
    from aaerec.evaluation import evaluate_ranks
    assert means == evaluate_ranks(R, ["mrr", "map"])


def test_the_recorded_tie_row_is_the_first_the_scan_finds():
    v = RC.values(RC.TIE_SEED, 0, RC.TIE_ROW, 1, RC.TIE_ITEMS)[0]
    assert RC.boundary_ties(v, np.zeros(0, dtype=np.int64), RC.TIE_K)
    assert RC.scan_tie_row(RC.TIE_SEED, RC.TIE_ITEMS, RC.TIE_K, rows=RC.TIE_ROW + 1) == RC.TIE_ROW


# ---- the entry points' argument checks (nothing here reaches a device) ----------------------------------------------------------
@pytest.fixture(scope="module")
def abi():
    from aaerec import _hip
    lib = _hip.load_library()
    room = (ctypes.c_int64 * 8)()                      # a valid host address: no call below gets as far as using it
    ptr = ctypes.cast(room, ctypes.c_void_p)

    def batch(n_rows=3, indptr=ptr, indices=ptr, max_row_nnz=0):
        b = _hip.AaeBatch()
        b.indptr_dev, b.indices_dev, b.values_dev, b.rows_dev = indptr.value, indices.value, None, None
        b.row_start, b.n_rows, b.nnz_bound, b.max_row_nnz = 0, n_rows, 1, max_row_nnz
        return b

    return lib, ptr, batch, ctypes.c_void_p(None)


def _refused(lib, rc, *words):
    msg = lib.aae_last_error().decode()
    assert rc == -1, msg
    for w in words:
        assert w in msg, msg


def test_rand_scores_refuses_bad_arguments(abi):
    lib, ptr, _, null = abi
    f = lib.aae_rand_scores
    _refused(lib, f(1, 0, 0, 24, 10, 3, null, 10, None), "aae_rand_scores", "out_dev")
    _refused(lib, f(1, 0, 0, 24, 0, 3, ptr, 10, None), "aae_rand_scores", "n_items")
    _refused(lib, f(1, 0, 0, 0, 10, 3, ptr, 10, None), "bits")
    _refused(lib, f(1, 0, 0, 25, 10, 3, ptr, 10, None), "bits")
    _refused(lib, f(1, -1, 0, 24, 10, 3, ptr, 10, None), "draw")
    _refused(lib, f(1, 0, -1, 24, 10, 3, ptr, 10, None), "row0")
    _refused(lib, f(1, 0, 0, 24, 10, -3, ptr, 10, None), "n_rows")
    _refused(lib, f(1, 0, 2 ** 31 - 2, 24, 10, 3, ptr, 10, None), "row0 + n_rows", "2^31")
    _refused(lib, f(1, 0, 0, 24, 10, 3, ptr, 9, None), "ld")
    assert f(1, 0, 2 ** 31 - 3, 24, 10, 0, ptr, 10, None) == 0             # no rows: nothing is launched


def test_rand_topk_refuses_bad_arguments(abi):
    lib, ptr, batch, null = abi
    f = lib.aae_rand_topk
    ok = batch()
    _refused(lib, f(1, 0, 0, 24, 10, None, 5, 1, ptr, ptr, None), "aae_rand_topk", "batch")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(batch(indptr=null)), 5, 1, ptr, ptr, None), "batch")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(batch(indices=null)), 5, 1, ptr, ptr, None), "batch")
    _refused(lib, f(1, 0, 0, 24, 0, ctypes.byref(ok), 5, 1, ptr, ptr, None), "n_items")
    for bits in (0, 25, -1):
        _refused(lib, f(1, 0, 0, bits, 10, ctypes.byref(ok), 5, 1, ptr, ptr, None), "bits")
    _refused(lib, f(1, -2, 0, 24, 10, ctypes.byref(ok), 5, 1, ptr, ptr, None), "draw")
    _refused(lib, f(1, 0, -2, 24, 10, ctypes.byref(ok), 5, 1, ptr, ptr, None), "row0")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(batch(n_rows=-1)), 5, 1, ptr, ptr, None), "n_rows")
    _refused(lib, f(1, 0, 2 ** 31 - 2, 24, 10, ctypes.byref(ok), 5, 1, ptr, ptr, None), "row0 + batch->n_rows", "2^31")
    for k, n_items in ((0, 10), (11, 10), (1025, 5000), (-1, 10)):
        _refused(lib, f(1, 0, 0, 24, n_items, ctypes.byref(ok), k, 1, ptr, ptr, None), "k must be in [1, min(1024, n_items)]")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), 5, 1, null, ptr, None), "idx_out_dev")
    assert f(1, 0, 0, 24, 10, ctypes.byref(batch(n_rows=0)), 5, 1, ptr, null, None) == 0        # no rows; scores are optional


def test_rand_ranks_refuses_bad_arguments(abi):
    lib, ptr, batch, null = abi
    f = lib.aae_rand_ranks
    ok, truth = batch(), batch(max_row_nnz=4096)
    _refused(lib, f(1, 0, 0, 24, 10, None, ctypes.byref(truth), 1, ptr, None), "aae_rand_ranks", "batch")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), None, 1, ptr, None), "truth")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), ctypes.byref(batch(indices=null)), 1, ptr, None), "truth")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), ctypes.byref(batch(n_rows=4)), 1, ptr, None), "truth", "rows")
    _refused(lib, f(1, 0, 0, 24, -5, ctypes.byref(ok), ctypes.byref(truth), 1, ptr, None), "n_items")
    _refused(lib, f(1, 0, 0, 30, 10, ctypes.byref(ok), ctypes.byref(truth), 1, ptr, None), "bits")
    _refused(lib, f(1, -1, 0, 24, 10, ctypes.byref(ok), ctypes.byref(truth), 1, ptr, None), "draw")
    _refused(lib, f(1, 0, -1, 24, 10, ctypes.byref(ok), ctypes.byref(truth), 1, ptr, None), "row0")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(batch(n_rows=-2)), ctypes.byref(batch(n_rows=-2)), 1, ptr, None), "n_rows")
    _refused(lib, f(1, 0, 2 ** 31, 24, 10, ctypes.byref(ok), ctypes.byref(truth), 1, ptr, None), "2^31")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), ctypes.byref(batch(max_row_nnz=4097)), 1, ptr, None), "max_row_nnz", "4096")
    _refused(lib, f(1, 0, 0, 24, 10, ctypes.byref(ok), ctypes.byref(truth), 1, null, None), "ranks_out_dev")
    assert f(1, 0, 0, 24, 10, ctypes.byref(batch(n_rows=0)), ctypes.byref(batch(n_rows=0)), 1, ptr, None) == 0
