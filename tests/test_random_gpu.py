"""The random baseline on the device (csrc/randrank.h, csrc/abi_random.h, aaerec/randbase.py) against the definition of
tests/random_cases.py and the host route.  A draw is an integer, its score that integer times 2^-bits and a scaled score one
fp32 formula over exact operands: ids, ranks, scores and scaled scores are all compared for EQUALITY.

Shapes: 1, 63, 64, 65 items (around one wavefront, fewer items than threads), 4097 (one more than the histogram has counters,
sixteen items a thread and one over) and 70 001 (columns beyond 2^16); six rows a case - empty, all but k - 1 items known, every
item known, three rows of ~20 known ids; lists of 1 to 1024."""
import numpy as np
import pytest
import torch

import random_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = RC.SEED
CASES = [(n, k) for n in RC.GRID_ITEMS for k in RC.GRID_KS if k <= n]


def _lists(seed, draw, row0, T, k, exclude_known, bits=24, row_start=0, n_rows=None):
    from aaerec import _hip
    n_rows = T.shape[0] if n_rows is None else n_rows
    idx, val = _hip.rand_topk(seed, draw, row0, T.shape[1], _hip.DeviceCSR(T, DEV), row_start, n_rows, k, exclude_known=exclude_known,
                              bits=bits)
    return idx.cpu().numpy(), val.cpu().numpy()


def _ranks(seed, draw, row0, T, Y, exclude_known, bits=24, row_start=0, n_rows=None):
    from aaerec import _hip
    n_rows = T.shape[0] if n_rows is None else n_rows
    n_truth = int(Y.indptr[row_start + n_rows] - Y.indptr[row_start])
    return _hip.rand_ranks(seed, draw, row0, T.shape[1], _hip.DeviceCSR(T, DEV), row_start, n_rows, _hip.DeviceCSR(Y, DEV), n_truth,
                           exclude_known=exclude_known, bits=bits).cpu().numpy()


def _same_lists(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ---- scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", RC.GRID_ITEMS)
@pytest.mark.parametrize("row0", [0, 3])
def test_scores_equal_draw_scores(n_items, row0):
    from aaerec import _hip, randbase
    got = _hip.rand_scores(SEED, 1, row0, 7, n_items, DEV)
    assert got.dtype == torch.float32 and got.shape[0] == 7 and got.shape[1] >= n_items
    want = randbase.draw_scores(SEED, 1, row0, 7, n_items)
    assert np.array_equal(got[:, :n_items].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, RC.scores(SEED, 1, row0, 7, n_items))


def test_scores_of_more_rows_than_the_grid_has_and_of_fewer_bits():
    from aaerec import _hip, randbase
    got = _hip.rand_scores(SEED, 0, 2, 1500, 65, DEV, bits=10)
    assert np.array_equal(got[:, :65].cpu().numpy(), randbase.draw_scores(SEED, 0, 2, 1500, 65, bits=10))


# ---- lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items,k", CASES)
@pytest.mark.parametrize("exclude_known", [0, 1])
@pytest.mark.parametrize("row0", [0, 3])
def test_lists_equal_the_definition(n_items, k, exclude_known, row0):
    T = RC.grid_rows(n_items, k)
    want = RC.want_topk(SEED, 0, row0, T, k, bool(exclude_known))
    if exclude_known:
        assert (want[0][1] >= 0).sum() == k - 1 and (want[0][2] == -1).all() and (want[0][0] >= 0).all()      # the tail, no list, a full one
    _same_lists(_lists(SEED, 0, row0, T, k, exclude_known), want)


def test_lists_equal_the_host_route_of_the_class():
    from aaerec.randbase import RandomBaseline
    T = RC.grid_rows(4097, 33)
    host = RandomBaseline(seed=SEED, device=None).predict_topk(RC.Rows(T), k=33, draw=2)
    _same_lists(_lists(SEED, 2, 0, T, 33, 1), host)


def test_lists_without_scores():
    from aaerec import _hip
    import ctypes
    T = RC.grid_rows(4097, 10)
    csr = _hip.DeviceCSR(T, DEV)
    idx = torch.full((T.shape[0], 10), -7, dtype=torch.int32, device=DEV)
    b = _hip._csr_batch(csr, 0, T.shape[0])
    with torch.cuda.device(DEV):
        _hip._check(_hip.load_library().aae_rand_topk(SEED, 0, 0, 24, 4097, ctypes.byref(b), 10, 1, _hip._ptr(idx), None, _hip._stream_of(DEV)))
    assert np.array_equal(idx.cpu().numpy(), RC.want_topk(SEED, 0, 0, T, 10)[0])


@pytest.mark.parametrize("bits", [4, 10])
@pytest.mark.parametrize("k", [k for k in RC.GRID_KS])
@pytest.mark.parametrize("exclude_known", [0, 1])
def test_lists_where_the_boundary_ties(bits, k, exclude_known):
    """4097 items over 16 or 1024 values: the k-th and the (k + 1)-th item share a value, and the smaller id is listed."""
    T = RC.grid_rows(4097, k)
    v = RC.values(SEED, 0, 0, T.shape[0], 4097, bits)
    known = [T.indices[T.indptr[i]:T.indptr[i + 1]] if exclude_known else np.zeros(0, dtype=np.int64) for i in range(T.shape[0])]
    tied = [RC.boundary_ties(v[i], known[i], k) for i in range(T.shape[0])]
    assert any(tied)                                                          # (of the fixture: a boundary where the tie rule decides)
    _same_lists(_lists(SEED, 0, 0, T, k, exclude_known, bits=bits), RC.want_topk(SEED, 0, 0, T, k, bool(exclude_known), bits=bits))


def test_a_tie_at_the_boundary_of_1024_among_24_bit_draws():
    T = RC.csr_of([[]], RC.TIE_ITEMS)
    v = RC.values(RC.TIE_SEED, 0, RC.TIE_ROW, 1, RC.TIE_ITEMS)[0]
    assert RC.boundary_ties(v, np.zeros(0, dtype=np.int64), RC.TIE_K)
    want = RC.want_topk(RC.TIE_SEED, 0, RC.TIE_ROW, T, RC.TIE_K)
    assert v[want[0][0, -1]] == np.sort(v)[::-1][RC.TIE_K]                      # the last listed item shares its value with one left out
    _same_lists(_lists(RC.TIE_SEED, 0, RC.TIE_ROW, T, RC.TIE_K, 1), want)


# ---- ranks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", RC.GRID_ITEMS)
@pytest.mark.parametrize("exclude_known", [0, 1])
@pytest.mark.parametrize("row0", [0, 3])
def test_ranks_equal_the_definition(n_items, exclude_known, row0):
    T = RC.grid_rows(n_items, min(10, n_items))
    Y = RC.truth_rows(T, n_items)
    assert list(np.diff(Y.indptr)) == [0, 1, 64, 65, 4096, 65] and Y.indices.max() >= n_items
    want = RC.want_ranks(SEED, 0, row0, T, Y, bool(exclude_known))
    got = _ranks(SEED, 0, row0, T, Y, exclude_known)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want == 0).any() and (n_items < 64 or (want > 0).sum() > 100)


@pytest.mark.parametrize("n_items", [n for n in RC.GRID_ITEMS if n <= 4097])
def test_ranks_equal_the_places_in_the_hosts_full_lists(n_items):
    from aaerec import _hip
    from aaerec.randbase import RandomBaseline
    T = RC.grid_rows(n_items, min(10, n_items))
    Y = RC.truth_rows(T, n_items)
    ids, _ = RandomBaseline(seed=SEED, device=None).predict_topk(RC.Rows(T), k=n_items)
    places = _hip.ranks_from_lists(torch.as_tensor(ids).to(DEV), _hip.DeviceCSR(Y, DEV), 0, T.shape[0], int(Y.nnz)).cpu().numpy()
    got = _ranks(SEED, 0, 0, T, Y, 1)
    listed = places != _hip.RANK_ABSENT
    assert np.array_equal(got[listed], places[listed])
    # what no list holds: a known item (behind every rankable one) or an id beyond the items (rank 0)
    rows = np.repeat(np.arange(T.shape[0]), np.diff(Y.indptr))
    for e in np.flatnonzero(~listed):
        known = T.indices[T.indptr[rows[e]]:T.indptr[rows[e] + 1]]
        assert got[e] == 0 if Y.indices[e] >= n_items else (Y.indices[e] in known and got[e] > n_items - known.size)


@pytest.mark.parametrize("bits", [4, 10])
def test_ranks_among_ties(bits):
    T = RC.grid_rows(4097, 10)
    Y = RC.truth_rows(T, 4097)
    for excl in (0, 1):
        assert np.array_equal(_ranks(SEED, 0, 0, T, Y, excl, bits=bits), RC.want_ranks(SEED, 0, 0, T, Y, bool(excl), bits=bits))


def test_a_row_of_4097_held_out_items_is_refused_by_the_call_and_ranked_on_the_host_by_the_class():
    from aaerec import _hip
    from aaerec.randbase import RandomBaseline
    T = RC.grid_rows(5000, 10)
    Y = RC.csr_of([[1, 2], np.arange(4097), [], [7], [], [4999]], 5000)
    with pytest.raises(_hip.AaeHipError, match="max_row_nnz"):
        _ranks(SEED, 0, 0, T, Y, 1)
    rec = RandomBaseline(seed=SEED, device=DEV)
    assert rec.route(RC.Rows(T), None, Y) is None and rec.route(RC.Rows(T)) == "device" and rec.route(RC.Rows(T), 1024) == "device"
    assert rec.route(RC.Rows(T), 1025) is None
    R = rec.predict_ranks(RC.Rows(T), Y)
    assert np.array_equal(R.data, RC.want_ranks(SEED, 0, 0, T, Y))


# ---- chunks --------------------------------------------------------------------------------------------------------------------
def test_chunks_of_rows_give_the_bits_of_one_call():
    from aaerec import _hip
    r = np.random.default_rng(2)
    T = RC.csr_of([np.sort(r.choice(4097, size=int(s), replace=False)) for s in r.integers(0, 40, size=11)], 4097)
    Y = RC.csr_of([np.sort(r.choice(4097, size=int(s), replace=False)) for s in r.integers(0, 9, size=11)], 4097)
    whole = _lists(SEED, 0, 0, T, 33, 1)
    a, b = _lists(SEED, 0, 0, T, 33, 1, n_rows=4), _lists(SEED, 0, 4, T, 33, 1, row_start=4, n_rows=7)
    _same_lists((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole)
    _same_lists(whole, RC.want_topk(SEED, 0, 0, T, 33))
    ranks = _ranks(SEED, 0, 0, T, Y, 1)
    parts = np.concatenate([_ranks(SEED, 0, 0, T, Y, 1, n_rows=4), _ranks(SEED, 0, 4, T, Y, 1, row_start=4, n_rows=7)])
    assert np.array_equal(parts, ranks) and np.array_equal(ranks, RC.want_ranks(SEED, 0, 0, T, Y))
    s = _hip.rand_scores(SEED, 0, 0, 11, 4097, DEV)[:, :4097].cpu().numpy()
    parts = torch.cat([_hip.rand_scores(SEED, 0, 0, 4, 4097, DEV), _hip.rand_scores(SEED, 0, 4, 7, 4097, DEV)])[:, :4097].cpu().numpy()
    assert np.array_equal(parts.view(np.uint32), s.view(np.uint32))
    # rows named by an index tensor are addressed like every aae_batch's: call row i is row rows[i] of the matrices, row0 + i of the draws
    rows = torch.tensor([9, 2, 2, 10], dtype=torch.int32, device=DEV)
    idx, _ = _hip.rand_topk(SEED, 0, 0, 4097, _hip.DeviceCSR(T, DEV), 0, 4, 33, rows=rows)
    assert np.array_equal(idx.cpu().numpy(), RC.want_topk(SEED, 0, 0, T[[9, 2, 2, 10]], 33)[0])


# ---- the class -----------------------------------------------------------------------------------------------------------------
LIST_NAMES = ["mrr@1000", "map@1000", "p@1000", "ndcg@1000"]
RANK_NAMES = ["mrr", "map", "mrr@1000"]


def _evaluation(names):
    from aaerec.randbase import RandomBaseline
    ev = RC.evaluation_setup(names)
    x = RC.Rows(ev.x_test)
    dev, host = RandomBaseline(seed=7, device=DEV), RandomBaseline(seed=7, device=None)
    assert dev.route(x, 1000) == "device" and dev.route(x, None, ev.y_test) == "device" and host.route(x, 1000) is None
    return ev, x, dev, host


@pytest.mark.parametrize("names,method", [(LIST_NAMES, "predict_topk"), (RANK_NAMES, "predict_ranks")])
def test_the_class_under_evaluation(names, method):
    """300 test rows over 5000 items.  Lists and ranks are the same integers on every route, and with them the metrics the host
    forms: Evaluation gives the same pairs with the device, with device=None, and on a second run; metrics_on="device" gives the
    same pairs twice."""
    ev, x, dev, host = _evaluation(names)
    asked = RC.counting(dev)
    on_host = ev([dev])[0]
    assert asked == [method]
    assert on_host == ev([host])[0] and on_host == ev([dev])[0]
    assert on_host[0][0] > 0
    ev.metrics_on = "device"
    on_dev = ev([dev])[0]
    assert on_dev == ev([dev])[0]
    assert np.all(np.isfinite(np.asarray(on_dev, dtype=np.float64)))
    # another draw: other lists / ranks
    if method == "predict_topk":
        a, b = dev.predict_topk(x, k=1000), dev.predict_topk(x, k=1000, draw=1)
        assert (a[0] != b[0]).mean() > 0.99
        _same_lists(b, host.predict_topk(x, k=1000, draw=1))
        _same_lists(a, RC.want_topk(7, 0, 0, ev.x_test, 1000))
    else:
        a, b = dev.predict_ranks(x, ev.y_test), dev.predict_ranks(x, ev.y_test, draw=1)
        assert (a.data != b.data).mean() > 0.9
        assert np.array_equal(b.data, host.predict_ranks(x, ev.y_test, draw=1).data)
        assert np.array_equal(a.data, RC.want_ranks(7, 0, 0, ev.x_test, ev.y_test.tocsr()))


@pytest.mark.parametrize("names,method", [(LIST_NAMES, "predict_topk"), (RANK_NAMES, "predict_ranks")])
def test_metrics_on_the_device_are_the_hosts_pairs(names, method):
    """Evaluation(metrics_on="device") against "host" and against device=None, for EQUALITY of the (mean, std) pairs: the lists and
    ranks are the same integers on every route, a row here holds one held-out item, so its value is one term on either side, and
    the class has the rows' values reduced by numpy whichever side formed them (ranking.rank_metrics, reduce_on="host").  With the
    device's own reduction (csrc/rank_metrics.h: another order of summation) mrr@1000, p@1000 and ndcg@1000 came out
    one unit in the last place apart: 0.001923789790639141 on the host against 0.0019237897906391407."""
    ev, x, dev, host = _evaluation(names)
    on_host, of_none = ev([dev])[0], ev([host])[0]
    ev.metrics_on = "device"
    on_dev = ev([dev])[0]
    for name, h, n, d in zip(names, on_host, of_none, on_dev):
        print(method, name, "host", repr(float(h[0])), repr(float(h[1])), "device=None", repr(float(n[0])), repr(float(n[1])),
              "device", repr(float(d[0])), repr(float(d[1])))
    assert on_host == of_none
    assert on_dev == on_host and on_dev == ev([host])[0]


def test_a_seeded_predict_on_the_device_is_draw_scores():
    from aaerec import randbase
    X = RC.Rows(RC.grid_rows(4097, 10))
    got = randbase.RandomBaseline(seed=7, device=DEV).predict(X)
    assert got.dtype == np.float32 and np.array_equal(got, randbase.draw_scores(7, 0, 0, 6, 4097))
