"""The most-popular baseline on the device (csrc/popular.h, csrc/abi_popular.h, aaerec/popular.py) against the definition of
tests/popular_cases.py.  Everything is an integer from the counts through to the ranks, so counts, ids and ranks are compared
for EQUALITY; the fp32 scaled scores are held to the bound popular_cases.SCALED_RTOL derives (every count here is below 2^24).

Shapes: N = 300 items (not a multiple of the 64 candidates a wavefront looks at per step; 16 rows = four workgroups of four
wavefronts) with the row kinds popular_cases.test_rows names; the counts also over 1 and 70 001 items (a column every row hits; once more entries than
the grid-stride count kernel has lanes); one end-to-end run at 100 000 items."""
import numpy as np
import pytest
import scipy.sparse as sp

import popular_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- counts --------------------------------------------------------------------------------------------------------------
def _count_matrix(N, rows=2000, seed=3, empty_rows=False):
    """CSR [rows, N] with multiplicities 1-3; column N // 2 is hit by every row (unless the row is emptied)."""
    r = np.random.default_rng(seed + N)
    hot = N // 2
    lists, vals = [], []
    for d in range(rows):
        if empty_rows and d % 7 in (0, 3):
            lists.append(np.zeros(0, dtype=np.int64))
            continue
        ids = np.unique(np.concatenate([[hot], r.integers(0, N, size=int(r.integers(0, 9)))]))
        lists.append(ids)
    ip = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    idx = np.concatenate(lists).astype(np.int32)
    vals = r.integers(1, 4, size=idx.size).astype(np.float64)
    return sp.csr_matrix((vals, idx, ip), shape=(rows, N)), hot


@pytest.mark.parametrize("N", [1, 300, 70001])
@pytest.mark.parametrize("empty_rows", [False, True])
def test_counts_equal_the_column_sums(N, empty_rows):
    from aaerec import _hip
    X, hot = _count_matrix(N, empty_rows=empty_rows)
    want = np.asarray(X.sum(0)).ravel().astype(np.int64)
    if not empty_rows:
        assert (np.diff(X.indptr) > 0).all() and want[hot] >= 2000 and X.data.max() == 3 and X.data.min() == 1
    else:
        assert (np.diff(X.indptr) == 0).sum() > 500
    got = _hip.pop_counts(_hip.DeviceCooc(X, DEV))
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (N,)
    np.testing.assert_array_equal(got.astype(np.int64), want)


def test_counts_beyond_one_pass_of_the_grid():
    """More stored entries than the count kernel has lanes (kPopCountBlocks x kPopNT = 2048 x 256, csrc/popular.h): every lane
    takes a second entry a grid further on, some a third."""
    from aaerec import _hip
    N, rows, per_row = 70001, 3000, 400
    r = np.random.default_rng(21)
    cols = r.integers(0, N, size=(rows, per_row))
    cols[:, 0] = N - 1                                                          # a column every row hits
    X = sp.csr_matrix((r.integers(1, 4, size=cols.size).astype(np.float64), cols.ravel(), per_row * np.arange(rows + 1)), shape=(rows, N))
    X.sum_duplicates()
    X.sort_indices()
    assert X.nnz > 2 * 2048 * 256
    want = np.asarray(X.sum(0)).ravel().astype(np.int64)
    got = _hip.pop_counts(_hip.DeviceCooc(X, DEV)).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.int64), want)
    assert want[N - 1] >= rows and want.max() < 2 ** 31


def test_counts_of_a_matrix_without_entries_or_without_rows_are_zero():
    from aaerec import _hip
    for shape in ((5, 300), (0, 300)):
        got = _hip.pop_counts(_hip.DeviceCooc(sp.csr_matrix(shape), DEV)).cpu().numpy()
        assert got.shape == (300,) and (got == 0).all()


# ---- lists and ranks over N = 300 ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    """The counts, the rows, the uploaded model and the full-call results every test reads: computed once, never written."""
    from aaerec import _hip
    counts = PC.counts_300()
    T, Y = PC.test_rows(counts)
    pop = _hip.DevicePopular(counts, DEV)
    csr, truth = _hip.DeviceCSR(T, DEV), _hip.DeviceCSR(Y, DEV)
    counts.setflags(write=False)
    return dict(counts=counts, T=T, Y=Y, pop=pop, csr=csr, truth=truth, n=T.shape[0])


def test_order_and_its_inverse_are_the_lexsort(case):
    order = PC.order_of(case["counts"])
    np.testing.assert_array_equal(case["pop"].order.cpu().numpy(), order)
    pos = np.empty(PC.N, dtype=np.int64)
    pos[order] = np.arange(PC.N)
    np.testing.assert_array_equal(case["pop"].pos.cpu().numpy(), pos)
    np.testing.assert_array_equal(case["pop"].counts.cpu().numpy(), case["counts"])


@pytest.mark.parametrize("exclude_known", [True, False])
@pytest.mark.parametrize("k", PC.KS)
def test_lists_equal_the_definition(case, k, exclude_known):
    from aaerec import _hip
    ids, val = _hip.pop_topk(case["pop"], case["csr"], 0, case["n"], k, exclude_known=exclude_known)
    want_ids, want_val = PC.want_topk(case["counts"], case["T"], k, exclude_known)
    ids, val = ids.cpu().numpy(), val.cpu().numpy()
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == val.shape == (case["n"], k)
    np.testing.assert_array_equal(ids, want_ids)
    PC.check_scaled(val, want_val)
    assert (val[ids < 0] == 0).all()


@pytest.mark.parametrize("exclude_known", [True, False])
def test_ranks_equal_the_definition(case, exclude_known):
    from aaerec import _hip
    got = _hip.pop_ranks(case["pop"], case["csr"], 0, case["n"], case["truth"], case["Y"].nnz, exclude_known=exclude_known)
    np.testing.assert_array_equal(got.cpu().numpy(), PC.want_ranks(case["counts"], case["T"], case["Y"], exclude_known))


def test_a_truth_id_outside_the_items_ranks_zero(case):
    import torch
    from aaerec import _hip
    Y = case["Y"]
    truth = _hip.DeviceCSR(Y, DEV)
    bad = [int(Y.indptr[1]), int(Y.indptr[4])]                 # the first entry of two non-empty rows
    assert Y.indptr[2] > Y.indptr[1] and Y.indptr[5] > Y.indptr[4]
    truth.indices[bad[0]] = PC.N
    truth.indices[bad[1]] = -3
    torch.cuda.synchronize()
    got = _hip.pop_ranks(case["pop"], case["csr"], 0, case["n"], truth, Y.nnz).cpu().numpy()
    want = PC.want_ranks(case["counts"], case["T"], Y)
    want[bad] = 0
    np.testing.assert_array_equal(got, want)


def test_the_same_rows_through_row_start_an_index_vector_and_two_calls(case):
    import torch
    from aaerec import _hip
    pop, csr, truth, T, Y, n = (case[x] for x in ("pop", "csr", "truth", "T", "Y", "n"))
    k = 65
    full_ids, full_val = (t.cpu().numpy() for t in _hip.pop_topk(pop, csr, 0, n, k))
    full_ranks = _hip.pop_ranks(pop, csr, 0, n, truth, Y.nnz).cpu().numpy()
    per_row = [full_ranks[Y.indptr[r]:Y.indptr[r + 1]] for r in range(n)]
    nnz_of = lambda rows: int(sum(Y.indptr[r + 1] - Y.indptr[r] for r in rows))      # noqa: E731

    # row_start != 0, and the call split in two
    cut = 5
    for r0, cnt in ((cut, n - cut), (0, cut), (3, 6)):
        ids, val = (t.cpu().numpy() for t in _hip.pop_topk(pop, csr, r0, cnt, k))
        assert ids.tobytes() == full_ids[r0:r0 + cnt].tobytes() and val.tobytes() == full_val[r0:r0 + cnt].tobytes()
        ranks = _hip.pop_ranks(pop, csr, r0, cnt, truth, nnz_of(range(r0, r0 + cnt))).cpu().numpy()
        np.testing.assert_array_equal(ranks, np.concatenate(per_row[r0:r0 + cnt]))

    # an index vector: rows out of order, one of them twice
    pick = [13, 0, 7, 7, 15, 2, 9]
    rows = torch.tensor(pick, dtype=torch.int32, device=DEV)
    ids, val = (t.cpu().numpy() for t in _hip.pop_topk(pop, csr, 0, len(pick), k, rows=rows))
    assert ids.tobytes() == full_ids[pick].tobytes() and val.tobytes() == full_val[pick].tobytes()
    ranks = _hip.pop_ranks(pop, csr, 0, len(pick), truth, nnz_of(pick), rows=rows).cpu().numpy()
    np.testing.assert_array_equal(ranks, np.concatenate([per_row[r] for r in pick]))


def test_all_counts_equal_give_the_id_order_and_zero_scores():
    from aaerec import _hip
    N = 70
    pop = _hip.DevicePopular(np.full(N, 3, dtype=np.int64), DEV)
    np.testing.assert_array_equal(pop.order.cpu().numpy(), np.arange(N))
    T = PC.csr_of([[], [0, 1, 69], list(range(64)), list(range(N))], N)
    Y = PC.csr_of([[0, 69], [1, 2], [64, 63, 0], [5]], N)
    ids, val = (t.cpu().numpy() for t in _hip.pop_topk(pop, _hip.DeviceCSR(T, DEV), 0, 4, N))
    want_ids, want_val = PC.want_topk(np.full(N, 3), T, N)
    np.testing.assert_array_equal(ids, want_ids)
    assert ids[2, :7].tolist() == [64, 65, 66, 67, 68, 69, -1] and (ids[3] == -1).all()
    assert (val == 0).all() and (want_val == 0).all()
    ranks = _hip.pop_ranks(pop, _hip.DeviceCSR(T, DEV), 0, 4, _hip.DeviceCSR(Y, DEV), Y.nnz).cpu().numpy()
    np.testing.assert_array_equal(ranks, PC.want_ranks(np.full(N, 3), T, Y))


def test_the_recommender_on_the_device_equals_the_definition(case):
    from aaerec.popular import MostPopular
    X = PC.training_set(case["counts"])
    for count in ("device", "host"):
        rec = MostPopular(device=DEV, count=count)
        rec.train(PC.Rows(X))
        assert rec.counted_on == count and rec.route(PC.Rows(case["T"]), PC.N) == "device" and rec.route(PC.Rows(case["T"])) == "device"
        ids, val = rec.predict_topk(PC.Rows(case["T"]), k=PC.N)
        want_ids, want_val = PC.want_topk(case["counts"], case["T"], PC.N)
        np.testing.assert_array_equal(ids, want_ids)
        PC.check_scaled(val, want_val)
        got = rec.predict_ranks(PC.Rows(case["T"]), case["Y"])
        np.testing.assert_array_equal(got.data, PC.want_ranks(case["counts"], case["T"], case["Y"]))
        np.testing.assert_array_equal(got.indices, case["Y"].indices)
        mp = rec.most_popular                                   # (after a device count: downloaded here)
        assert isinstance(mp, np.matrix) and mp.shape == (1, PC.N) and mp.dtype == X.sum(0).dtype
        np.testing.assert_array_equal(np.asarray(mp).ravel(), case["counts"])
        assert rec.route(PC.Rows(case["T"]), PC.N + 1) is None
        wide, _ = rec.predict_topk(PC.Rows(case["T"]), k=PC.N + 1)                     # the host route, the same lists
        np.testing.assert_array_equal(wide[:, :PC.N], want_ids)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_device_and_host_recommenders_agree_at_100000_items():
    from aaerec.popular import MostPopular
    N, docs, n_test = 100000, 20000, 64
    r = np.random.default_rng(12)
    ids = r.permutation(N)
    p = 1.0 / (np.arange(N) + 10.0)

    def corpus(n):
        lens = r.integers(2, 13, size=n)
        draws = ids[r.choice(N, size=int(lens.sum()), p=p / p.sum())]
        M = sp.csr_matrix((np.ones(draws.size), draws, np.concatenate([[0], np.cumsum(lens)])), shape=(n, N))
        M.sum_duplicates()
        M.sort_indices()
        return M

    X, T = corpus(docs), corpus(n_test)
    held = r.integers(0, N, size=(n_test, 3))
    Y = sp.csr_matrix((np.ones(held.size), held.ravel(), 3 * np.arange(n_test + 1)), shape=T.shape)
    dev, host = MostPopular(device=DEV, count="device"), MostPopular(device=None)
    dev.train(PC.Rows(X))
    host.train(PC.Rows(X))
    assert dev.counted_on == "device" and dev.route(PC.Rows(T), 500) == "device" and dev.route(PC.Rows(T)) == "device"
    assert host.route(PC.Rows(T), 10) is None
    np.testing.assert_array_equal(np.asarray(dev.most_popular), np.asarray(host.most_popular))
    for k in (10, 500):
        a, av = dev.predict_topk(PC.Rows(T), k=k)
        b, bv = host.predict_topk(PC.Rows(T), k=k)
        np.testing.assert_array_equal(a, b)
        # (both routes form the same fp32 expression; each lies within SCALED_RTOL of the exact quotient)
        np.testing.assert_allclose(av, bv, rtol=2 * PC.SCALED_RTOL, atol=0)
        assert ((av == 0) == (bv == 0)).all()
    a, b = dev.predict_ranks(PC.Rows(T), Y), host.predict_ranks(PC.Rows(T), Y)
    np.testing.assert_array_equal(a.data, b.data)
    np.testing.assert_array_equal(a.indices, b.indices)
    assert a.data.min() >= 1 and a.data.max() > 1000


@pytest.mark.parametrize("metrics,method", [(["mrr@5", "p@5"], "predict_topk"), (["mrr", "map"], "predict_ranks")])
def test_evaluation_on_the_device_route_gives_the_host_numbers(metrics, method):
    from aaerec.popular import MostPopular
    rec = MostPopular(device=DEV, count="device")
    asked = PC.counting(rec)
    ev = PC.evaluation_setup(metrics, topk=True)
    got = ev([rec])[0]
    assert asked == [method] and rec.counted_on == "device" and rec.route(ev.test_set, 5) == "device"
    host = PC.evaluation_setup(metrics, topk=True)([MostPopular(device=None)])[0]
    np.testing.assert_array_equal(np.asarray(got, dtype=np.float64), np.asarray(host, dtype=np.float64))
