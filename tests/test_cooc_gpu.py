"""The item co-occurrence baseline on the device (csrc/cooc.h, csrc/abi_cooc.h, aaerec/cooc.py) against the definition, from
scipy and NumPy in this file:

    S = X_test @ (X^T X) in int64;  order by (-S, id) with the input row's items removed;
    scaled = (S - min) / (max - min) over the unmasked row.

Under the exactness guard every score is a whole number fp32 represents, so ids, ranks and the raw score matrix are compared
for EQUALITY.  The device forms a scaled score as fl(fl(v - min) * fl(1 / span)): the difference is exact, the reciprocal and
the product round once each, so it lies within (1 + 2^-24)^2 - 1 < 1.0001 * 2^-23 of the exact quotient, relatively.

Shape: N = 2 * COOC_TILE + 37 items - three tiles, the last one partial; ~2000 training documents of 2-12 items drawn from a
skewed distribution spread over the whole id range (rows of C span all three tiles, many scores tie); 70 test rows with the
edge rows `_build` names."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SCALED_RTOL = 1.0001 * 2.0 ** -23
DEV = "cuda:0"


class _Rows:
    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()


def _lil_to_csr(rows, N):
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.asarray([i for r in rows for i, _ in r], dtype=np.int64)
    val = np.asarray([v for r in rows for _, v in r], dtype=np.float64)
    M = sp.csr_matrix((val, idx, ip), shape=(len(rows), N))
    M.sum_duplicates()
    M.sort_indices()
    return M


def _build(N, docs, n_test, seed, tile):
    r = np.random.default_rng(seed)
    never = 123 % N
    island = sorted({5, (tile + 5) % N, (2 * tile + 5) % N, 77 % N})      # items that only ever occur with each other
    special = {never, *island}
    free = np.asarray([i for i in range(N) if i not in special])
    perm = r.permutation(free)                                            # popularity rank -> id, over the whole range
    p = 1.0 / (np.arange(perm.size) + 4.0)
    p /= p.sum()

    def draw(lo, hi):
        return [(int(i), 1.0) for i in perm[r.choice(perm.size, size=int(r.integers(lo, hi + 1)), replace=False, p=p)]]

    edge = [e for e in (tile - 1, tile, N - 1) if 0 <= e < N and e not in special]
    train = [draw(2, 12) for _ in range(docs)]
    for e in edge:                                                        # the tile-boundary items do occur
        for d in range(3):
            train.append([(e, 1.0)] + draw(2, 5))
    train += [[(i, 1.0) for i in island]] * 2 + [[(island[0], 1.0), (island[-1], 1.0)]]
    X = _lil_to_csr(train, N)
    top = int(perm[0])
    test = [[],                                                           # 0: empty
            [(never, 1.0)],                                               # 1: an item that never occurred: all scores 0
            [(top, 3.0)] + draw(2, 4),                                    # 2: a multiplicity of 3
            [(e, 1.0) for e in edge] or draw(2, 3),                       # 3: ids at COOC_TILE - 1, COOC_TILE, N - 1
            [(i, 1.0) for i in island]]                                   # 4: every item with a non-zero score is known
    while len(test) < n_test:
        test.append(draw(1, 10))
    T = _lil_to_csr(test, N)
    return X, T, dict(never=never, island=island, edge=edge, top=top)


def _definition(X, T):
    Xi = X.astype(np.int64)
    S = np.asarray((T.astype(np.int64) @ (Xi.T @ Xi)).toarray(), dtype=np.int64)
    n, N = S.shape
    order = []                     # per row: every item id, rankable ones first by (-S, id), then the known ones by id
    n_rankable = np.zeros(n, dtype=np.int64)
    for r in range(n):
        known = T.indices[T.indptr[r]:T.indptr[r + 1]]
        o = np.lexsort((np.arange(N), -S[r]))
        is_known = np.zeros(N, dtype=bool)
        is_known[known] = True
        order.append(np.concatenate([o[~is_known[o]], np.sort(known)]))
        n_rankable[r] = N - known.size
    return S, np.stack(order), n_rankable


def _want_topk(S, order, n_rankable, k):
    n = S.shape[0]
    ids = np.full((n, k), -1, dtype=np.int64)
    val = np.zeros((n, k), dtype=np.float64)
    for r in range(n):
        m = int(min(k, n_rankable[r]))
        ids[r, :m] = order[r, :m]
        span = S[r].max() - S[r].min()
        if span:
            val[r, :m] = (S[r, ids[r, :m]] - S[r].min()) / span
    return ids, val


@pytest.fixture(scope="module")
def big():
    """The three-tile corpus, its definition and a trained model: computed once, read by every test, never written."""
    from aaerec import _hip
    from aaerec.cooc import Countbased, device_route_ok
    tile = _hip.COOC_TILE
    N = 2 * tile + 37
    X, T, info = _build(N, 2000, 70, 11, tile)
    S, order, n_rankable = _definition(X, T)
    rec = Countbased(device=DEV)
    rec.train(_Rows(X))
    C = rec.cooccurences
    assert device_route_ok(T, C) and rec.on_device(T, 500)
    # the shape does what it is meant to: rows of C across all three tiles, ties, the edge rows
    spans = [(C.indices[C.indptr[i]:C.indptr[i + 1]] // tile) for i in range(N) if C.indptr[i + 1] > C.indptr[i]]
    assert sum(1 for s in spans if {0, 1, 2} <= set(s.tolist())) > 50
    assert S[0].max() == 0 and S[1].max() == 0 and T[2].data.max() == 3
    assert T[3].indices.tolist() == [tile - 1, tile, N - 1]
    assert set(np.flatnonzero(S[4]).tolist()) == set(info["island"]) == set(T[4].indices.tolist())
    assert np.mean([np.unique(S[r][S[r] > 0]).size < np.count_nonzero(S[r]) for r in range(5, 70)]) > 0.9      # ties
    for a in (S, order, n_rankable):
        a.setflags(write=False)
    return dict(N=N, tile=tile, X=X, T=T, S=S, order=order, n_rankable=n_rankable, rec=rec, info=info)


def test_scores_equal_the_integer_product_cell_for_cell(big):
    import torch
    from aaerec import _hip
    T, S, N, rec = big["T"], big["S"], big["N"], big["rec"]
    n = T.shape[0]
    csr = _hip.DeviceCSR(T, DEV)
    got = _hip.cooc_scores(rec._dev, csr, 0, n).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (n, N)
    np.testing.assert_array_equal(got.astype(np.int64), S)
    assert (got == np.rint(got)).all() and S.max() < 2 ** 24 and S.max() > 500
    # a window of the rows, into a caller's matrix with an odd leading dimension (the scalar-store tail)
    out = torch.full((9, N + 3), -7.0, dtype=torch.float32, device=DEV)
    part = _hip.cooc_scores(rec._dev, csr, 2, 9, out=out).cpu().numpy()
    np.testing.assert_array_equal(part.astype(np.int64), S[2:11])
    assert (out[:, N:] == -7.0).all()                      # nothing is written beyond n_items
    # rows named through rows_dev, in permuted order
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    rows = torch.as_tensor(perm).to(DEV)
    got = _hip.cooc_scores(rec._dev, csr, 0, n, rows=rows).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.int64), S[perm])
    # ids outside [0, n_items), written straight into the device CSR, are skipped
    bad = _hip.DeviceCSR(T, DEV)
    lo = int(T.indptr[6])
    assert T.indptr[7] - lo >= 2
    bad.indices[lo] = N + 5
    bad.indices[lo + 1] = -1
    Tb = T.copy().tolil()
    for j in T.indices[lo:lo + 2]:
        Tb[6, j] = 0
    Xi = big["X"].astype(np.int64)
    want6 = np.asarray((sp.csr_matrix(Tb)[6].astype(np.int64) @ (Xi.T @ Xi)).toarray(), dtype=np.int64)
    got = _hip.cooc_scores(rec._dev, bad, 6, 1).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.int64), want6)


@pytest.mark.parametrize("k", [10, 500])
def test_topk_ids_equal_the_definition(big, k):
    rec, T = big["rec"], big["T"]
    ids, val = rec.predict_topk(_Rows(T), k=k)
    want_ids, want_val = _want_topk(big["S"], big["order"], big["n_rankable"], k)
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == val.shape == (T.shape[0], k)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_allclose(val, want_val, rtol=SCALED_RTOL, atol=0)
    # the span-0 rows (empty; an item that never occurred) list the rankable items by id at score 0
    assert ids[0].tolist() == list(range(k)) and (val[0] == 0).all() and (val[1] == 0).all()
    assert big["info"]["never"] not in ids[1]
    # every item with a non-zero score known: what is left ties at the row's minimum, by id
    assert (val[4] == 0).all() and not set(ids[4].tolist()) & set(big["info"]["island"])


def test_topk_pads_rows_with_fewer_rankable_items_than_k():
    from aaerec.cooc import Countbased
    N = 40
    X, T, _ = _build(N, 150, 12, 3, 16)
    full = sp.csr_matrix(np.ones((1, N)))
    T = sp.vstack([T, full]).tocsr()                                     # a row that knows every item: nothing to rank
    rec = Countbased(device=DEV)
    rec.train(_Rows(X))
    assert rec.on_device(T, N)
    ids, val = rec.predict_topk(_Rows(T), k=N)
    S, order, n_rankable = _definition(X, T)
    want_ids, want_val = _want_topk(S, order, n_rankable, N)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_allclose(val, want_val, rtol=SCALED_RTOL, atol=0)
    assert (ids[-1] == -1).all() and (val[ids < 0] == 0).all()
    assert (np.sum(ids >= 0, axis=1) == n_rankable).all() and (ids[1:, -1] == -1).all() and ids[0, -1] == N - 1


def test_ranks_of_the_held_out_items_and_the_list_of_500(big):
    import torch
    from aaerec import _hip
    rec, T, S, order, N = big["rec"], big["T"], big["S"], big["order"], big["N"]
    n = T.shape[0]
    r = np.random.default_rng(21)
    lens = [0, 1, 8, 9, 20] + [int(v) for v in r.choice([1, 8, 9, 20], size=n - 5)]      # across the groups of 8 slots
    truth = []
    for d in range(n):
        top = order[d, :600]
        pick = r.choice(top, size=lens[d] // 2, replace=False).tolist()                  # half of them near the head of the ranking
        rest = [int(i) for i in r.choice(N, size=4 * lens[d] + 8, replace=False) if i not in pick][:lens[d] - len(pick)]
        truth.append([(int(i), 1.0) for i in pick + rest])
    truth[2][0] = (int(T[2].indices[0]), 1.0)                                             # a held-out item that is a known item
    Y = _lil_to_csr(truth, N)
    assert Y.indptr[1] == 0 and {1, 8, 9, 20} <= set(np.diff(Y.indptr).tolist())
    pos = np.empty_like(order)
    for d in range(n):
        pos[d, order[d]] = np.arange(N)
    want = np.asarray([1 + pos[d, Y.indices[e]] for d in range(n) for e in range(Y.indptr[d], Y.indptr[d + 1])], dtype=np.int64)
    # through the recommender
    got = rec.predict_ranks(_Rows(T), Y)
    assert got.dtype == np.int32 and got.shape == Y.shape
    np.testing.assert_array_equal(got.indptr, Y.indptr)
    np.testing.assert_array_equal(got.indices, Y.indices)
    np.testing.assert_array_equal(got.data, want)
    e_known = int(Y.indptr[2] + np.flatnonzero(Y.indices[Y.indptr[2]:Y.indptr[3]] == T[2].indices[0])[0])
    assert got.data[e_known] == big["n_rankable"][2] + 1                                  # behind every rankable item
    # an id outside the range, written straight into the device CSR: rank 0, the others untouched
    csr, tcsr = _hip.DeviceCSR(T, DEV), _hip.DeviceCSR(Y, DEV)
    e_bad = int(Y.indptr[3] + 8)                                                          # the 9th entry of a 9-entry row
    assert Y.indptr[4] - Y.indptr[3] == 9
    tcsr.indices[e_bad] = N + 1
    ranks = _hip.cooc_ranks(rec._dev, csr, 0, n, tcsr, Y.nnz).cpu().numpy()
    want_bad = want.copy()
    want_bad[e_bad] = 0
    np.testing.assert_array_equal(ranks, want_bad)
    # rows through rows_dev in permuted order: the entries follow the call's row order
    perm = r.permutation(n).astype(np.int32)
    rows = torch.as_tensor(perm).to(DEV)
    tcsr = _hip.DeviceCSR(Y, DEV)
    ranks = _hip.cooc_ranks(rec._dev, csr, 0, n, tcsr, Y.nnz, rows=rows).cpu().numpy()
    np.testing.assert_array_equal(ranks, np.concatenate([want[Y.indptr[d]:Y.indptr[d + 1]] for d in perm]))
    # the list of 500 holds exactly the truth items of rank <= 500, each at position rank - 1
    ids, _ = rec.predict_topk(_Rows(T), k=500)
    hits = 0
    for d in range(n):
        for e in range(Y.indptr[d], Y.indptr[d + 1]):
            if got.data[e] <= 500:
                assert ids[d, got.data[e] - 1] == Y.indices[e]
                hits += 1
            else:
                assert Y.indices[e] not in ids[d]
    assert hits > 100


def test_chunked_and_repeated_calls_agree_bit_for_bit(big):
    from aaerec.cooc import Countbased
    rec, T, N = big["rec"], big["T"], big["N"]
    small = Countbased(scratch_bytes=3 * 4 * ((N + 3) & ~3), device=DEV)
    small.train(_Rows(big["X"]))
    assert small._chunk_rows(N) == 3 and rec._chunk_rows(N) >= T.shape[0]
    Y = sp.csr_matrix((np.ones(3 * T.shape[0]), big["order"][:, [0, 40, 700]].ravel(), 3 * np.arange(T.shape[0] + 1)), shape=T.shape)
    one_ids, one_val = rec.predict_topk(_Rows(T), k=100)
    for other in (small, rec):                       # chunks of 3 rows; the same call again
        ids, val = other.predict_topk(_Rows(T), k=100)
        assert ids.tobytes() == one_ids.tobytes() and val.tobytes() == one_val.tobytes()
    one = rec.predict_ranks(_Rows(T), Y)
    for other in (small, rec):
        again = other.predict_ranks(_Rows(T), Y)
        assert again.data.tobytes() == one.data.tobytes()
    assert sorted(set(one.data.tolist()) - {1, 41, 701}) == []


def _bags():
    from aaerec.datasets import Bags
    rng = np.random.RandomState(4)
    protos = [rng.choice(250, size=9, replace=False) for _ in range(40)]
    data, owners, years = [], [], {}
    for i in range(500):
        k = rng.randint(40)
        data.append(["i%d" % t for t in rng.choice(protos[k], size=rng.randint(3, 8), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // 500
    return Bags(data, owners, {"year": years})


@pytest.mark.parametrize("metrics", [["mrr@10", "map@10", "p@5"], ["mrr", "map"]])
def test_evaluation_takes_the_device_route_and_gives_the_dense_numbers(metrics):
    from aaerec import evaluation as E
    from aaerec.cooc import Countbased
    ev = E.Evaluation(_bags(), 2009, metrics=metrics, logfile=None, topk=True).setup(min_elements=2, drop=1)
    rec = Countbased(device=DEV)
    asked = []
    real = rec.predict
    rec.predict = lambda *a, **kw: (asked.append("predict"), real(*a, **kw))[1]
    got = ev([rec])[0]
    assert asked == [] and rec.on_device(ev.x_test, 10)
    # the dense pipeline on predict()'s matrix, ties ordered by the smaller id: a score that falls with the place in that order
    host = Countbased(device=None)
    host.train(ev.train_set)
    S = np.asarray(host.predict(ev.test_set).toarray())
    n, N = S.shape
    dense = np.zeros((n, N))
    for r in range(n):
        known = ev.x_test.indices[ev.x_test.indptr[r]:ev.x_test.indptr[r + 1]]
        o = np.lexsort((np.arange(N), -S[r]))
        o = o[~np.isin(o, known)]
        dense[r, o] = N - np.arange(o.size)                    # (known items stay at 0, below every rankable item)
    want = E.evaluate(ev.y_test, dense, metrics=metrics)
    print(metrics, np.asarray(got).ravel().tolist(), np.asarray(want).ravel().tolist())
    assert np.asarray(want)[:, 0].min() > 0.05                 # the split is one the baseline can answer
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), rtol=0, atol=1e-12)


def test_order_2_beyond_the_bound_takes_the_host_route_and_agrees(monkeypatch):
    from aaerec import _hip
    from aaerec.cooc import Countbased, device_route_ok
    N = 300
    X, T, _ = _build(N, 4000, 20, 8, 100)
    rec = Countbased(2, device=DEV)
    rec.train(_Rows(X))
    C1 = (X.T @ X)
    C2 = sp.csr_matrix(C1.T @ C1)
    assert abs(T).sum(axis=1).max() * C2.max() >= 2 ** 24 and C2.max() < 2 ** 31
    assert rec._dev is not None and not device_route_ok(T, rec.cooccurences) and not rec.on_device(T, 10)
    for name in ("cooc_topk", "cooc_ranks", "cooc_scores"):
        monkeypatch.setattr(_hip, name, lambda *a, **kw: pytest.fail("the device route was taken beyond the exactness bound"))
    S = np.asarray((T.astype(np.int64) @ C2.astype(np.int64)).toarray(), dtype=np.int64)
    ids, val = rec.predict_topk(_Rows(T), k=25)
    pos = np.empty((T.shape[0], N), dtype=np.int64)
    for r in range(T.shape[0]):
        known = T.indices[T.indptr[r]:T.indptr[r + 1]]
        o = np.lexsort((np.arange(N), -S[r]))
        o = np.concatenate([o[~np.isin(o, known)], np.sort(known)])
        pos[r, o] = np.arange(N)
        np.testing.assert_array_equal(ids[r], o[:25])
    Y = sp.csr_matrix((np.ones(2 * T.shape[0]), np.stack([ids[:, 3], ids[:, 24]], axis=1).ravel(), 2 * np.arange(T.shape[0] + 1)), shape=T.shape)
    Y.sort_indices()
    ranks = rec.predict_ranks(_Rows(T), Y)
    want = [1 + pos[r, Y.indices[e]] for r in range(T.shape[0]) for e in range(Y.indptr[r], Y.indptr[r + 1])]
    np.testing.assert_array_equal(ranks.data, want)
    assert sorted(set(ranks.data.tolist())) == [4, 25]
    # a single-item row of the same model fits the bound again: the device answers it, with the same ids
    monkeypatch.undo()
    one = sp.csr_matrix(([1.0], ([0], [int(T[5].indices[0])])), shape=(1, N))
    assert rec.on_device(one, 25)
    d_ids, _ = rec.predict_topk(_Rows(one), k=25)
    host = Countbased(2, device=None)
    host.train(_Rows(X))
    np.testing.assert_array_equal(d_ids, host.predict_topk(_Rows(one), k=25)[0])
