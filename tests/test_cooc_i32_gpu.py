"""The int32 route of the item co-occurrence baseline on the device (csrc/cooc.h cooc_scores_kernel<int32_t>, the integer members
of rank_long_dense_kernel / rank_full_dense_kernel, csrc/abi_cooc.h aae_cooc_*_i32, aaerec/cooc.py device_route) against the
definition, from scipy and NumPy in this file:

    S = X_test @ C in int64;  order by (-S, id) with the input row's items removed;
    scaled = (S - min) / (max - min) over the unmasked row.

The scores are ranked as the integers they are, so ids, ranks and the raw int32 score matrix are compared for EQUALITY - past
2^24 too, where fp32 keys tie what the definition tells apart.  The scaled scores are held to the bound of tests/test_cooc_gpu.py,
1.0001 * 2^-23 relative to the exact quotient: the device forms fl(fl(float(v) - float(min)) * fl(1 / span)), and where v, min and
max are whole numbers fp32 represents the difference is exact and the reciprocal and the product round once each,
(1 + 2^-24)^2 - 1 < 1.0001 * 2^-23.  Beyond 2^24 a conversion rounds too, by up to 2^-24 of the converted number, so the
derivation is applied only where it holds: every score of the scaled corpus is a multiple of 2^16 below 2^31, which fp32
represents, and the five hand-made rows that pass 2^24 are gone through one by one in `_small`; the fixtures assert both.

Shapes: a hand-made C over N = 300 items with <= 40 test rows (every row kind `_small` names), and the corpus builder of
tests/test_cooc_gpu.py at N = COOC_TILE + 37 - two tiles, the second partial - with the training multiplicities scaled by 256
so that the scores pass 2^24, 30 test rows."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SCALED_RTOL = 1.0001 * 2.0 ** -23
DEV = "cuda:0"
I31 = 2 ** 31 - 1
KS = [1, 10, 33, 300]


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


# ---- the definition -------------------------------------------------------------------------------------------------
def _order(S, T, exclude_known=True):
    """Per row every item id - the rankable ones first by (-S, id), then the known ones by id - and the number of rankable ones."""
    n, N = S.shape
    order, n_rankable = [], np.zeros(n, dtype=np.int64)
    for r in range(n):
        known = T.indices[T.indptr[r]:T.indptr[r + 1]] if exclude_known else np.zeros(0, dtype=np.int64)
        o = np.lexsort((np.arange(N), -S[r]))
        is_known = np.zeros(N, dtype=bool)
        is_known[known] = True
        order.append(np.concatenate([o[~is_known[o]], np.sort(known)]))
        n_rankable[r] = N - known.size
    return np.stack(order), n_rankable


def _want_topk(S, order, n_rankable, k):
    n = S.shape[0]
    ids = np.full((n, k), -1, dtype=np.int64)
    val = np.zeros((n, k), dtype=np.float64)
    for r in range(n):
        m = int(min(k, n_rankable[r]))
        ids[r, :m] = order[r, :m]
        span = int(S[r].max()) - int(S[r].min())
        if span:
            val[r, :m] = (S[r, ids[r, :m]] - int(S[r].min())) / span
    return ids, val


def _want_ranks(order, Y):
    pos = np.empty_like(order)
    for d in range(order.shape[0]):
        pos[d, order[d]] = np.arange(order.shape[1])
    return np.asarray([1 + pos[d, Y.indices[e]] for d in range(Y.shape[0]) for e in range(Y.indptr[d], Y.indptr[d + 1])], dtype=np.int64)


def _check_topk(ids, val, S, order, n_rankable, k):
    ids, val = ids.cpu().numpy(), val.cpu().numpy()
    want_ids, want_val = _want_topk(S, order, n_rankable, k)
    assert ids.dtype == np.int32 and val.dtype == np.float32 and ids.shape == val.shape == want_ids.shape
    np.testing.assert_array_equal(ids, want_ids)
    err = np.abs(val - want_val) / np.where(want_val != 0, np.abs(want_val), 1.0)
    print("k", k, "scaled scores: largest relative error %.3g of the bound" % (err.max() / SCALED_RTOL))
    np.testing.assert_allclose(val, want_val, rtol=SCALED_RTOL, atol=0)
    assert (val[ids < 0] == 0).all() and (np.sum(ids >= 0, axis=1) == np.minimum(k, n_rankable)).all()
    return ids, val


# ---- the small catalogue --------------------------------------------------------------------------------------------
N_SMALL = 300
PAIR, PA, PB = 7, 20, 21                          # C[PAIR][PA] = 2^24 + 3, C[PAIR][PB] = 2^24 + 4, PA < PB
BIG = (7, 30, 90, 91)                             # rows of C with entries near the int32 range: in no long bag
ROW = dict(empty=0, pair=1, extremes=2, negative=3, top_tie=4, all_known=5, all_zero=6, sum_max=7, sum_min=8, few=9, pair_mixed=10)


def _small():
    """C [300 x 300] and 34 test rows.  Rows 100-299 of C: 12 entries each in (-2^20, 2^20).  The special rows, all below 100:
      7      the pair, 2^24 + 3 at item 20 and 2^24 + 4 at item 21 (fp32 rounds both to 2^24 + 4)
      30     2^31 - 1 and -(2^31 - 1) in one row
      50,51  small values, read with the multiplicities -3 and 2
      60     5000 three times at items 100-102, 4999 at 103: a tie on the first place
      70,71  each other and themselves, nothing else
      80     no entries
      90,91  2^30 and 2^30 - 1 at item 10: their sum is 2^31 - 1, the per-row bound exactly; negated it is -(2^31 - 1)
    The scaled scores of the rows that pass 2^24 (every other row stays below it: the fixture asserts that):
      pair, pair_mixed  min 0, max 2^24 + 4, both exact.  2^24 + 3 converts to 2^24 + 4, off by 2^-24 of itself, and its scaled
                        score is max * fl(1 / max), which is 1 or 1 - 2^-24: at most 2^-24 from the exact 1 - 1 / (2^24 + 4).
                        Every other score of the row is exact in fp32.
      extremes          float(min) = -2^31, float(max) = 2^31, span 2^32, inv 2^-32: all powers of two, every product exact.
                        Only 12345 + 2^31 rounds (to a multiple of 256): 57 / 2^31 < 2^-25.
      sum_max, sum_min  the scores are 0, +-(2^31 - 1) and -+(2^30 - 1): float gives 2^31 and 2^30, each off by less than
                        2^-29; every difference is then 2^30, 2^31 or 3 * 2^30, exact, the span is 3 * 2^30, and only the
                        reciprocal and the product round."""
    r = np.random.default_rng(3)
    N = N_SMALL
    cells = {}
    for i in range(100, N):
        for j in r.choice(N, size=12, replace=False):
            cells[(i, int(j))] = int(r.integers(1, 2 ** 20)) * (1 if r.random() < 0.7 else -1)
    cells.update({(7, PA): 2 ** 24 + 3, (7, PB): 2 ** 24 + 4, (7, 150): 1000, (7, 151): 7,
                  (30, 40): I31, (30, 41): -I31, (30, 42): 12345,
                  (50, 200): 11, (50, 201): 5, (50, 60): 3, (51, 200): 4, (51, 202): 9, (51, 203): -6,
                  (60, 100): 5000, (60, 101): 5000, (60, 102): 5000, (60, 103): 4999,
                  (70, 70): 4, (70, 71): 9, (71, 70): 9, (71, 71): 4,
                  (90, 10): 2 ** 30, (91, 10): 2 ** 30 - 1, (91, 11): -(2 ** 30 - 1)})
    ij = np.asarray(list(cells), dtype=np.int64)
    Cm = sp.csr_matrix((np.asarray(list(cells.values()), dtype=np.int64), (ij[:, 0], ij[:, 1])), shape=(N, N))
    Cm.sort_indices()
    rankable_of_few = {0, *BIG}
    test = [[],                                                          # 0  empty
            [(7, 1)],                                                    # 1  the pair
            [(30, 1)],                                                   # 2  2^31 - 1 and -(2^31 - 1): min, max and span are powers of two in fp32
            [(50, -3), (51, 2)],                                         # 3  negative multiplicities, scores of both signs
            [(60, 1)],                                                   # 4  a tie that straddles k = 1 (and zeros that straddle every other k)
            [(70, 1), (71, 1)],                                          # 5  every non-zero score belongs to a known item
            [(80, 1)],                                                   # 6  all zero: span 0
            [(90, 1), (91, 1)],                                          # 7  a sum of 2^31 - 1
            [(90, -1), (91, -1)],                                        # 8  a sum of -(2^31 - 1)
            [(i, 1) for i in range(N) if i not in rankable_of_few],      # 9  five rankable items: fewer than k = 10, 33, 300
            [(7, 1), (60, 1)]]                                           # 10 the pair among other scores
    while len(test) < 34:
        items = r.choice(np.arange(100, N), size=int(r.integers(1, 7)), replace=False)
        test.append([(int(i), int(r.choice([1, 1, 2, 3, -1]))) for i in items])
    return Cm, _lil_to_csr(test, N)


def _truth(S, order, T, lens, seed):
    """Held-out rows of the given lengths: half of each from the head of its row's ranking, the rest from anywhere."""
    r = np.random.default_rng(seed)
    n, N = S.shape
    truth = []
    for d in range(n):
        pick = r.choice(order[d, :40], size=lens[d] // 2, replace=False).tolist()
        rest = [int(i) for i in r.permutation(N) if i not in pick][:lens[d] - len(pick)]
        truth.append([(int(i), 1.0) for i in pick + rest])
    return truth


@pytest.fixture(scope="module")
def small():
    """The hand-made catalogue on the device and its definition: computed once, read by every test, never written."""
    from aaerec import _hip
    from aaerec.cooc import device_route, device_route_ok
    Cm, T = _small()
    assert device_route(T, Cm) == "i32" and not device_route_ok(T, Cm) and T.shape[0] <= 40
    S = np.asarray((T.astype(np.int64) @ Cm).toarray(), dtype=np.int64)
    # the rows are what their names say
    R = ROW
    assert S[R["pair"], PA] == 2 ** 24 + 3 and S[R["pair"], PB] == 2 ** 24 + 4 and np.float32(2 ** 24 + 3) == np.float32(2 ** 24 + 4)
    assert S[R["extremes"]].max() == I31 and S[R["extremes"]].min() == -I31
    assert S[R["sum_max"]].max() == I31 and S[R["sum_min"]].min() == -I31
    assert (S[R["negative"]] < 0).sum() >= 3 and (S[R["negative"]] > 0).sum() >= 1
    assert S[R["top_tie"], 100:104].tolist() == [5000, 5000, 5000, 4999]
    assert set(np.flatnonzero(S[R["all_known"]]).tolist()) == {70, 71} and not S[R["all_zero"]].any() and not S[R["empty"]].any()
    assert N_SMALL - np.diff(T.indptr)[R["few"]] == 5
    past = sorted(np.flatnonzero(np.abs(S).max(axis=1) >= 2 ** 24).tolist())
    assert past == sorted(R[x] for x in ("pair", "pair_mixed", "extremes", "sum_max", "sum_min"))
    out = {}
    for ex in (1, 0):
        order, n_rankable = _order(S, T, bool(ex))
        out[ex] = (order, n_rankable)
    lens = [0, 1, 8, 9, 17] + [int(v) for v in np.random.default_rng(2).choice([0, 1, 8, 9, 17], size=T.shape[0] - 5)]
    truth = _truth(S, out[1][0], T, lens, 4)
    truth[1][0] = (PAIR, 1.0)                                            # a held-out item that is a known item
    truth[4] = [(100, 1.0), (102, 1.0), (103, 1.0), (PAIR, 1.0)] + [t for t in truth[4] if t[0] not in (100, 102, 103, PAIR)][:13]      # inside the tie
    Y = _lil_to_csr(truth, N_SMALL)
    assert Y.indptr[1] == 0 and {0, 1, 8, 9, 17} <= set(np.diff(Y.indptr).tolist())
    for a in (S, out[0][0], out[1][0]):
        a.setflags(write=False)
    return dict(C=_hip.DeviceCooc(Cm, DEV), Cm=Cm, T=T, csr=_hip.DeviceCSR(T, DEV), S=S, order=out, Y=Y)


def test_scores_i32_equal_the_integer_product_up_to_the_ends_of_int32(small):
    import torch
    from aaerec import _hip
    S, T = small["S"], small["T"]
    n = T.shape[0]
    got = _hip.cooc_scores_i32(small["C"], small["csr"], 0, n)            # a new matrix: ld = 300, the int4 stores
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, N_SMALL)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), S)
    assert S.max() == I31 and S.min() == -I31
    out = torch.full((9, N_SMALL + 3), -7, dtype=torch.int32, device=DEV)      # an odd leading dimension: the scalar stores
    part = _hip.cooc_scores_i32(small["C"], small["csr"], 2, 9, out=out).cpu().numpy()
    np.testing.assert_array_equal(part.astype(np.int64), S[2:11])
    assert (out[:, N_SMALL:] == -7).all()
    with pytest.raises(TypeError):
        _hip.cooc_scores_i32(small["C"], small["csr"], 0, n, out=torch.empty(n, N_SMALL, dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        _hip.cooc_topk(small["C"], small["csr"], 0, n, 5, scratch=torch.empty(n, N_SMALL, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("exclude_known", [1, 0])
@pytest.mark.parametrize("k", KS)
def test_topk_i32_equals_the_definition(small, k, exclude_known):
    from aaerec import _hip
    S, T = small["S"], small["T"]
    order, n_rankable = small["order"][exclude_known]
    ids, val = _hip.cooc_topk_i32(small["C"], small["csr"], 0, T.shape[0], k, exclude_known=bool(exclude_known))
    ids, val = _check_topk(ids, val, S, order, n_rankable, k)
    R = ROW
    for row in ("pair", "pair_mixed"):                                   # the larger score first: float keys would put 20 first
        assert ids[R[row], 0] == PB and (k == 1 or ids[R[row], 1] == PA)
    assert ids[R["top_tie"], :3].tolist() == [100, 101, 102][:k]
    assert (val[R["all_zero"]] == 0).all() and (val[R["empty"]] == 0).all() and ids[R["empty"]].tolist() == list(range(k))
    if exclude_known:
        assert (ids[R["few"]] >= 0).sum() == min(k, 5) and (val[R["all_known"]] == 0).all()
        assert not {70, 71} & set(ids[R["all_known"]].tolist())
    else:
        assert set(ids[R["all_known"], :2].tolist()) == ({70, 71} if k > 1 else {70}) and (ids >= 0).all()
    assert ids[R["sum_max"], 0] == 10 and ids[R["sum_min"], 0] == 11


@pytest.mark.parametrize("exclude_known", [1, 0])
def test_ranks_i32_equal_the_definition(small, exclude_known):
    import torch
    from aaerec import _hip
    T, Y = small["T"], small["Y"]
    n = T.shape[0]
    order, n_rankable = small["order"][exclude_known]
    want = _want_ranks(order, Y)
    tcsr = _hip.DeviceCSR(Y, DEV)
    got = _hip.cooc_ranks_i32(small["C"], small["csr"], 0, n, tcsr, Y.nnz, exclude_known=bool(exclude_known)).cpu().numpy()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    e_known = int(Y.indptr[1] + np.flatnonzero(Y.indices[Y.indptr[1]:Y.indptr[2]] == PAIR)[0])
    S1 = small["S"][1]                                                   # (the item's own score is 0: it ties with every untouched item)
    assert got[e_known] == (n_rankable[1] + 1 if exclude_known else 1 + np.count_nonzero(S1 > 0) + np.count_nonzero(S1[:PAIR] == 0))
    # an id outside the range, written straight into the device CSR: rank 0, the others untouched
    e_bad = int(Y.indptr[3] + 8)
    assert Y.indptr[4] - Y.indptr[3] == 9
    tcsr.indices[e_bad] = N_SMALL + 1
    bad = _hip.cooc_ranks_i32(small["C"], small["csr"], 0, n, tcsr, Y.nnz, exclude_known=bool(exclude_known)).cpu().numpy()
    want_bad = want.copy()
    want_bad[e_bad] = 0
    np.testing.assert_array_equal(bad, want_bad)
    # rows through rows_dev in permuted order: the entries follow the call's row order, and so do the lists
    perm = np.random.default_rng(6).permutation(n).astype(np.int32)
    rows = torch.as_tensor(perm).to(DEV)
    tcsr = _hip.DeviceCSR(Y, DEV)
    got = _hip.cooc_ranks_i32(small["C"], small["csr"], 0, n, tcsr, Y.nnz, rows=rows, exclude_known=bool(exclude_known)).cpu().numpy()
    np.testing.assert_array_equal(got, np.concatenate([want[Y.indptr[d]:Y.indptr[d + 1]] for d in perm]))
    ids, val = _hip.cooc_topk_i32(small["C"], small["csr"], 0, n, 33, rows=rows, exclude_known=bool(exclude_known))
    _check_topk(ids, val, small["S"][perm], order[perm], n_rankable[perm], 33)
    # a window of the rows
    ids, val = _hip.cooc_topk_i32(small["C"], small["csr"], 3, 8, 10, exclude_known=bool(exclude_known))
    _check_topk(ids, val, small["S"][3:11], order[3:11], n_rankable[3:11], 10)


# ---- two tiles, the second partial ------------------------------------------------------------------------------------
def _build(N, docs, n_test, seed, tile):
    """The corpus builder of tests/test_cooc_gpu.py: a skewed popularity spread over the whole id range, the tile-boundary items
    in the training set, the edge rows first."""
    r = np.random.default_rng(seed)
    never = 123 % N
    island = sorted({5, (tile + 5) % N, (2 * tile + 5) % N, 77 % N})      # items that only ever occur with each other
    special = {never, *island}
    free = np.asarray([i for i in range(N) if i not in special])
    perm = r.permutation(free)
    p = 1.0 / (np.arange(perm.size) + 4.0)
    p /= p.sum()

    def draw(lo, hi):
        return [(int(i), 1.0) for i in perm[r.choice(perm.size, size=int(r.integers(lo, hi + 1)), replace=False, p=p)]]

    edge = [e for e in (tile - 1, tile, N - 1) if 0 <= e < N and e not in special]
    train = [draw(2, 12) for _ in range(docs)]
    for e in edge:
        for d in range(3):
            train.append([(e, 1.0)] + draw(2, 5))
    train += [[(i, 1.0) for i in island]] * 2 + [[(island[0], 1.0), (island[-1], 1.0)]]
    X = _lil_to_csr(train, N)
    top = int(perm[0])
    test = [[], [(never, 1.0)], [(top, 3.0)] + draw(2, 4), [(e, 1.0) for e in edge] or draw(2, 3), [(i, 1.0) for i in island]]
    while len(test) < n_test:
        test.append(draw(1, 10))
    return X, _lil_to_csr(test, N), dict(never=never, island=island, edge=edge, top=top)


SCALE = 256


@pytest.fixture(scope="module")
def tiled():
    from aaerec import _hip
    from aaerec.cooc import Countbased
    tile = _hip.COOC_TILE
    N = tile + 37
    X, T, info = _build(N, 2000, 30, 11, tile)
    X.data *= SCALE                                                       # C = 65536 x the counts
    Xi = X.astype(np.int64)
    S = np.asarray((T.astype(np.int64) @ (Xi.T @ Xi)).toarray(), dtype=np.int64)
    rec = Countbased(device=DEV)
    rec.train(_Rows(X))
    assert rec.route(_Rows(T), 1024) == "i32" and rec.route(_Rows(T)) == "i32" and not rec.on_device(T, 10)
    assert not (S % SCALE ** 2).any()                                     # multiples of 2^16 below 2^31: fp32 represents every score
    assert 2 ** 24 < S.max() < 2 ** 31 and info["edge"] == [tile - 1, tile, N - 1] and T[3].indices.tolist() == info["edge"]
    assert S[:, tile - 1].any() and S[:, tile].any() and S[:, N - 1].any()
    order, n_rankable = _order(S, T)
    for a in (S, order, n_rankable):
        a.setflags(write=False)
    return dict(N=N, tile=tile, X=X, T=T, S=S, order=order, n_rankable=n_rankable, rec=rec)


def test_scores_i32_across_the_tile_boundary(tiled):
    from aaerec import _hip
    T, S = tiled["T"], tiled["S"]
    got = _hip.cooc_scores_i32(tiled["rec"]._dev, _hip.DeviceCSR(T, DEV), 0, T.shape[0]).cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.int64), S)


def test_list_of_1024_across_the_tile_boundary(tiled):
    from aaerec import _hip
    T = tiled["T"]
    ids, val = _hip.cooc_topk_i32(tiled["rec"]._dev, _hip.DeviceCSR(T, DEV), 0, T.shape[0], 1024)
    _check_topk(ids, val, tiled["S"], tiled["order"], tiled["n_rankable"], 1024)


def test_countbased_takes_the_i32_route_and_agrees_with_the_host_route(tiled, monkeypatch):
    from aaerec import _hip
    from aaerec.cooc import Countbased
    rec, T, N = tiled["rec"], tiled["T"], tiled["N"]
    n = T.shape[0]
    host = Countbased(device=None)
    host.train(_Rows(tiled["X"]))
    assert host.route(_Rows(T), 10) is None
    for name in ("cooc_topk", "cooc_ranks", "cooc_scores"):
        monkeypatch.setattr(_hip, name, lambda *a, **kw: pytest.fail("the fp32 route was taken beyond its bound"))
    Y = sp.csr_matrix((np.ones(3 * n), tiled["order"][:, [0, 40, 700]].ravel(), 3 * np.arange(n + 1)), shape=T.shape)
    Y.sort_indices()
    small = Countbased(scratch_bytes=7 * 4 * ((N + 3) & ~3), device=DEV)
    small.train(_Rows(tiled["X"]))
    assert small._chunk_rows(N) == 7 and rec._chunk_rows(N) >= n and small.route(_Rows(T), 10) == "i32"
    h_ids, h_val = host.predict_topk(_Rows(T), k=10)
    want_ids, _ = _want_topk(tiled["S"], tiled["order"], tiled["n_rankable"], 10)
    np.testing.assert_array_equal(h_ids, want_ids)
    h_ranks = host.predict_ranks(_Rows(T), Y)
    assert sorted(set(h_ranks.data.tolist())) == [1, 41, 701]
    for dev in (rec, small):                                              # one call; chunks of 7 rows
        ids, val = dev.predict_topk(_Rows(T), k=10)
        assert ids.dtype == np.int32 and val.dtype == np.float32
        np.testing.assert_array_equal(ids, h_ids)
        np.testing.assert_array_equal(val, h_val)                         # the same fp32 formula on both routes
        ranks = dev.predict_ranks(_Rows(T), Y)
        np.testing.assert_array_equal(ranks.indptr, h_ranks.indptr)
        np.testing.assert_array_equal(ranks.indices, h_ranks.indices)
        np.testing.assert_array_equal(ranks.data, h_ranks.data)


# ---- the old domain ---------------------------------------------------------------------------------------------------
def test_same_bits_as_the_float_calls_where_the_f32_rule_admits_the_input():
    from aaerec import _hip
    from aaerec.cooc import Countbased, device_route
    N = 300
    X, T, _ = _build(N, 400, 25, 5, 100)
    T.data[::3] *= -1                                                     # scores of both signs
    rec = Countbased(device=DEV)
    rec.train(_Rows(X))
    assert device_route(T, rec.cooccurences) == "f32" and rec.route(_Rows(T), 10) == "f32" and rec.on_device(T, 10)
    n = T.shape[0]
    csr = _hip.DeviceCSR(T, DEV)
    f = _hip.cooc_scores(rec._dev, csr, 0, n).cpu().numpy()
    i = _hip.cooc_scores_i32(rec._dev, csr, 0, n).cpu().numpy()
    assert (f < 0).any() and (f > 0).any()
    np.testing.assert_array_equal(f, i.astype(np.float32))
    np.testing.assert_array_equal(f.astype(np.int64), i)
    r = np.random.default_rng(9)
    Y = _lil_to_csr([[(int(j), 1.0) for j in r.choice(N, size=int(r.choice([0, 1, 8, 9, 17])), replace=False)] for _ in range(n)], N)
    for ex in (True, False):
        for k in (1, 10, 33, 300):
            f_ids, f_val = _hip.cooc_topk(rec._dev, csr, 0, n, k, exclude_known=ex)
            i_ids, i_val = _hip.cooc_topk_i32(rec._dev, csr, 0, n, k, exclude_known=ex)
            assert f_ids.cpu().numpy().tobytes() == i_ids.cpu().numpy().tobytes()
            assert f_val.cpu().numpy().tobytes() == i_val.cpu().numpy().tobytes()
        tcsr = _hip.DeviceCSR(Y, DEV)
        f_r = _hip.cooc_ranks(rec._dev, csr, 0, n, tcsr, Y.nnz, exclude_known=ex).cpu().numpy()
        i_r = _hip.cooc_ranks_i32(rec._dev, csr, 0, n, tcsr, Y.nnz, exclude_known=ex).cpu().numpy()
        np.testing.assert_array_equal(f_r, i_r)
        assert f_r.min() >= 1


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_i32_calls_refuse_bad_arguments_with_einval(small):
    import torch
    from aaerec import _hip
    lib = _hip.load_library()
    n = 4
    c, b = small["C"].struct(), _hip._csr_batch(small["csr"], 0, n)
    tcsr = _hip.DeviceCSR(small["Y"], DEV)
    t = _hip._csr_batch(tcsr, 0, n)
    scratch = torch.zeros(n, N_SMALL, dtype=torch.int32, device=DEV)
    idx = torch.full((n, 10), -5, dtype=torch.int32, device=DEV)
    val = torch.zeros(n, 10, dtype=torch.float32, device=DEV)
    ranks = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())                                                                   # noqa: E731
    ref = C.byref
    EINVAL = -1
    assert lib.aae_cooc_scores_i32(ref(c), N_SMALL, ref(b), None, N_SMALL, None) == EINVAL                   # a NULL scratch
    assert lib.aae_cooc_topk_i32(ref(c), N_SMALL, ref(b), 10, 1, None, N_SMALL, p(idx), p(val), None) == EINVAL
    assert lib.aae_cooc_ranks_i32(ref(c), N_SMALL, ref(b), ref(t), 1, None, N_SMALL, p(ranks), None) == EINVAL
    assert lib.aae_cooc_scores_i32(ref(c), N_SMALL, ref(b), p(scratch), N_SMALL - 1, None) == EINVAL         # ld < n_items
    assert lib.aae_cooc_topk_i32(ref(c), N_SMALL, ref(b), 10, 1, p(scratch), N_SMALL - 1, p(idx), p(val), None) == EINVAL
    assert lib.aae_cooc_ranks_i32(ref(c), N_SMALL, ref(b), ref(t), 1, p(scratch), N_SMALL - 1, p(ranks), None) == EINVAL
    assert lib.aae_cooc_topk_i32(ref(c), N_SMALL, ref(b), N_SMALL + 1, 1, p(scratch), N_SMALL, p(idx), p(val), None) == EINVAL      # k > n_items
    assert lib.aae_last_error().decode().startswith("aae_cooc_topk_i32: k must be")
    torch.cuda.synchronize()
    assert (idx == -5).all() and not scratch.any()                                                           # nothing was launched
