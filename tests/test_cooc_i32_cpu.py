"""What the int32 route of the item co-occurrence baseline (aaerec/cooc.py device_route, csrc/abi_cooc.h aae_cooc_*_i32) needs
no device for: the routing rule on both sides of each of its bounds, the library's surface and argument checks, and the host
route on scores past 2^24, where fp32 keys would tie what the definition tells apart:

    S = X_test @ C in int64;  order by (-S, id) with the input row's items removed."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

F32, I32 = "f32", "i32"


class _Rows:
    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()


def _m(a):
    return sp.csr_matrix(np.asarray(a, dtype=np.float64))


# (X, C, device_route, device_route_ok): the old rule's answer is written down beside the new one
_CM = [[4096, 1], [1, 2]]
_POP = [[2.0 ** 30, 0, 0], [0, 5, 0], [0, 0, 7]]                  # item 0 is the popular one
_ROUTES = {
    "just under 2^24 by the old rule": ([[4095, 0], [1, 1]], _CM, F32, True),                   # 4095 * 4096 = 2^24 - 4096
    "one C value raised: the old product passes 2^24": ([[4095, 0], [1, 1]], [[4098, 1], [1, 2]], I32, False),             # 4095 * 4098 > 2^24
    "the old rule's edge, 2^24 itself": ([[4095, 1], [1, 1]], _CM, I32, False),
    "per-row bound 2^31 - 1": ([[1, 0]], [[2.0 ** 31 - 1, 0], [0, 1]], I32, False),
    "per-row bound 2^31": ([[1, 1]], [[2.0 ** 31 - 1, 0], [0, 1]], None, False),
    "per-row bound 2^31 - 1 from two rows of C": ([[2, 1]], [[2.0 ** 30 - 1, 0], [1, 1]], I32, False),      # 2 (2^30 - 1) + 1
    "per-row bound 2^31 from two rows of C": ([[2, 1]], [[2.0 ** 30 - 1, 0], [2, 1]], None, False),
    "a negative multiplicity counts by its magnitude": ([[-2, 1]], [[2.0 ** 30 - 1, 0], [2, 1]], None, False),
    "negative values of C count by their magnitude": ([[1, 0]], [[-(2.0 ** 31 - 1), 5], [0, 1]], I32, False),
    "the popular item is not in the bag": ([[0, 4, 4]], _POP, I32, False),                      # 8 * 2^30 globally, 48 per row
    "the popular item is in the bag": ([[2, 4, 4]], _POP, None, False),
    "max |x| = 2^24": ([[2.0 ** 24, 0]], [[1, 0], [0, 1]], None, False),
    "max |x| = 2^24 - 1 on a C of ones": ([[2.0 ** 24 - 1, 0]], [[1, 0], [0, 1]], F32, True),
    "max |x| = 2^24 - 1 on a C of twos": ([[2.0 ** 24 - 1, 0]], [[2, 0], [0, 1]], I32, False),
    "a fractional x": ([[0.5, 0], [1, 1]], _CM, None, False),
    "a fractional x beyond the old bound": ([[4095.5, 1]], _CM, None, False),
    "a non-whole C": ([[4095, 0], [1, 1]], [[1.25, 1], [1, 2]], None, False),
    "C does not fit int32": ([[1, 0]], [[2.0 ** 31, 0], [0, 1]], None, False),
    "no rows to score": (np.zeros((2, 2)), _CM, F32, True),
    "an empty C": ([[4095, 1]], np.zeros((2, 2)), F32, True),
}


@pytest.mark.parametrize("name", list(_ROUTES))
def test_device_route_on_both_sides_of_every_bound(name):
    from aaerec.cooc import device_route, device_route_ok
    X, Cm, want, want_ok = _ROUTES[name]
    X, Cm = _m(X), _m(Cm)
    assert device_route(X, Cm) == want
    assert device_route(X, Cm, device="cuda:0") == want
    assert device_route(X, Cm, device=None) is None                  # nowhere to upload C to
    assert device_route_ok(X, Cm) is want_ok                         # the old rule answers as it did
    assert (want == F32) == want_ok


def test_the_bound_is_taken_row_by_row_of_the_batch_and_of_c():
    from aaerec.cooc import device_route
    Cm = _m(_POP)
    light, heavy = [0, 4, 4], [2, 0, 0]
    assert device_route(_m([light]), Cm) == I32 and device_route(_m([heavy]), Cm) is None
    assert device_route(_m([light, heavy]), Cm) is None              # one row beyond the bound sends the call to the host
    assert device_route(_m([light, [1, 0, 0]]), Cm) == I32           # 2^30 < 2^31


def test_countbased_routes_without_a_device_and_keeps_on_device():
    from aaerec.cooc import Countbased
    X = sp.csr_matrix(np.ones((400, 12)))
    rows = sp.csr_matrix(np.ones((3, 12)))
    two = Countbased(2, device=None)
    two.train(_Rows(X))
    assert two.route(_Rows(rows), 5) is None and two.route(_Rows(rows)) is None
    assert not two.on_device(rows, 5)
    with pytest.raises(ValueError):
        two.route(_Rows(sp.csr_matrix(np.ones((3, 11)))), 5)         # another number of columns, as predict_topk refuses it


def test_library_exports_the_i32_calls():
    from aaerec import _hip
    lib = _hip.load_library()
    for name in ("aae_cooc_scores_i32", "aae_cooc_topk_i32", "aae_cooc_ranks_i32"):
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
        assert _hip._PROTOS[name] == _hip._PROTOS[name[:-4]]         # the float call's arguments, pointer for pointer
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    for name in ("cooc_scores_i32", "cooc_topk_i32", "cooc_ranks_i32"):
        assert callable(getattr(_hip, name))


def _args(**over):
    from aaerec import _hip
    p = 0x1000                                                       # pointers nothing may dereference
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
    ref = C.byref
    if which == "scores":
        return lib.aae_cooc_scores_i32(ref(a["cooc"]), a["n_items"], ref(a["batch"]), a["scratch"], a["ld"], None)
    if which == "topk":
        return lib.aae_cooc_topk_i32(ref(a["cooc"]), a["n_items"], ref(a["batch"]), a["k"], 1, a["scratch"], a["ld"], a["idx"], a["val"], None)
    return lib.aae_cooc_ranks_i32(ref(a["cooc"]), a["n_items"], ref(a["batch"]), ref(a["truth"]), 1, a["scratch"], a["ld"], a["ranks"], None)


_BAD = [(w, o) for w in ("scores", "topk", "ranks") for o in (dict(scratch=None), dict(ld=49), dict(n_items=0))] + \
       [("topk", dict(k=51)), ("topk", dict(k=0)), ("topk", dict(k=1025, n_items=5000, ld=5000)), ("topk", dict(idx=None)),
        ("topk", dict(val=None)), ("ranks", dict(ranks=None))]


@pytest.mark.parametrize("case", range(len(_BAD)))
def test_i32_calls_refuse_invalid_arguments_before_the_device(case):
    from aaerec import _hip
    lib = _hip.load_library()
    which, over = _BAD[case]
    assert _call(lib, which, _args(**over)) == -1                    # AAE_EINVAL
    msg = lib.aae_last_error().decode()
    assert msg.startswith("aae_cooc_%s_i32: " % which), msg
    a = _args()
    a["batch"].n_rows = a["truth"].n_rows = 0                        # well-formed and without rows: nothing is launched
    assert _call(lib, which, a) == 0


# ---- the host route past 2^24 ---------------------------------------------------------------------------------------
P, A, B, Q, NEG, N = 2, 5, 9, 11, 13, 16


def _past_2_24():
    """Training documents whose X^T X holds C[P][A] = 2^24 + 3 and C[P][B] = 2^24 + 4 (A < B), and test bags that read them."""
    X = sp.lil_matrix((4, N))
    X[0, P], X[0, A], X[0, B] = 1, 2 ** 24 + 3, 2 ** 24 + 4
    X[1, Q], X[1, NEG] = 1, 5
    X[2, 3], X[2, 4], X[2, 7] = 1, 1, 2
    X[3, 4], X[3, 7] = 3, 1
    T = sp.lil_matrix((5, N))
    T[0, P] = 1                                                       # the pair alone
    T[1, P], T[1, Q] = 1, -2                                          # ... and a negative score at NEG: -10
    T[2, P], T[2, 3] = 3, 1                                           # 3 (2^24 + 3) and 3 (2^24 + 4): both need 26 bits
    T[3, Q] = -1                                                      # every non-zero score negative
    return sp.csr_matrix(X), sp.csr_matrix(T)                         # (row 4 stays empty)


def _int64_definition(X, T):
    Xi = X.astype(np.int64)
    S = np.asarray((T.astype(np.int64) @ (Xi.T @ Xi)).toarray(), dtype=np.int64)
    order, n_rankable = [], []
    for r in range(S.shape[0]):
        known = T.indices[T.indptr[r]:T.indptr[r + 1]]
        o = np.lexsort((np.arange(S.shape[1]), -S[r]))
        keep = ~np.isin(o, known)
        order.append(np.concatenate([o[keep], np.sort(known)]))
        n_rankable.append(int(keep.sum()))
    return S, np.stack(order), n_rankable


def test_host_route_orders_scores_that_fp32_would_tie():
    from aaerec.cooc import Countbased, device_route
    X, T = _past_2_24()
    rec = Countbased(device=None)
    rec.train(_Rows(X))
    Cm = rec.cooccurences
    assert Cm[P, A] == 2 ** 24 + 3 and Cm[P, B] == 2 ** 24 + 4 and A < B
    assert np.float32(Cm[P, A]) == np.float32(Cm[P, B])               # fp32 keys tie the pair: the smaller id, A, would come first
    assert rec.route(_Rows(T), 3) is None
    assert device_route(T, Cm) is None                                # (C[A][B] ~ 2^48 does not fit the int32 upload)
    S, order, n_rankable = _int64_definition(X, T)
    assert S[1, NEG] == -10 and S[0, A] == 2 ** 24 + 3 and S[2, B] == 3 * (2 ** 24 + 4) and S[3].max() == 0 > S[3].min()
    for k in (1, 2, 5, N):
        ids, val = rec.predict_topk(_Rows(T), k=k)
        for r in range(T.shape[0]):
            m = min(k, n_rankable[r])
            np.testing.assert_array_equal(ids[r, :m], order[r, :m])
            assert (ids[r, m:] == -1).all() and (val[r, m:] == 0).all()
    ids, val = rec.predict_topk(_Rows(T), k=2)
    assert ids[0].tolist() == [B, A] and ids[1].tolist() == [B, A] and ids[2].tolist() == [B, A]
    # the scaled scores are the fp32 formula over the converted integers
    lo, hi = np.float32(S[1].min()), np.float32(S[1].max())
    np.testing.assert_array_equal(val[1], (S[1, [B, A]].astype(np.float32) - lo) * (np.float32(1) / (hi - lo)))
    # ranks of every item of every row, the known and the negative ones too
    Y = sp.csr_matrix(np.ones((T.shape[0], N)))
    got = rec.predict_ranks(_Rows(T), Y)
    pos = np.empty_like(order)
    for r in range(T.shape[0]):
        pos[r, order[r]] = np.arange(N)
    np.testing.assert_array_equal(got.data.reshape(T.shape[0], N), 1 + pos)
    assert got[1, NEG] == n_rankable[1] and got[1, B] == 1 and got[1, A] == 2 and got[1, P] == n_rankable[1] + 1
