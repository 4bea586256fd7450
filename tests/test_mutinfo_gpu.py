"""The mutual information of a dataset on the device (csrc/mutinfo.h, csrc/abi_mutinfo.h, `_hip.mutual_info_i32`,
`aaerec.utils.mutual_info(device=...)`) against scipy's int64 contingency table and scikit-learn's mutual_info_score on the CPU.

Every case is judged as tests/mi_cases.py says: T and row_pi by EQUALITY, row_s1 per row and mi within their float64 bounds.
No case asserts on mi alone: a dropped entry moves a row's row_pi by an integer.  Figures are printed before they are asserted."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import mi_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _device(X, Y):
    """(mi, T, row_s1, row_pi on the host, the product bound of every row) by the route aaerec.utils takes: X is uploaded and
    transposed on the device."""
    from aaerec import _hip
    a, b = _hip.cooc_transpose(_hip.DeviceCooc(X, DEV)), _hip.DeviceCooc(Y, DEV)
    u = _hip.spgemm_bound(a, b).cpu().numpy()
    mi, T, s1, pi = _hip.mutual_info_i32(a, b)
    assert isinstance(mi, float) and isinstance(T, int) and s1.dtype.is_floating_point and s1.element_size() == 8 and pi.element_size() == 8
    assert s1.is_cuda and pi.is_cuda and s1.shape == pi.shape == (X.shape[1],)
    return mi, T, s1.cpu().numpy(), pi.cpu().numpy(), u


def _judge(name, got, t):
    mi, T, s1, pi, _ = got
    err = np.abs(s1 - t["row_s1"])
    live = t["s1_bound"] > 0
    ratio = float((err[live] / t["s1_bound"][live]).max()) if live.any() else 0.0
    print("{}: T {} | mi {!r} scikit-learn {!r} |diff| {:.3e} bound {:.3e} | row_s1 max |diff| {:.3e}, largest |diff| / bound {:.3e}, "
          "|diff| where the bound is 0: {:.1e}".format(name, T, mi, t["mi"], abs(mi - t["mi"]), t["mi_bound"], float(err.max()), ratio,
                                                      float(err[~live].max()) if (~live).any() else 0.0))
    assert T == t["T"]
    np.testing.assert_array_equal(pi, t["pi"])
    assert np.all(np.isfinite(s1)) and np.all(err <= t["s1_bound"])
    assert np.isfinite(mi) and mi >= 0.0 and abs(mi - t["mi"]) <= t["mi_bound"]


def test_hash_path_alone():
    X, Y, t = mi_cases.case("small")
    got = _device(X, Y)
    assert got[4].max() <= mi_cases.SPGEMM_HASH_PRODUCTS and t["C"].nnz > 300
    _judge("small", got, t)


def test_bin_edge_rows_take_different_kernels():
    from aaerec import _hip
    assert (_hip.SPGEMM_HASH_PRODUCTS, _hip.COOC_TILE, _hip.SPGEMM_STAGE) == (mi_cases.SPGEMM_HASH_PRODUCTS, mi_cases.COOC_TILE, mi_cases.SPGEMM_STAGE)
    X, Y, t = mi_cases.case("bin_edge")
    got = _device(X, Y)
    assert got[4].tolist() == [_hip.SPGEMM_HASH_PRODUCTS, _hip.SPGEMM_HASH_PRODUCTS + 1]
    _judge("bin_edge", got, t)


@pytest.mark.parametrize("name", ["collide_small", "collide"])
def test_colliding_columns_at_every_capacity(name):
    X, Y, t = mi_cases.case(name)
    got = _device(X, Y)
    assert got[4].tolist() == ([28, 12, 4, 28] if name == "collide_small" else [3360, 1440, 480, 3360])
    _judge(name, got, t)


def test_wide_table_takes_both_paths():
    X, Y, t = mi_cases.case("wide")
    got = _device(X, Y)
    u, H = got[4], mi_cases.SPGEMM_HASH_PRODUCTS
    assert u[mi_cases.WIDE_HOT] > H and (u > H).sum() >= 1 and (u <= H).sum() > 1000
    _judge("wide", got, t)
    # dropping one entry of the hot row would move mi by more than its bound - and row_pi by an integer
    C = t["C"]
    hot = mi_cases.WIDE_HOT
    assert C.indptr[hot + 1] - C.indptr[hot] > 5000


def test_features_that_are_not_the_labels():
    X, Y, t = mi_cases.case("rect")
    assert X.shape[1] != Y.shape[1]
    _judge("rect", _device(X, Y), t)


@pytest.mark.parametrize("name", ["holes", "single_cell"])
def test_degenerate_tables(name):
    X, Y, t = mi_cases.case(name)
    got = _device(X, Y)
    _judge(name, got, t)
    if name == "holes":
        assert got[3][20] == 0 and got[2][20] == 0.0 and got[3][49] == 0 and got[2][49] == 0.0      # pi_i = 0: zeros, no NaN
    else:
        assert got[1] == 6 and got[0] == 0.0 and np.count_nonzero(got[3]) == 1


def test_all_empty_input_launches_nothing():
    from aaerec import _hip, utils
    X, Y = sp.csr_matrix((5, 4)), sp.csr_matrix((5, 7))
    a, b = _hip.DeviceCooc(X.T.tocsr(), DEV), _hip.DeviceCooc(Y, DEV)
    mi, T, s1, pi = _hip.mutual_info_i32(a, b)
    assert mi == 0.0 and T == 0 and s1.shape == (4,) and not s1.any() and not pi.any()
    assert utils.mutual_info(X, Y, device=DEV) == 0.0
    # entries on one side only
    a = _hip.DeviceCooc(sp.csr_matrix(np.ones((4, 5))), DEV)
    assert _hip.mutual_info_i32(a, b)[:2] == (0.0, 0)
    # entries on both sides that never meet: the kernels run and find an empty table
    a = _hip.DeviceCooc(sp.csr_matrix(([2.0], ([1], [0])), shape=(4, 5)), DEV)
    b = _hip.DeviceCooc(sp.csr_matrix(([3.0], ([4], [2])), shape=(5, 7)), DEV)
    mi, T, s1, pi = _hip.mutual_info_i32(a, b)
    assert mi == 0.0 and T == 0 and not s1.any() and not pi.any()


def test_independent_features_and_labels():
    X, Y, t = mi_cases.case("identical")
    got = _device(X, Y)
    _judge("identical", got, t)
    assert 0.0 <= got[0] <= t["mi_bound"]                       # the true mutual information is 0


def test_same_bits_twice():
    import torch
    from aaerec import _hip
    X, Y, _ = mi_cases.case("wide")
    a, b = _hip.cooc_transpose(_hip.DeviceCooc(X, DEV)), _hip.DeviceCooc(Y, DEV)
    one, two = _hip.mutual_info_i32(a, b), _hip.mutual_info_i32(a, b)
    assert one[1] == two[1] > 0
    assert np.float64(one[0]).tobytes() == np.float64(two[0]).tobytes()
    assert torch.equal(one[2].view(torch.int64), two[2].view(torch.int64)) and torch.equal(one[3], two[3])


def test_compute_mutual_info_on_the_device():
    from scipy.stats import entropy
    from aaerec import utils
    X, Y, t = mi_cases.case("small")
    bags = mi_cases.bags_of(Y)
    h = float(entropy(np.asarray(Y.sum(0)).ravel()))
    for normalize in (False, True):
        host = utils.compute_mutual_info(bags, normalize=normalize)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="mutual_info")     # the device takes these operands: no fall-back
            dev = utils.compute_mutual_info(bags, normalize=normalize, device=DEV)
        # normalised: both sides divide by the same entropy, and each quotient is rounded once
        bound = t["mi_bound"] / h + 2 * mi_cases.U * host if normalize else t["mi_bound"]
        print("normalize", normalize, "host", repr(host), "device", repr(dev), "|diff|", abs(dev - host), "bound", bound)
        assert host == (t["mi"] / h if normalize else t["mi"])
        assert dev > 0.0 and abs(dev - host) <= bound
    # a condition imposed on the labels arrives as COO and goes to the device all the same
    from aaerec.condition import ConditionList, CountCondition
    _, Yr, _ = mi_cases.case("rect")
    titles = ["w%d w%d common" % (d % 5, d % 3) for d in range(Yr.shape[0])]
    bags = mi_cases.bags_of(Yr, titles)
    Xr = mi_cases.canon(sp.hstack([Yr, CountCondition().fit_transform(titles)]).tocsr().astype(np.float64))
    tr = mi_cases.truth(Xr, Yr)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="mutual_info")
        dev = utils.compute_mutual_info(bags, conditions=ConditionList([("title", CountCondition())]), normalize=False, device=DEV)
    assert abs(dev - tr["mi"]) <= tr["mi_bound"] and dev != 0.0


def test_fractional_features_warn_and_return_the_hosts_bits():
    from aaerec import utils
    X, Y, _ = mi_cases.case("rect")
    half = X.copy()
    half.data[::7] = 0.5
    host = utils.mutual_info(half, Y)
    with pytest.warns(UserWarning, match="fractional"):
        dev = utils.mutual_info(half, Y, device=DEV)
    assert np.float64(dev).tobytes() == np.float64(host).tobytes()
    with pytest.warns(UserWarning, match="dense"):
        assert utils.mutual_info(X.toarray(), Y, device=DEV) == utils.mutual_info(X.toarray(), Y)


def test_bad_arguments_are_refused_before_the_device():
    import ctypes as C
    from aaerec import _hip
    X, Y, _ = mi_cases.case("small")
    a, b = _hip.DeviceCooc(X.T.tocsr(), DEV), _hip.DeviceCooc(Y, DEV)
    with pytest.raises(ValueError):
        _hip.mutual_info_i32(b, b)                              # [40 x 300] . [40 x 300]
    with pytest.raises(ValueError):
        _hip.mutual_info_i32(a, a)
    lib = _hip.load_library()
    sa, sb = a.struct(), b.struct()
    u = _hip.spgemm_bound(a, b)
    buf = _hip.upload(np.zeros(400, dtype=np.int64), DEV)
    p = _hip._ptr
    assert lib.aae_mi_i32_marginals(C.byref(sa), C.byref(sb), 40, 300, p(buf), None, p(buf), None) != 0
    assert lib.aae_mi_i32_marginals(C.byref(sa), C.byref(sb), 41, 300, p(buf), p(buf), p(buf), None) != 0       # p > rows of B
    assert lib.aae_mi_i32_marginals(C.byref(sa), C.byref(sb), 40, -1, p(buf), p(buf), p(buf), None) != 0
    assert lib.aae_mi_i32_rows(C.byref(sa), C.byref(sb), 300, p(u), None, p(buf), p(buf), None) != 0
    assert lib.aae_mi_i32_rows(None, C.byref(sb), 300, p(u), p(buf), p(buf), p(buf), None) != 0
    assert lib.aae_mi_i32_finish(-1, p(buf), p(buf), p(buf), None) != 0
    assert lib.aae_mi_i32_finish(300, p(buf), p(buf), None, None) != 0
    assert lib.aae_mi_i32_finish(300, p(buf), p(buf), C.c_void_p(buf.data_ptr() + 4), None) != 0                # misaligned out
    assert b"aae_mi_i32_finish" in lib.aae_last_error()
