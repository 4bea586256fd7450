"""The mutual information of a dataset (aaerec/utils.py) without a GPU: the host route against scikit-learn and against the
fixture recorded from the reference, the guard that admits operands to the device (`device_mi_ok`), and the arithmetic the
device route rests on - the marginal identities and the per-row form - restated in float64 on the host and held to the bounds
of tests/mi_cases.py."""
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.stats import entropy
from sklearn.metrics import mutual_info_score

import mi_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_host_route_is_scikit_learn_bit_for_bit():
    from aaerec import utils
    for name in ("small", "rect", "holes"):
        X, Y, _ = mi_cases.case(name)
        want = mutual_info_score(None, None, contingency=X.T @ Y)
        assert utils.mutual_info(X, Y) == want and utils.mutual_info(X, Y, device=None) == want


def test_normalize_divides_by_the_entropy_of_the_features(capsys):
    from aaerec import utils
    from aaerec.condition import ConditionList, CountCondition
    _, Y, _ = mi_cases.case("rect")
    titles = ["w%d w%d common" % (d % 5, d % 3) for d in range(Y.shape[0])]
    bags = mi_cases.bags_of(Y, titles)
    assert (bags.tocsr() != Y).nnz == 0
    want = mutual_info_score(None, None, contingency=Y.T @ Y)
    assert utils.compute_mutual_info(bags, normalize=False) == want
    assert utils.compute_mutual_info(bags, normalize=True) == want / entropy(np.asarray(Y.sum(0)).ravel())
    # the condition imposed on the labels: X = [Y | counts]
    cond = ConditionList([("title", CountCondition())])
    W = CountCondition().fit_transform(titles)
    X = sp.hstack([Y, W])
    got = utils.compute_mutual_info(bags, conditions=cond, normalize=True)
    assert got == mutual_info_score(None, None, contingency=X.T @ Y) / entropy(np.asarray(X.sum(0)).ravel())
    # the condition alone
    cond = ConditionList([("title", CountCondition())])
    got = utils.compute_mutual_info(bags, conditions=cond, include_labels=False, normalize=False)
    assert got == mutual_info_score(None, None, contingency=W.T @ Y)
    assert all(line.startswith("[MI]") for line in capsys.readouterr().out.splitlines())
    with pytest.raises(AssertionError):
        utils.compute_mutual_info(bags, conditions=None, include_labels=False)
    with pytest.raises(AssertionError):
        utils.compute_mutual_info(Y)


def test_reproduces_the_reference_in_all_three_input_forms():
    from aaerec import utils
    from aaerec.condition import ConditionList, CountCondition
    from aaerec.datasets import BagsWithVocab
    z = np.load(os.path.join(GOLDEN, "mutual_info.npz"))
    ip, tokens, n = z["bag_indptr"], z["bag_tokens"], int(z["n_items"])
    owners = ["d%d" % d for d in range(len(ip) - 1)]
    bags = BagsWithVocab([tokens[ip[d]:ip[d + 1]].tolist() for d in range(len(owners))], {"i%d" % j: j for j in range(n)},
                         owners=owners, attributes={"title": dict(zip(owners, z["titles"].tolist()))})
    assert z["forms"].tolist() == ["labels", "imposed", "conditions"]
    for form, with_cond, include_labels in (("labels", False, True), ("imposed", True, True), ("conditions", True, False)):
        for normalize in (False, True):
            cond = ConditionList([("title", CountCondition())]) if with_cond else None
            got = utils.compute_mutual_info(bags, conditions=cond, include_labels=include_labels, normalize=normalize)
            want = float(z["mi.%s.%s" % (form, "normalized" if normalize else "raw")])
            assert want > 0.2 and abs(got - want) <= 1e-12 * want, (form, normalize, got, want)


def test_device_mi_ok_truth_table():
    from aaerec.utils import device_mi_ok
    X, Y, _ = mi_cases.case("rect")
    assert device_mi_ok(X, Y) == (True, "") and device_mi_ok(Y, Y) == (True, "")
    assert device_mi_ok(X.astype(np.int64), Y.astype(np.int32)) == (True, "")
    assert device_mi_ok(sp.csr_matrix((5, 3)), sp.csr_matrix((5, 4))) == (True, "")

    def refused(A, B, word):
        ok, why = device_mi_ok(A, B)
        assert not ok and word in why, (ok, why)

    def with_value(v, at=3):
        M = X.copy()
        M.data[at] = v
        return M
    refused(with_value(0.5), Y, "fractional")
    refused(with_value(0.0), Y, "zero")
    negative = Y.copy()
    negative.data[5] = -2.0
    refused(X, negative, "negative")
    refused(X.astype(np.float32), Y, "float32")
    # unsorted columns, duplicate columns
    r = int(np.flatnonzero(np.diff(Y.indptr) >= 2)[0])
    lo = Y.indptr[r]
    swapped = sp.csr_matrix((Y.data.copy(), Y.indices.copy(), Y.indptr.copy()), shape=Y.shape)
    swapped.indices[[lo, lo + 1]] = swapped.indices[[lo + 1, lo]]
    refused(X, swapped, "unsorted")
    doubled = sp.csr_matrix((Y.data.copy(), Y.indices.copy(), Y.indptr.copy()), shape=Y.shape)
    doubled.indices[lo + 1] = doubled.indices[lo]
    refused(doubled, Y, "duplicate")
    refused(X.toarray(), Y, "dense")
    refused(X, np.asarray(Y.todense()), "dense")
    refused(X.tocoo(), Y, "CSR")
    refused(X[:-1], Y, "rows")
    # the Cauchy-Schwarz product: (sum x^2)(sum y^2) = 2^62 is refused, one document fewer is accepted
    big = float(2 ** 15)
    col = sp.csr_matrix(np.full((2, 1), big))                   # sum of squares 2 * 2^30 = 2^31
    assert device_mi_ok(col, col)[0] is False and "2^62" in device_mi_ok(col, col)[1]
    assert device_mi_ok(col, sp.csr_matrix(np.array([[big], [big - 1.0]])))[0] is True
    refused(sp.csr_matrix(np.full((1, 1), 2.0 ** 16)), col[:1], "2^62")
    # T >= 2^53 while every entry of the table stays small: 2^17 documents x 2^18 features x 2^18 labels of ones is too large to
    # build; instead rows whose sums multiply up - one document with 2^14 features of 2^13 and 2^14 labels of 2^12
    wide_x = sp.csr_matrix(np.full((1, 2 ** 14), 2.0 ** 13))
    wide_y = sp.csr_matrix(np.full((1, 2 ** 14), 2.0 ** 12))
    assert 2 ** 27 * 2 ** 26 == 2 ** 53                         # T exactly at the limit; every c_ij = 2^25
    refused(wide_x, wide_y, "2^53")
    assert device_mi_ok(wide_x, sp.csr_matrix(np.full((1, 2 ** 14 - 1), 2.0 ** 12)))[0] is True


def test_marginal_identities_hold_against_the_table():
    for name in mi_cases.CASES:
        X, Y, t = mi_cases.case(name)
        Xi, Yi = sp.csr_matrix(X, dtype=np.int64), sp.csr_matrix(Y, dtype=np.int64)
        a, b = np.asarray(Xi.sum(axis=1)).ravel(), np.asarray(Yi.sum(axis=1)).ravel()
        np.testing.assert_array_equal(Yi.T @ a, t["pj"])
        np.testing.assert_array_equal(Xi.T @ b, t["pi"])
        assert int(a @ b) == t["T"]


@pytest.mark.parametrize("name", mi_cases.CASES)
def test_per_row_form_in_float64_is_inside_the_bounds(name):
    """The device's arithmetic restated with numpy: what the GPU tests ask of the kernels holds for the formula itself."""
    X, Y, t = mi_cases.case(name)
    mi, s1, pi, T = mi_cases.per_row_form(X, Y)
    assert T == t["T"]
    np.testing.assert_array_equal(pi, t["pi"])
    assert np.all(np.abs(s1 - t["row_s1"]) <= t["s1_bound"])
    assert abs(mi - t["mi"]) <= t["mi_bound"], (mi, t["mi"], t["mi_bound"])
    assert mi >= 0.0 and np.isfinite(mi)


def test_case_shapes_reach_the_branches_they_are_named_for():
    H, tile = mi_cases.SPGEMM_HASH_PRODUCTS, mi_cases.COOC_TILE

    def bound(name):
        X, Y, _ = mi_cases.case(name)
        return np.asarray(X.T.astype(bool).astype(np.int64) @ np.diff(Y.indptr)).ravel()      # products per row of X^T . Y
    assert bound("small").max() <= H
    assert bound("bin_edge").tolist() == [H, H + 1]
    assert bound("collide_small").tolist() == [28, 12, 4, 28] and bound("collide").tolist() == [3360, 1440, 480, 3360]
    u = bound("wide")
    X, _, t = mi_cases.case("wide")
    hot = mi_cases.WIDE_HOT
    assert X.shape[1] == tile + 5 and u[hot] > H and X.T.tocsr().indptr[hot + 1] - X.T.tocsr().indptr[hot] == 700 > mi_cases.SPGEMM_STAGE
    assert (u <= H).sum() > 1000
    C = t["C"]
    row = C.indices[C.indptr[hot]:C.indptr[hot + 1]]
    assert {0, tile - 1, tile, tile + 4} <= set(row.tolist())
    X, Y, t = mi_cases.case("rect")
    assert X.shape == (60, 237) and Y.shape == (60, 200)
    _, _, t = mi_cases.case("holes")
    assert t["pi"][20] == 0 and t["pi"][49] == 0 and t["pi"][:20].max() > 0 and t["pi"][21:49].max() > 0
    _, _, t = mi_cases.case("identical")
    assert t["mi"] <= t["mi_bound"]                             # scikit-learn's own value of a true 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert mi_cases.case("single_cell")[2]["T"] == 6
