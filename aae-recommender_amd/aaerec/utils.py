"""Dataset statistics: the mutual information between a dataset's features and its labels (the counterpart of the reference's
aaerec/utils.py, whose tables are the numbers it publishes per dataset).

The statistic is scikit-learn's mutual_info_score of the contingency table C = X^T Y [features, labels].  On the host
(`device=None`, the default) it is scipy's product followed by that call.  With a device the table is never stored:
csrc/mutinfo.h accumulates one row of it at a time in LDS with the exact int32 product's own code (csrc/spgemm.h) and reduces
it on the spot,

    MI = (1/T) sum_i [ S1_i + pi_i (ln T - ln pi_i) ],   S1_i = sum_j c_ij (ln c_ij - ln pj_j),

with the marginals pi, pj and T whole numbers in int64 and every logarithm and sum in float64 - the same bits every run.  The
device takes whole-number data only (`device_mi_ok`): dense condition blocks such as word embeddings, fractional tf-idf weights
and negative values go the host route with a warning that says why.  The entropy that normalises the result is O(nnz(X)) work
over a vector of `features` numbers and stays on the host."""
import warnings

import numpy as np
import scipy.sparse as sp

from .condition import ConditionList
from .cooc import INT32_LIMIT, _EXACT_DTYPES, _canonical
from .datasets import BagsWithVocab

_EXACT_DOUBLE = 1 << 53                 # whole numbers below it are exact in float64


def _say(*words):
    print("[MI]", *words)


def _whole_positive(M, name):
    """None, or why the stored values of the CSR matrix M are not strictly positive whole numbers of an exact type."""
    data = np.asarray(M.data)
    if data.dtype not in _EXACT_DTYPES:
        return "{} holds {} values: float64 or 32- / 64-bit integers only".format(name, data.dtype)
    if M.nnz and not np.all(data > 0):
        return "{} stores a zero or a negative value".format(name)
    if M.nnz and not np.all(data == np.rint(data)):
        return "{} stores a fractional value".format(name)
    return None


def _max_column_square_sum(M):
    """max_j sum_d M_dj^2 as a Python int (the caller has checked that every square is exact), 0 without entries."""
    if not M.nnz:
        return 0
    sq = np.bincount(M.indices, weights=np.asarray(M.data, dtype=np.float64) ** 2, minlength=M.shape[1])
    return int(sq.max())


def device_mi_ok(X, Y):
    """(ok, why): whether the device computes the mutual information of C = X^T Y as the host does, and the reason when not.
    ok when both are canonical scipy CSR matrices (columns ascending, no duplicates) with equally many rows and shapes inside
    int32, of float64 or integer type with every stored value a strictly positive whole number - then the pattern of C is
    scipy's - and
      (max_i sum_d x_di^2) (max_j sum_d y_dj^2) < 2^62   every c_ij <= sqrt(sum_d x_di^2 sum_d y_dj^2) < 2^31 (Cauchy-Schwarz),
                                                          and, the terms being positive, so is every partial sum; for X = Y
                                                          this is aaerec.cooc.device_build_ok's rule;
      T = sum_d (sum_i x_di) (sum_j y_dj) < 2^53          T and every marginal below it are exact in float64."""
    for M, name in ((X, "X"), (Y, "Y")):
        if not sp.issparse(M):
            return False, "{} is dense".format(name)
        if M.format != "csr":
            return False, "{} is a sparse {} matrix, not CSR".format(name, M.format)
    if X.shape[0] != Y.shape[0]:
        return False, "X has {} rows and Y {}".format(X.shape[0], Y.shape[0])
    if max(X.shape + Y.shape) >= INT32_LIMIT:
        return False, "a shape leaves int32"
    for M, name in ((X, "X"), (Y, "Y")):
        if not _canonical(M):
            return False, "{} has unsorted or duplicate columns in a row".format(name)
        why = _whole_positive(M, name)
        if why:
            return False, why
    if not X.nnz or not Y.nnz:
        return True, ""
    if max(float(X.data.max()), float(Y.data.max())) ** 2 >= 2.0 ** 31:      # (every square and sum below is then exact)
        return False, "a stored value reaches 2^15.5: the Cauchy-Schwarz product reaches 2^62"
    if _max_column_square_sum(X) * _max_column_square_sum(Y) >= 1 << 62:
        return False, "(max_i sum_d x_di^2)(max_j sum_d y_dj^2) reaches 2^62: an entry of the contingency table may leave int32"
    rx = np.asarray(X.sum(axis=1), dtype=np.float64).ravel()                # (exact: below nnz * 2^15.5)
    ry = np.asarray(Y.sum(axis=1), dtype=np.float64).ravel()
    total = float(rx @ ry)                                                  # (relative error below rows * 2^-53 <= 2^-22)
    if total >= 2.0 ** 52:
        if total >= 2.0 ** 54 or sum(int(a) * int(b) for a, b in zip(rx, ry)) >= _EXACT_DOUBLE:
            return False, "the table's total reaches 2^53: its marginals are not exact in float64"
    return True, ""


def mutual_info(X, Y, device=None):
    """Mutual information (base e) between the features X [docs, features] and the labels Y [docs, labels]: scikit-learn's
    mutual_info_score of the contingency table X^T Y.  device=None: scipy's product, then
    mutual_info_score(None, None, contingency=...) - the reference's route, bit for bit.  With a device (e.g. "cuda:0") and
    operands device_mi_ok accepts, X is transposed on the device and the table is reduced row by row without being stored; the
    result is within 2^-53 (nnz + 64) sum (c/T)(|ln c| + ln T + ln pi + ln pj) + nnz 2^-52 of scikit-learn's.  Operands the
    device does not take go the host route with a warning that names why."""
    if device is not None:
        ok, why = device_mi_ok(X, Y)
        if ok:
            from . import _hip
            xt = _hip.cooc_transpose(_hip.DeviceCooc(X, device))           # X^T [features, docs]
            return _hip.mutual_info_i32(xt, _hip.DeviceCooc(Y, device))[0]
        warnings.warn("mutual_info(device={!r}): computing on the host: {}".format(str(device), why))
    from sklearn.metrics import mutual_info_score
    return mutual_info_score(None, None, contingency=X.T @ Y)


def _features(bags, Y, conditions, include_labels):
    """The feature matrix of the three input forms: the labels themselves; the labels with every condition imposed on them;
    the first condition's encoding with the further conditions imposed on it."""
    if not conditions:
        return Y
    assert isinstance(conditions, ConditionList), "conditions must be a ConditionList"
    _say("conditions:", ", ".join(map(str, conditions.keys())))
    fitted = conditions.fit_transform(bags.get_attributes(conditions.keys()))
    if include_labels:
        _say("features = labels with the conditions imposed")
        return conditions.encode_impose(Y, fitted)
    _say("features = condition data alone")
    blocks = conditions.encode(fitted)
    X = blocks[0]
    for cond, block in list(zip(conditions.values(), blocks))[1:]:
        X = cond.impose(X, block)
    return X


def compute_mutual_info(bags, conditions=None, include_labels=True, normalize=True, device=None):
    """Mutual information between the features and the labels of `bags` (a BagsWithVocab), base e.
    conditions      None, or a ConditionList over attributes of the bags' owners
    include_labels  True: the features are the labels, with the conditions (if any) imposed on them; False: the features are
                    the condition data alone (conditions required)
    normalize       divide by the entropy of the features' column sums
    device          None: the host route; a device such as "cuda:0": mutual_info's device route
    Progress goes to stdout behind an "[MI]" tag."""
    assert isinstance(bags, BagsWithVocab), "bags must be a BagsWithVocab: apply a vocabulary first"
    assert conditions or include_labels, "without conditions the labels are the only features: include_labels must be True"
    Y = bags.tocsr()
    _say("labels", Y.shape)
    X = _features(bags, Y, conditions, include_labels)
    _say("features", X.shape)
    if device is not None and sp.issparse(X) and not (X.format == "csr" and _canonical(X)):
        # (a block stacked onto the labels may arrive as COO, and CountVectorizer leaves its columns unsorted within a row:
        #  the same matrix in the layout the device reads - a copy, the labels may be the same object)
        X = sp.csr_matrix(X, copy=True)
        X.sum_duplicates()
        X.sort_indices()
    _say("contingency table", (X.shape[1], Y.shape[1]), "on", "the host" if device is None else device)
    mi = mutual_info(X, Y, device=device)
    _say("mutual information (base e):", mi)
    if normalize:
        from scipy.stats import entropy
        h = entropy(np.asarray(X.sum(0)).ravel())
        _say("entropy of the features:", h)
        mi = mi / h
        _say("normalised mutual information:", mi)
    return mi
