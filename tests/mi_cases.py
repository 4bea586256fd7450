"""Shared by tests/test_mutinfo_cpu.py and tests/test_mutinfo_gpu.py: the (X, Y) cases of the mutual information of a dataset
(aaerec/utils.py, csrc/mutinfo.h), the host truth of each and the bounds the device is held to.

Host truth is scipy's int64 C = X^T Y and scikit-learn's mutual_info_score(contingency=C).
  T, row_pi   compared by EQUALITY with C.sum() and C.sum(1).
  row_s1[i]   against the float64 sum_j c_ij (ln c_ij - ln pj_j) within 2^-53 (nnz_i + 64) sum_j c_ij (|ln c_ij| + ln pj_j).
  mi          against scikit-learn's value within 2^-53 (nnz + 64) S + nnz 2^-52, S = sum (c/T)(|ln c| + ln T + ln pi + ln pj):
              the any-order summation bound (n - 1) u sum |t| plus 64 u for a term's four logarithms and five operations; the
              second summand covers scikit-learn's zeroing of terms below epsilon.
Shapes are the smallest that reach each branch (those of tests/test_cooc_build_gpu.py): rows on either side of the bin edge
SPGEMM_HASH_PRODUCTS, columns that collide in the hash table at every capacity it takes, a table wider than one LDS tile with
entries at the tile's first and last cells, a row of X^T longer than one staging piece, features that are not the labels."""
import functools

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
# (include/aaerec_hip.h; restated so that the CPU tests need no library)
COOC_TILE, SPGEMM_HASH_PRODUCTS, SPGEMM_STAGE = 16384, 4096, 512


def canon(M):
    M = sp.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return M


def docs(rng, n_docs, items, lo, hi, values=(1,)):
    """n_docs rows of lo..hi distinct items each, the values drawn from `values`: canonical float64 CSR."""
    lens = rng.integers(lo, hi + 1, size=n_docs)
    rows = np.repeat(np.arange(n_docs), lens)
    cols = np.concatenate([rng.choice(items, size=int(n), replace=False) for n in lens])
    return canon(sp.csr_matrix((rng.choice(values, size=cols.size).astype(np.float64), (rows, cols)), shape=(n_docs, items)))


def _small():
    X = docs(np.random.default_rng(1), 40, 300, 1, 6)
    return X, X


def _bin_edge():
    """X^T has two rows: u = SPGEMM_HASH_PRODUCTS (the last hash row) and one more (the first tile row)."""
    r = np.random.default_rng(4)
    per = 64
    k, n = SPGEMM_HASH_PRODUCTS // per, 5000
    Y = sp.vstack([docs(r, k, n, per, per, values=(1, 2)), sp.csr_matrix(([1.0], ([0], [n - 1])), shape=(1, n))]).tocsr()
    A = sp.csr_matrix(np.vstack([np.r_[np.ones(k), 0], np.ones(k + 1)]))
    return canon(A.T), canon(Y)


def _collide_blocks():
    cap = 2 * SPGEMM_HASH_PRODUCTS
    n = 3 * cap + 10
    rows = [[c + k * cap for k in range(4)] for c in range(6)] + [[7 + k * cap for k in range(3)] + [3 * cap + 9]]
    assert all(len({j % cap for j in r}) <= 2 for r in rows)
    B = sp.csr_matrix((np.arange(1, 29, dtype=np.float64), np.concatenate(rows), 4 * np.arange(8)), shape=(7, n))
    A = sp.csr_matrix(np.array([[1, 1, 1, 1, 1, 1, 1], [0, 2, 0, 3, 0, 1, 0], [5, 0, 0, 0, 0, 0, 0], [1, 2, 3, 1, 2, 3, 1]], dtype=np.float64))
    return A, B


def _collide_small():
    """Label columns congruent modulo the hash table's largest capacity, and so modulo every smaller one a row's table takes:
    within a row of Y every insert behind the first collides.  u = 28, 12, 4, 28: the smallest table, 64 slots."""
    A, B = _collide_blocks()
    return canon(A.T), canon(B)


def _collide():
    """The same colliding labels in 840 documents: u = 3360, 1440, 480, 3360 - tables of 8192, 4096 and 1024 slots."""
    A, B = _collide_blocks()
    X = sp.vstack([A.T.tocsr()] * 120).tocsr()
    X.data[::3] += 1.0
    return canon(X), canon(sp.vstack([B] * 120))


WIDE_HOT = 4321


def _wide():
    """n = COOC_TILE + 5 items, 700 documents of about 20 with values in {1, 2, 3}; item WIDE_HOT is in every document: its row of
    X^T exceeds SPGEMM_STAGE and goes the tile path; entries at the tile's first and last cells and in the 5-column tail."""
    n = COOC_TILE + 5
    X = docs(np.random.default_rng(2), 700, n, 17, 22, values=(1, 2, 3)).tolil()
    X[:, WIDE_HOT] = 2
    for d, c in enumerate((0, COOC_TILE - 1, COOC_TILE, n - 1)):
        X[d, c] = 3
        X[d + 10, c] = 1
    X = canon(X.tocsr())
    return X, X


def _rect():
    """X = [Y | 37 count columns] over 60 documents x 200 labels: m != n, the features are not the labels."""
    r = np.random.default_rng(8)
    Y = docs(r, 60, 200, 1, 8, values=(1, 2, 3))
    W = docs(r, 60, 37, 0, 5)
    return canon(sp.hstack([Y, W]).tocsr()), Y


def _holes():
    """Items no document holds (pi_i = 0 in the middle of the table) and documents without items."""
    X = docs(np.random.default_rng(5), 30, 50, 1, 5).tolil()
    X[7, :] = 0
    X[19, :] = 0
    X[:, 20] = 0
    X[:, 49] = 0
    X = canon(X.tocsr())
    X.eliminate_zeros()
    return X, X


def _single_cell():
    X = sp.csr_matrix(([3.0], ([2], [1])), shape=(4, 5))
    Y = sp.csr_matrix(([2.0], ([2], [6])), shape=(4, 9))
    return X, Y


def _identical():
    """Seven identical documents: features and labels are independent, the true mutual information is 0."""
    row = np.zeros(23)
    row[[0, 3, 4, 11, 22]] = [1, 2, 1, 3, 1]
    X = canon(sp.csr_matrix(np.tile(row, (7, 1))))
    return X, X


BUILDERS = {"small": _small, "bin_edge": _bin_edge, "collide_small": _collide_small, "collide": _collide, "wide": _wide, "rect": _rect, "holes": _holes,
            "single_cell": _single_cell, "identical": _identical}
CASES = tuple(BUILDERS)


def truth(X, Y):
    """Everything a result is judged by, from scipy's int64 contingency table: T, row_pi (int64), pj, the float64 row_s1 with
    its bound per row, scikit-learn's mi and the bound on mi."""
    from sklearn.metrics import mutual_info_score
    C = canon(sp.csr_matrix(X, dtype=np.int64).T @ sp.csr_matrix(Y, dtype=np.int64))
    assert C.dtype == np.int64 and (C.nnz == 0 or (C.data.min() > 0 and C.data.max() < 2 ** 31))
    m = C.shape[0]
    c = C.data.astype(np.float64)
    rows = np.repeat(np.arange(m), np.diff(C.indptr))
    pi = np.asarray(C.sum(axis=1)).ravel().astype(np.int64)
    pj = np.asarray(C.sum(axis=0)).ravel().astype(np.int64)
    T = int(C.sum())
    ln_c, ln_pj, ln_pi = np.log(c), np.log(pj[C.indices].astype(np.float64)), np.log(pi[rows].astype(np.float64))
    row_s1 = np.bincount(rows, weights=c * (ln_c - ln_pj), minlength=m)
    row_nnz = np.diff(C.indptr)
    s1_bound = U * (row_nnz + 64) * np.bincount(rows, weights=c * (np.abs(ln_c) + ln_pj), minlength=m)
    S = float(np.sum(c / T * (np.abs(ln_c) + np.log(T) + ln_pi + ln_pj))) if T else 0.0
    mi = float(mutual_info_score(None, None, contingency=sp.csr_matrix(X).T @ sp.csr_matrix(Y))) if T else 0.0
    return dict(C=C, T=T, pi=pi, pj=pj, row_s1=row_s1, s1_bound=s1_bound, mi=mi, mi_bound=U * (C.nnz + 64) * S + C.nnz * 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, Y, truth) of a case, computed once and shared; the matrices are not to be written to."""
    X, Y = BUILDERS[name]()
    return X, Y, truth(X, Y)


def per_row_form(X, Y):
    """(mi, row_s1, row_pi, T) by the device's arithmetic restated on the host: the marginals from the operands' own entries
    (pj = Y^T rowsum(X), pi = X^T rowsum(Y)), MI = (1/T) sum_i [S1_i + pi_i (ln T - ln pi_i)], everything float64."""
    Xi, Yi = sp.csr_matrix(X, dtype=np.int64), sp.csr_matrix(Y, dtype=np.int64)
    pj = np.asarray(Yi.T @ np.asarray(Xi.sum(axis=1)).ravel()).ravel()
    pi = np.asarray(Xi.T @ np.asarray(Yi.sum(axis=1)).ravel()).ravel()
    C = canon(Xi.T @ Yi)
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    c = C.data.astype(np.float64)
    s1 = np.bincount(rows, weights=c * (np.log(c) - np.log(pj[C.indices].astype(np.float64))), minlength=C.shape[0])
    T = int(pi.sum())
    live = pi > 0
    terms = s1[live] + pi[live] * (np.log(float(T)) - np.log(pi[live].astype(np.float64))) if T else np.zeros(0)
    return (max(float(terms.sum()) / T, 0.0) if T else 0.0), s1, pi, T


def bags_of(Y, titles=None):
    """A BagsWithVocab whose tocsr() is the 0/1 (or count) matrix Y, with one title per document when given."""
    from aaerec.datasets import BagsWithVocab
    Y = sp.csr_matrix(Y)
    data = [np.repeat(Y.indices[Y.indptr[d]:Y.indptr[d + 1]], Y.data[Y.indptr[d]:Y.indptr[d + 1]].astype(int)).tolist()
            for d in range(Y.shape[0])]
    owners = ["d%d" % d for d in range(Y.shape[0])]
    attrs = {"title": dict(zip(owners, titles))} if titles is not None else None
    return BagsWithVocab(data, {"i%d" % j: j for j in range(Y.shape[1])}, owners=owners, attributes=attrs)
