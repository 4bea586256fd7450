"""Shared by tests/test_svdfit_cpu.py and tests/test_svdfit_gpu.py: the fit cases of SVDRecommender(fit="device"), the host
emulations of scikit-learn's randomized SVD as TruncatedSVD calls it, and the quantities a fit is judged by.

`emulate(A, dims, seed, dtype)` is scikit-learn 1.7's TruncatedSVD.fit written out in numpy / scipy: M = A or A^T
(transpose="auto"), Omega = check_random_state(seed).normal(size=(M.shape[1], l)), n_iter = 5 rounds of the LU normaliser
("auto" with n_iter > 2), the closing QR, B = Q^T M, scipy's gesdd, un-transpose, truncate, svd_flip(u_based_decision=False).
  float64   must reproduce TruncatedSVD(dims, random_state=seed) with difference 0.0 (test_svdfit_cpu.py): it pins the algorithm
            and the Omega draw the device fit shares.
  float32   the same steps with every array - A, Omega, the products, LU, QR, B and its SVD - in float32: the reference run in
            the device's precision.  Its deviation d32 from scikit-learn's float64 fit sizes the bound the device is held to
            (8 * d32 per quantity: the device uses another normaliser (QR) and another summation order).

Quantities (`deviations`): max_i |sigma^_i - sigma_i| / sigma_1; the reconstruction residual ||A||_F^2 - ||A V^T||_F^2 (float64
on the host) relative to scikit-learn's; max |V V^T - I|.  components_ are NOT compared element by element: neighbouring singular
values of these matrices are closer than 2e-3 sigma_1 and their vectors rotate freely within that gap."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from sklearn.decomposition import TruncatedSVD
from sklearn.utils import check_random_state
from sklearn.utils.extmath import svd_flip

N_ITER, N_OVERSAMPLES = 5, 10          # TruncatedSVD's defaults: what the reference's drivers run
FACTOR = 8.0                           # the device may deviate from scikit-learn's fit by FACTOR * d32
# name: (rows, columns, dims, random_state)
BAG_CASES = {"wide_300x500": (300, 500, 16, 11),        # the transposed branch (samples < features)
             "odd_700x257": (700, 257, 33, 12),         # untransposed, odd sizes, l = 43 is no multiple of 4
             "tall_2000x1500": (2000, 1500, 100, 13)}   # a larger untransposed case
TITLE_CASE = "titles_400x(230+words)"                   # bags plus a tf-idf title block: float values
CASES = tuple(BAG_CASES) + (TITLE_CASE,)
TITLE_DIMS, TITLE_SEED = 24, 14


def bag_matrix(rows, cols, seed):
    """0/1 bags of 2-12 items per row, the columns drawn with a Zipf-like popularity (p_j ~ 1 / (j + 1)), float64 CSR."""
    r = np.random.default_rng(seed)
    p = 1.0 / (1.0 + np.arange(cols))
    p /= p.sum()
    ip, idx = [0], []
    for _ in range(rows):
        ids = np.sort(r.choice(cols, size=int(r.integers(2, 13)), replace=False, p=p))
        idx.append(ids)
        ip.append(ip[-1] + ids.size)
    idx = np.concatenate(idx)
    return sp.csr_matrix((np.ones(idx.size), idx, np.asarray(ip)), shape=(rows, cols))


_WORDS = ["graph", "neural", "sparse", "matrix", "kernel", "model", "ranking", "music", "paper", "citation", "tag", "learning",
          "deep", "random", "survey", "fast", "adversarial", "autoencoder", "item", "user", "title", "network", "method", "data",
          "analysis", "large", "scale", "text", "code", "search"]


def titled_bags(rows=400, cols=230, seed=TITLE_SEED):
    """(X, titles): a bag matrix and one title of 2-6 words per row."""
    r = np.random.default_rng(seed + 1000)
    titles = [" ".join(r.choice(_WORDS, size=int(r.integers(2, 7)))) for _ in range(rows)]
    return bag_matrix(rows, cols, seed), titles


def emulate(A, dims, seed, dtype, n_iter=N_ITER, n_oversamples=N_OVERSAMPLES):
    """(components [dims, features], singular values [dims]) in `dtype`: the module docstring's algorithm."""
    A = sp.csr_matrix(A, dtype=dtype)
    n, m = A.shape
    transpose = n < m
    M = A.T.tocsr() if transpose else A
    l = dims + n_oversamples
    Q = check_random_state(seed).normal(size=(M.shape[1], l)).astype(dtype, copy=False)
    for _ in range(n_iter):
        Q, _ = scipy.linalg.lu(M @ Q, permute_l=True, check_finite=False)
        Q, _ = scipy.linalg.lu(M.T @ Q, permute_l=True, check_finite=False)
    Q, _ = scipy.linalg.qr(M @ Q, mode="economic", check_finite=False)
    B = Q.T @ M
    Uhat, s, Vt = scipy.linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    assert Q.dtype == B.dtype == s.dtype == np.dtype(dtype)
    U, s, Vt = (Vt[:dims].T, s[:dims], U[:, :dims].T) if transpose else (U[:, :dims], s[:dims], Vt[:dims])
    U, Vt = svd_flip(U, Vt, u_based_decision=False)
    return Vt, s


def quantities(A, components, sigma, sk_sigma):
    """(sigma deviation relative to sigma_1, residual ||A||_F^2 - ||A V^T||_F^2, max |V V^T - I|), all in float64."""
    A = sp.csr_matrix(A, dtype=np.float64)
    V = np.asarray(components, dtype=np.float64)
    dev = float(np.abs(np.asarray(sigma, dtype=np.float64) - sk_sigma).max() / sk_sigma[0])
    resid = float(A.multiply(A).sum() - np.square(A @ V.T).sum())
    orth = float(np.abs(V @ V.T - np.eye(V.shape[0])).max())
    return dev, resid, orth


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything a test needs of one case, computed once: the matrix (and titles), scikit-learn's float64 fit, the exact
    optimum of the residual, both emulations, d32 and the bounds."""
    if name == TITLE_CASE:
        from sklearn.feature_extraction.text import TfidfVectorizer
        X, titles = titled_bags()
        A = sp.hstack([X, TfidfVectorizer(input="content").fit_transform(titles)]).tocsr()
        dims, seed = TITLE_DIMS, TITLE_SEED
    else:
        rows, cols, dims, seed = BAG_CASES[name]
        X, titles = bag_matrix(rows, cols, seed), None
        A = X
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    sk = TruncatedSVD(dims, random_state=seed).fit(A)
    exact = np.linalg.svd(A.toarray(), compute_uv=False)
    optimum = float(np.square(exact[dims:]).sum())              # the residual no rank-dims V can go below
    V64, s64 = emulate(A, dims, seed, np.float64)
    V32, s32 = emulate(A, dims, seed, np.float32)
    _, sk_resid, _ = quantities(A, sk.components_, sk.singular_values_, sk.singular_values_)
    dev32, resid32, orth32 = quantities(A, V32, s32, sk.singular_values_)
    d32 = dict(sigma=dev32, resid=abs(resid32 - sk_resid) / sk_resid, orth=orth32)
    return dict(name=name, X=X, titles=titles, A=A, dims=dims, seed=seed, sk=sk, sk_resid=sk_resid, optimum=optimum,
                emu64=(V64, s64), emu32=(V32, s32), d32=d32, bound={q: FACTOR * v for q, v in d32.items()})


def deviations(c, components, sigma):
    """The three deviations of a fit from scikit-learn's float64 fit of case c, and its residual."""
    dev, resid, orth = quantities(c["A"], components, sigma, c["sk"].singular_values_)
    return dict(sigma=dev, resid=abs(resid - c["sk_resid"]) / c["sk_resid"], orth=orth), resid
