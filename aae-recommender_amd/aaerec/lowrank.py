"""Truncated-SVD baseline with its ranking on the device (the reference's SVDRecommender, svd.py:15-57).

    scores = (X_test V^T) V[:, :n_classes],   V = TruncatedSVD.components_  [dims, features]
    features = items (+ the tf-idf vocabulary of the titles when use_title)

`train` fits scikit-learn's TruncatedSVD where `fit` says - "host": TruncatedSVD.fit, as the reference does; "device": the same
randomized range finder with its sparse products on the device (`SVDRecommender._fit_device`) - and `predict` is the reference's
host route (float64, transform then inverse_transform, sliced to the items).  `predict_topk` / `predict_ranks` are what `Evaluation` asks
for where a recommender offers them: V is uploaded once as one fp32 table Vt [features, dims] (_hip.DeviceLowRank), csrc/lowrank.h
projects the sparse feature rows onto it, the tiled fp32 GEMM of csrc/gemm_f32.h reconstructs the item scores into a
[rows, items] scratch, and the dense kernels of csrc/rank_long.h / rank_full.h rank them there - row-wise min-max scaling with the
known items still in the minimum and maximum, known ITEMS masked (the title columns are features, never candidates), the better
score first, the smaller id at equal scores.  Only [n, k] ids or nnz(truth) ranks cross PCIe.

The device computes in fp32 where the host route computes in float64: scores agree within the bound csrc/lowrank.h states,
and two items closer than that may swap places.  The host answers, from predict() and with the same ordering rule, when
device is None, for a list longer than min(1024, items), for more than 4096 dimensions and for a table that is not finite.

This module is not `aaerec.svd`: that name keeps resolving to the user's checkout of the reference through the package path
(aaerec/__init__.py), as `aaerec.baselines` does beside `aaerec.cooc`.
"""
import time
import warnings

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import torch
from sklearn.decomposition import TruncatedSVD
from sklearn.feature_extraction.text import TfidfVectorizer
from sklearn.utils import check_random_state
from sklearn.utils.extmath import svd_flip
from sklearn.utils.sparsefuncs import mean_variance_axis

from . import _hip, ranking
from .base import Recommender
from .ub import AutoEncoderMixin


def _canonical(M):
    M = sp.csr_matrix(M, dtype=np.float64, copy=True)
    M.sum_duplicates()
    M.sort_indices()
    return M


def _scaled(s, best):
    """The scaled scores of the items `best` of a row: float64, rounded to fp32 once (where they are stored)."""
    span = s.max() - s.min()
    return (s[best] - s.min()) / (span if span > 0 else 1.0)


class SVDRecommender(ranking.ScratchRanker, Recommender, AutoEncoderMixin):
    """SVD baseline, capable of dealing with text.  dims, use_title, tfidf_params and the further keyword arguments
    (TruncatedSVD's) are the reference's.  scratch_bytes: the [rows, items] fp32 scratch of one device call - the rows of a
    predict_topk / predict_ranks call are chunked to it.  device: where Vt lives and the ranking runs; None keeps everything
    on the host.

    fit: where the decomposition is computed.  "host" (the default): TruncatedSVD.fit.  "device": scikit-learn's randomized_svd
    as TruncatedSVD calls it, step for step, with M = A when samples >= features and A^T otherwise and l = dims + n_oversamples:
    Omega is drawn on the host exactly as scikit-learn draws it (check_random_state(random_state).normal(size=(M.shape[1], l)))
    and uploaded as fp32, so a given random_state follows the host fit's path; n_iter rounds of Q <- orth(M Q), Q <- orth(M^T Q),
    then Q <- qr(M Q), both products through _hip.spmm_f32 on CSR(M) and CSR(M^T) (the latter from _hip.csr_transpose), orth =
    torch.linalg.qr(mode="reduced") on the device in fp32; B = (M^T Q)^T [l, M.shape[1]] is downloaded once and decomposed where
    scikit-learn decomposes it (host, float64, scipy.linalg.svd with gesdd); the result is un-transposed, truncated to dims and
    sign-fixed by svd_flip(u_based_decision=False) on the components, as the installed TruncatedSVD does.  EVERY value of
    power_iteration_normalizer ("auto", "LU", "QR", "none") maps to QR here: the normaliser changes the basis of Q, not its
    span, and QR is scikit-learn's own most accurate choice; in fp32 "none" would lose the small singular directions.
    self.svd is left with components_, singular_values_, explained_variance_, explained_variance_ratio_ and n_features_in_.
    The host fit answers instead, with a one-line warning that names the reason, for l > 4096, l beyond the smaller side of the
    matrix, algorithm="arpack", values that are not finite (in float64 or as fp32) and a working set above fit_bytes.
    fit="device" without a device raises.

    fit_bytes: the largest working set of the device fit - two [max(samples, features), l] fp32 buffers and both CSR forms.
    The default, 32 GiB, is four times what the largest setting of the reference's drivers needs (10^6 rows, dims 1000: 2 x 4 GB
    of buffers), which leaves room for torch.linalg.qr's own copy and workspace of one such buffer, and a ninth of the HBM of
    the device the library is built for."""

    FITS = ("host", "device")

    def __init__(self, dims=1000, use_title=False, tfidf_params={}, scratch_bytes=256 << 20, device="cuda:0", fit="host",
                 fit_bytes=32 << 30, **kwargs):
        super().__init__()
        if fit not in self.FITS:
            raise ValueError("fit must be one of {}, not {!r}".format(self.FITS, fit))
        if fit == "device" and device is None:
            raise ValueError('fit="device" needs a device')
        self.fit_on = fit
        self.fit_bytes = int(fit_bytes)
        self.fitted_on = None             # "host" / "device": where the last fit() ran
        self.fit_seconds = None           # set to {} by a caller who wants the device fit's phases timed (tools/svd_fit_rate.py)
        self.qr_on_host = False           # set when torch.linalg.qr raised on the device: the orthonormalisation then runs on the host
        if use_title:
            self.tfidf = TfidfVectorizer(input="content", **tfidf_params)
        self.svd = TruncatedSVD(dims, **kwargs)
        self.use_title = use_title
        self.scratch_bytes = int(scratch_bytes)
        self.device = device
        self._dev = self._dev_of = None

    def __str__(self):
        return str(self.svd)

    def fit(self, X, y=None):
        self._dev = self._dev_of = None
        self.fitted_on = None
        if self.fit_on == "device":
            why = self._fit_device(X)
            if why is None:
                self.fitted_on = "device"
                return self
            warnings.warn('SVDRecommender(fit="device"): fitting on the host: ' + why)
        self.svd.fit(X)
        self.fitted_on = "host"
        return self

    def _orth(self, Y):
        """An orthonormal basis of the columns of the fp32 device matrix Y [rows, l]: torch.linalg.qr on the device, or - once
        that has raised there - scipy's QR of the downloaded matrix on the host."""
        if not self.qr_on_host:
            try:
                return torch.linalg.qr(Y, mode="reduced")[0]
            except RuntimeError as e:
                self.qr_on_host = True
                warnings.warn("SVDRecommender: torch.linalg.qr is unusable on {} ({}): orthonormalising on the host".format(
                    Y.device, str(e).splitlines()[0] if str(e) else type(e).__name__))
        Q = scipy.linalg.qr(Y.cpu().numpy(), mode="economic", check_finite=False)[0]
        return _hip.upload(np.ascontiguousarray(Q, dtype=np.float32), Y.device)

    def _fit_device(self, X):
        """The randomized SVD of the class docstring.  None when self.svd has been fitted, or the reason (one line) for which
        the host has to fit."""
        svd = self.svd
        if svd.algorithm != "randomized":
            return 'algorithm="{}" has no device form'.format(svd.algorithm)
        A = _canonical(X)
        n, m = A.shape
        k, l = int(svd.n_components), int(svd.n_components) + int(svd.n_oversamples)
        if k > m:
            raise ValueError("n_components({}) must be <= n_features({}).".format(k, m))
        if l > _hip.LOWRANK_DIMS_MAX:
            return "dims + n_oversamples = {} exceeds the {} columns of the product kernel".format(l, _hip.LOWRANK_DIMS_MAX)
        if m < 2 or l > min(n, m):
            return "dims + n_oversamples = {} exceeds the smaller side of the [{} x {}] matrix".format(l, n, m)
        with np.errstate(over="ignore"):
            finite = bool(np.isfinite(A.data).all() and np.isfinite(A.data.astype(np.float32)).all())
        if not finite:
            return "the matrix holds values that are not finite (in fp32)"
        ld, tall = (l + 3) & ~3, max(n, m)
        need = 2 * tall * ld * 4 + 2 * (A.nnz * 8 + (tall + 1) * 8)
        if need > self.fit_bytes:
            return "a working set of {} bytes exceeds fit_bytes = {}".format(need, self.fit_bytes)
        dev = torch.device(self.device)
        clock = self.fit_seconds
        last = [time.perf_counter()]

        def lap(phase):
            if clock is not None:
                torch.cuda.synchronize(dev)
                now = time.perf_counter()
                clock[phase] = clock.get(phase, 0.0) + now - last[0]
                last[0] = now

        lap("other")
        dA = _hip.DeviceCSR(A, dev)
        lap("upload")
        dAt = _hip.csr_transpose(dA)
        lap("transpose")
        transpose = n < m                                   # (scikit-learn's transpose="auto")
        M, Mt = (dAt, dA) if transpose else (dA, dAt)       # CSR(M) [rows x cols], CSR(M^T)
        rows, cols = M.shape
        omega = check_random_state(svd.random_state).normal(size=(cols, l))
        # two buffers, the padding columns [l, ld) zero throughout: `qb` holds the dense operand of a product, `yb` its result
        qb = torch.zeros(tall, ld, dtype=torch.float32, device=dev)
        yb = torch.zeros(tall, ld, dtype=torch.float32, device=dev)
        qb[:cols, :l] = _hip.upload(omega.astype(np.float32), dev)
        del omega
        lap("upload")

        def product(S, normalise):
            """qb[:S.shape[0], :l] <- orth(S @ qb[:S.shape[1]]) (or the product as it is)."""
            Y = _hip.spmm_f32(S, qb[:S.shape[1]], width=l, out=yb)
            lap("products")
            if normalise:
                qb[:S.shape[0], :l] = self._orth(Y)
                lap("orthonormalisation")
            return Y

        for _ in range(int(svd.n_iter)):
            product(M, True)
            product(Mt, True)
        product(M, True)                                    # Q [rows, l]
        Bt = product(Mt, False).cpu().numpy().astype(np.float64)        # B^T = M^T Q  [cols, l]: the one download (+ Q below)
        Q = qb[:rows, :l].cpu().numpy().astype(np.float64) if transpose else None
        lap("download")
        Uhat, sigma, Vt = scipy.linalg.svd(Bt.T, full_matrices=False, lapack_driver="gesdd")
        del Bt
        # back to the input's convention, truncated: (U, s, V^T) of M^T is (V, s, U^T) of M
        components = (Q @ Uhat[:, :k]).T if transpose else Vt[:k]
        _, components = svd_flip(None, np.ascontiguousarray(components), u_based_decision=False)
        lap("host SVD")
        svd.components_ = components
        svd.singular_values_ = sigma[:k]
        svd.n_features_in_ = m
        # TruncatedSVD's explained variance: the column variances of A V^T (one more product, fp32; reduced in float64)
        qb[:m, :k] = _hip.upload(np.ascontiguousarray(components.T, dtype=np.float32), dev)
        T = _hip.spmm_f32(dA, qb[:m], width=k, out=yb)
        var = torch.cat([T[:, c:c + 64].double().var(dim=0, unbiased=False) for c in range(0, k, 64)]).cpu().numpy()
        svd.explained_variance_ = var
        svd.explained_variance_ratio_ = var / mean_variance_axis(A, axis=0)[1].sum()
        lap("explained variance")
        return None

    def transform(self, X, y=None):
        return self.svd.transform(X)

    def inverse_transform(self, X, y=None):
        return self.svd.inverse_transform(X)

    def train(self, training_set):
        x_train = training_set.tocsr()
        self.n_classes = x_train.shape[1]
        if self.use_title:
            titles = self.tfidf.fit_transform(training_set.get_single_attribute("title"))
            x_train = sp.hstack([x_train, titles])
        self.fit(x_train)
        self._table()                     # one upload (a table the device route can take, and a device to take it)

    def _features(self, test_set):
        """The rows the model reads: the item columns, then the tf-idf block of the titles."""
        x_test = test_set.tocsr()
        if self.use_title:
            titles = self.tfidf.transform(test_set.get_single_attribute("title"))
            x_test = sp.hstack([x_test, titles]).tocsr()
        return x_test

    def predict(self, test_set):
        return self.reconstruct(self._features(test_set))[:, :self.n_classes]

    # ---- ranking ---------------------------------------------------------------------------------------------------
    def _table(self):
        """The device table of self.svd.components_ as they stand (built when first needed, again when the array is another
        one), or None: no device, more dimensions than the projection kernel takes, values that are not finite."""
        V = getattr(self.svd, "components_", None)
        if self.device is None or V is None:
            return None
        if self._dev_of is not V:
            self._dev_of = V
            ok = V.shape[0] <= _hip.LOWRANK_DIMS_MAX and bool(np.isfinite(V).all()) and \
                bool(np.isfinite(np.asarray(V, dtype=np.float32)).all())
            self._dev = _hip.DeviceLowRank(V, self.device) if ok else None
        return self._dev

    def on_device(self, k=None):
        """Whether a call (k: its list length) takes the device route."""
        if k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, self.n_classes):
            return False
        return self._table() is not None

    def _inputs(self, test_set):
        """(feature rows, their item columns) in canonical CSR form, float64."""
        F = _canonical(self._features(test_set))
        if F.shape[1] != self.svd.components_.shape[1]:
            raise ValueError("the test set has {} feature columns, the model {}".format(F.shape[1], self.svd.components_.shape[1]))
        return F, _canonical(F[:, :self.n_classes])

    def _host_rows(self, F, X):
        def scores(r0, r1):
            return np.asarray(self.reconstruct(F[r0:r1]), dtype=np.float64)[:, :self.n_classes]
        return ranking.host_rows(X, scores, F.shape[1])

    def _scratch(self, n_items):
        """The two buffers of a device call, for _device_chunks."""
        dev, dims = self._dev.device, self._dev.shape[1]
        return lambda rows: {"scratch": torch.empty(rows, (n_items + 3) & ~3, dtype=torch.float32, device=dev),
                             "hidden": torch.empty(rows, (dims + 3) & ~3, dtype=torch.float32, device=dev)}

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None):
        """(item ids int32 [n, k], scaled scores float32 [n, k]) of the k best new items per test bag: predict ->
        remove_non_missing -> argtopk; id -1 / score 0 behind a row's last rankable item.  metrics: a list of bounded metric
        names - [(mean, std)] per name against y_true comes back instead (ranking.rank_metrics on the device route)."""
        F, X = self._inputs(test_set)
        n, n_items = X.shape
        if k < 1:
            raise ValueError("k must be positive")
        if not (self.on_device(k) and n):
            return ranking.host_finish_lists(ranking.host_topk(self._host_rows(F, X), n, k, _scaled), metrics, y_true, X.shape)
        lr = self._dev
        feat, items = _hip.DeviceCSR(F, lr.device), _hip.DeviceCSR(X, lr.device)
        parts = self._device_chunks(n, n_items, self._scratch(n_items),
                                    lambda s0, rows, **b: _hip.lowrank_topk(lr, n_items, feat, items, s0, rows, k, **b))
        return ranking.finish_lists(parts, k, metrics, y_true, X.shape)

    def predict_ranks(self, test_set, y_true, metrics=None):
        """CSR of int32 with y_true's (canonical) pattern: the 1-based rank of every held-out item in the full ranking of its
        test bag, in predict_topk's ordering.  A held-out item that is a known item ranks behind every rankable one, among
        the known items by id.  metrics: a list of metric names - [(mean, std)] per name comes back instead."""
        F, X = self._inputs(test_set)
        n, n_items = X.shape
        Ys = ranking.canonical_truth(y_true, X.shape, "the test set")
        if not (self.on_device() and n):
            return ranking.host_finish_ranks(ranking.host_ranks(self._host_rows(F, X), Ys), metrics)
        lr = self._dev
        feat, items, truth = (_hip.DeviceCSR(M, lr.device) for M in (F, X, Ys))
        return ranking.finish_ranks(self._device_chunks(
            n, n_items, self._scratch(n_items),
            lambda s0, rows, **b: _hip.lowrank_ranks(lr, n_items, feat, items, s0, rows, truth,
                                                     int(Ys.indptr[s0 + rows] - Ys.indptr[s0]), **b)), Ys, metrics)
