"""Item co-occurrence baseline with its ranking on the device (the reference's Countbased, baselines.py:22-43).

    scores = X_test @ C,   C = X^T X of the training set   (order n: C <- C^T C, n - 1 times)

`predict` is the reference's: the scipy product, the host route.  `predict_topk` / `predict_ranks` are what `Evaluation` asks
for where a recommender offers them: the scores are formed by csrc/cooc.h in int32 (exact), written as fp32 into a
[rows, items] scratch and ranked there by the dense kernels of csrc/rank_long.h / rank_full.h - row-wise min-max scaling with
the known items still in the minimum and maximum, known items masked, the better score first, THE SMALLER ID AT EQUAL SCORES
(the reference leaves ties to np.argpartition's order; co-occurrence counts tie often).  Only [n, k] ids or nnz(truth) ranks
cross PCIe.

The device is used only where it is exact (`device_route_ok`): whole-number values in X and C, max |C| < 2^31, and
max_r (sum_i |x_ri|) * max |C| < 2^24, so that every score is a whole number fp32 represents.  Anything else - and a list
longer than min(1024, items) - is answered on the host from predict() with the same ordering rule: callers see no difference
beyond speed.  C itself is built on the host with scipy, as the reference builds it, and uploaded once by train().

This module is not `aaerec.baselines`: that name (MostPopular, RandomBaseline, the reference's own Countbased) keeps resolving
to the user's checkout of the reference through the package path (aaerec/__init__.py).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _hip
from .base import Recommender

EXACT_FP32 = 1 << 24          # every whole number up to here is an fp32
INT32_LIMIT = 1 << 31


def _abs_max(M):
    return float(np.abs(M.data).max()) if M.nnz else 0.0


def _whole(M):
    return bool(np.all(M.data == np.rint(M.data))) if M.nnz else True


def device_route_ok(X, C):
    """True when X @ C on the device is exact: X and C hold whole numbers, max |C| < 2^31 (its int32 upload), and the largest
    score any row can reach, max_r (sum_i |x_ri|) * max |C|, stays below 2^24 (the int32 sum is then a whole number that fp32
    represents).  X, C: scipy sparse matrices."""
    X, C = sp.csr_matrix(X), sp.csr_matrix(C)
    if not (_whole(X) and _whole(C)):
        return False
    cmax = _abs_max(C)
    if cmax >= INT32_LIMIT:
        return False
    row_sum = float(abs(X).sum(axis=1).max()) if X.nnz else 0.0
    return row_sum * cmax < EXACT_FP32


def _order_row(s, known):
    """Item ids of one row, best first: score descending, the smaller id at equal scores, known items left out."""
    ids = np.lexsort((np.arange(s.size), -s))
    return ids[~np.isin(ids, known)] if len(known) else ids


class Countbased(Recommender):
    """Item Co-Occurrence.  order: 1 = C = X^T X; n = C <- C^T C repeated n - 1 times.  scratch_bytes: the [rows, items]
    fp32 scratch of one device call - the rows of a predict_topk / predict_ranks call are chunked to it.  device: where C
    lives and the ranking runs; None keeps everything on the host."""

    def __init__(self, order=1, scratch_bytes=256 << 20, device="cuda:0"):
        super().__init__()
        self.order = order
        self.scratch_bytes = int(scratch_bytes)
        self.device = device
        self.cooccurences = None        # (the reference's spelling: drivers and notebooks read this attribute)
        self._dev = None

    def __str__(self):
        return "Count-based Predictor (order {})".format(self.order)

    def train(self, X):
        X = X.tocsr()
        C = (X.T @ X).tocsr()
        for _ in range(self.order - 1):
            C = (C.T @ C).tocsr()
        C.sum_duplicates()
        C.sort_indices()
        self.cooccurences = C
        self._dev = None
        # one upload, and only of a matrix the device route can ever take: whole numbers that fit int32
        if self.device is not None and _whole(C) and _abs_max(C) < INT32_LIMIT:
            self._dev = _hip.DeviceCooc(C, self.device)

    def predict(self, X):
        return X.tocsr() @ self.cooccurences

    # ---- ranking ---------------------------------------------------------------------------------------------------
    def _inputs(self, test_set):
        X = test_set.tocsr().astype(np.float64)
        X.sum_duplicates()
        X.sort_indices()
        if X.shape[1] != self.cooccurences.shape[0]:
            raise ValueError("the test set has {} columns, the model {} items".format(X.shape[1], self.cooccurences.shape[0]))
        return X

    def on_device(self, X, k=None):
        """Whether a call over the rows X (k: its list length) takes the device route."""
        n_items = self.cooccurences.shape[1]
        if self._dev is None or (k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, n_items)):
            return False
        return device_route_ok(X, self.cooccurences)

    def _chunk_rows(self, n_items):
        return max(1, self.scratch_bytes // (4 * ((n_items + 3) & ~3)))

    def _host_rows(self, X):
        """(row number, its scores float64 [items], its known item ids) over the rows of X, a bounded block at a time."""
        step = max(1, (64 << 20) // (8 * max(1, X.shape[1])))
        for r0 in range(0, X.shape[0], step):
            S = np.asarray((X[r0:r0 + step] @ self.cooccurences).toarray(), dtype=np.float64)
            for j in range(S.shape[0]):
                yield r0 + j, S[j], X.indices[X.indptr[r0 + j]:X.indptr[r0 + j + 1]]

    def predict_topk(self, test_set, k=10):
        """(item ids int32 [n, k], scaled scores float32 [n, k]) of the k best new items per test bag: predict ->
        remove_non_missing -> argtopk; id -1 / score 0 behind a row's last rankable item."""
        X = self._inputs(test_set)
        n, n_items = X.shape
        if k < 1:
            raise ValueError("k must be positive")
        if self.on_device(X, k) and n:
            csr = _hip.DeviceCSR(X, self._dev.device)
            chunk = self._chunk_rows(n_items)
            scratch = torch.empty(min(chunk, n), (n_items + 3) & ~3, dtype=torch.float32, device=self._dev.device)
            parts = [_hip.cooc_topk(self._dev, csr, s0, min(chunk, n - s0), k, scratch=scratch) for s0 in range(0, n, chunk)]
            return torch.cat([p[0] for p in parts]).cpu().numpy(), torch.cat([p[1] for p in parts]).cpu().numpy()
        ids = np.full((n, k), -1, dtype=np.int32)
        val = np.zeros((n, k), dtype=np.float32)
        for r, s, known in self._host_rows(X):
            best = _order_row(s, known)[:k]
            lo, span = np.float32(s.min()), np.float32(s.max()) - np.float32(s.min())
            inv = np.float32(1) / span if span > 0 else np.float32(1)
            ids[r, :best.size] = best
            val[r, :best.size] = (s[best].astype(np.float32) - lo) * inv
        return ids, val

    def predict_ranks(self, test_set, y_true):
        """CSR of int32 with y_true's (canonical) pattern: the 1-based rank of every held-out item in the full ranking of its
        test bag, in predict_topk's ordering.  A held-out item that is a known item ranks behind every rankable one, among
        the known items by id."""
        X = self._inputs(test_set)
        n, n_items = X.shape
        Ys = sp.csr_matrix(y_true, copy=True) if not sp.issparse(y_true) else y_true.tocsr(copy=True)
        if Ys.shape != X.shape:
            raise ValueError("the ground truth has shape {}, the test set {}".format(Ys.shape, X.shape))
        Ys.sum_duplicates()
        Ys.sort_indices()
        if self.on_device(X) and n:
            csr, truth = _hip.DeviceCSR(X, self._dev.device), _hip.DeviceCSR(Ys, self._dev.device)
            chunk = self._chunk_rows(n_items)
            scratch = torch.empty(min(chunk, n), (n_items + 3) & ~3, dtype=torch.float32, device=self._dev.device)
            parts = []
            for s0 in range(0, n, chunk):
                rows = min(chunk, n - s0)
                nnz = int(Ys.indptr[s0 + rows] - Ys.indptr[s0])
                parts.append(_hip.cooc_ranks(self._dev, csr, s0, rows, truth, nnz, scratch=scratch))
            data = torch.cat(parts).cpu().numpy().astype(np.int32, copy=False)
        else:
            data = np.zeros(Ys.nnz, dtype=np.int32)
            for r, s, known in self._host_rows(X):
                lo, hi = Ys.indptr[r], Ys.indptr[r + 1]
                if lo == hi:
                    continue
                s = s.copy()
                s[known] = -np.inf
                ids = np.arange(n_items)
                for e in range(lo, hi):
                    t = Ys.indices[e]
                    data[e] = 1 + np.count_nonzero((s > s[t]) | ((s == s[t]) & (ids < t)))
        return sp.csr_matrix((data, Ys.indices.copy(), Ys.indptr.copy()), shape=Ys.shape)
