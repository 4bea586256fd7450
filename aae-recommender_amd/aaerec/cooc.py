"""Item co-occurrence baseline with its ranking on the device (the reference's Countbased, baselines.py:22-43).

    scores = X_test @ C,   C = X^T X of the training set   (order n: C <- C^T C, n - 1 times)

`predict` is the reference's: the scipy product, the host route.  `predict_topk` / `predict_ranks` are what `Evaluation` asks
for where a recommender offers them: the scores are formed by csrc/cooc.h in int32 (exact), written into a [rows, items]
scratch and ranked there by the dense kernels of csrc/rank_long.h / rank_full.h - row-wise min-max scaling with the known items
still in the minimum and maximum, known items masked, the better score first, THE SMALLER ID AT EQUAL SCORES (the reference
leaves ties to np.argpartition's order; co-occurrence counts tie often).  Only [n, k] ids or nnz(truth) ranks cross PCIe.

The device is used only where it is exact, and `device_route` says how (`Countbased.route` for a trained model).  X and C hold
whole numbers and max |C| < 2^31 on both device routes.
  "f32"  max_r (sum_i |x_ri|) * max |C| < 2^24 (`device_route_ok`): every score is a whole number fp32 represents; the scratch
         is fp32 and the float rank kernels order it.
  "i32"  otherwise, while max |x| < 2^24 and max_r sum_i |x_ri| * m_i < 2^31 with m_i = max_j |C_ij|: no sum leaves int32; the
         scratch is int32 and the integer members of the same kernels order the scores themselves, so nothing ties that is
         not equal.  The bound counts only the rows of C that a bag touches, each with its own maximum.
  None   anything else - and a list longer than min(1024, items) - is answered on the host from predict() with the same
         ordering rule and the same fp32 formula for the scaled scores: callers see no difference beyond speed.

C is built where `build` says.  "host": scipy's product, as the reference builds it, uploaded once by train().  "device": X goes
up as int32 CSR, X^T is formed there by csrc/sptrans.h (`_hip.cooc_transpose`) and C = X^T . X by the exact int32 sparse product of
csrc/spgemm.h (`_hip.spgemm_i32`), as is C . C for every further order; nothing is uploaded a second time, and `cooccurences`
is downloaded only when somebody reads it.  The device builds only what it builds exactly (`device_build_ok`: a canonical X of
strictly positive whole numbers with max_i sum_d x_di^2 < 2^31; before each further order max_i sum_j C_ij^2 < 2^31): the
result has scipy's indptr, indices and values.  "auto" takes the device route when AUTO_BUILDS_ON_DEVICE says the measurement
favoured it, a device is named and the guard passes, and continues on the host from the order at which a guard fails.

This module is not `aaerec.baselines`: that name (MostPopular, RandomBaseline, the reference's own Countbased) keeps resolving
to the user's checkout of the reference through the package path (aaerec/__init__.py).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _hip, ranking
from .base import Recommender

EXACT_FP32 = 1 << 24          # every whole number up to here is an fp32
INT32_LIMIT = 1 << 31
# value types in which scipy's product of whole numbers below 2^31 is exact, so that both builds give the same matrix
_EXACT_DTYPES = tuple(np.dtype(t) for t in (np.float64, np.int32, np.int64, np.uint32, np.uint64))


def _abs_max(M):
    return float(np.abs(M.data).max()) if M.nnz else 0.0


def _whole(M):
    return bool(np.all(M.data == np.rint(M.data))) if M.nnz else True


def _route_ok(X, c_whole, c_abs_max):
    """The one rule of device_route_ok, from what is known of C: whether its values are whole, and max |C|."""
    X = sp.csr_matrix(X)
    if not (_whole(X) and c_whole):
        return False
    if c_abs_max >= INT32_LIMIT:
        return False
    row_sum = float(abs(X).sum(axis=1).max()) if X.nnz else 0.0
    return row_sum * c_abs_max < EXACT_FP32


def device_route_ok(X, C):
    """True when X @ C on the device is exact: X and C hold whole numbers, max |C| < 2^31 (its int32 upload), and the largest
    score any row can reach, max_r (sum_i |x_ri|) * max |C|, stays below 2^24 (the int32 sum is then a whole number that fp32
    represents).  X, C: scipy sparse matrices."""
    C = sp.csr_matrix(C)
    return _route_ok(X, _whole(C), _abs_max(C))


def _route(X, c_whole, c_abs_max, row_abs_max):
    """device_route's rule from what is known of an uploaded C: whether its values are whole, max |C|, and a function that
    returns m_i = max_j |C_ij| as a host array [items] (called only when the "f32" rule fails)."""
    X = sp.csr_matrix(X)
    if _route_ok(X, c_whole, c_abs_max):
        return "f32"
    if not (c_whole and c_abs_max < INT32_LIMIT and _whole(X) and _abs_max(X) < EXACT_FP32):
        return None
    bound = abs(X).astype(np.float64) @ np.asarray(row_abs_max(), dtype=np.float64)
    return "i32" if float(bound.max()) < INT32_LIMIT else None


def device_route(X, C, device="cuda:0"):
    """How the device answers X @ C exactly: "f32", "i32" or None (the host route).  X, C: scipy sparse matrices; device: None
    when there is none to upload C to.
      "f32"  exactly where device_route_ok(X, C) holds.
      "i32"  otherwise, when X and C hold whole numbers, max |x| < 2^24 (the batch travels as fp32 and the kernel reads it
             back with a round to nearest), max |C| < 2^31 (its int32 upload) and, with m_i = max_j |C_ij|,
                 B = max_r sum_i |x_ri| * m_i < 2^31.
             For row r and any column j, every partial sum of sum_i x_ri * C_ij, in any order, is at most
             sum_i |x_ri| * |C_ij| <= B in magnitude: the int32 accumulation cannot wrap, every score lies in
             [-(2^31 - 1), 2^31 - 1], and INT32_MIN - what the rank kernels mask a known item to - is never a score.
      None   everything else.
    B is computed as abs(X) @ m in float64.  All terms are non-negative whole numbers.  If the true sum of a row is below 2^31
    then so is every product and partial sum, all of them are exact in float64 (whole numbers below 2^53), and the computed
    value is the true one.  If it is not, take the first operation, in the order the products and sums are evaluated, whose
    exact result reaches 2^31: its operands are still exact, rounding is monotone and 2^31 is a float64, so its rounded result
    is >= 2^31, and adding non-negative terms never lowers a rounded sum below it.  Either way the comparison is the true one."""
    if device is None:
        return None
    C = sp.csr_matrix(C)
    return _route(X, _whole(C), _abs_max(C), lambda: np.asarray(abs(C).max(axis=1).toarray(), dtype=np.float64).ravel()
                  if C.nnz else np.zeros(C.shape[0]))


def _canonical(X):
    """Columns strictly ascending within every row of the CSR matrix X (sorted, no duplicates) - looked at, not enforced."""
    nnz = int(X.indptr[-1])
    if nnz < 2:
        return True
    rising = np.diff(X.indices[:nnz]) > 0
    starts = np.asarray(X.indptr[1:-1])
    starts = starts[(starts > 0) & (starts < nnz)]
    rising[starts - 1] = True                     # (the step from a row's last entry to the next row's first is free)
    return bool(rising.all())


def device_build_ok(X):
    """True when the device builds C = X^T X exactly as scipy does (csrc/spgemm.h): X is a canonical CSR matrix of float64 or
    of 32- / 64-bit integers (what scipy itself multiplies exactly below 2^31), every stored value a strictly positive whole number - scipy keeps a structural entry for an explicit zero and for a sum that cancels;
    positive values rule both out, so the pattern is scipy's - and max_i sum_d x_di^2 < 2^31: for a Gram matrix
    C_ij <= sqrt(C_ii C_jj) <= max_i C_ii, so every entry and, the terms being positive, every partial sum fits int32."""
    if not sp.issparse(X) or X.format != "csr":
        return False
    if X.shape[0] >= INT32_LIMIT or X.shape[1] >= INT32_LIMIT or not _canonical(X):
        return False
    if not X.nnz:
        return True
    data = np.asarray(X.data)
    if data.dtype not in _EXACT_DTYPES:           # (scipy's own product would round or wrap: the two builds would differ)
        return False
    if not (np.all(data > 0) and np.all(data == np.rint(data))):
        return False
    if float(data.max()) ** 2 >= INT32_LIMIT:     # (every square below is then an integer float64 holds)
        return False
    diag = np.bincount(X.indices, weights=data.astype(np.float64) ** 2, minlength=X.shape[1])
    return bool(diag.max() < INT32_LIMIT)


def _power_ok(C):
    """Whether the device may form C . C for the symmetric DeviceCooc C: max_i sum_j C_ij^2 < 2^31 - the largest diagonal
    entry of the Gram matrix C^T C, which bounds all of it.  An int64 reduction over the CSR values on the device."""
    if not C.nnz:
        return True
    if C.abs_max() ** 2 >= INT32_LIMIT:           # (each square below is then < 2^31: no row sum can leave int64)
        return False
    sq = C.values[:C.nnz].to(torch.int64) ** 2
    rows = torch.repeat_interleave(torch.arange(C.shape[0], device=C.device), C.indptr.diff())
    return int(torch.zeros(C.shape[0], dtype=torch.int64, device=C.device).index_add_(0, rows, sq).max()) < INT32_LIMIT


def _scaled(s, best):
    """The scaled scores of the items `best` of a row as the device routes form them: fp32 arithmetic throughout."""
    lo, span = np.float32(s.min()), np.float32(s.max()) - np.float32(s.min())
    inv = np.float32(1) / span if span > 0 else np.float32(1)
    return (s[best].astype(np.float32) - lo) * inv


_SCRATCH = {"f32": torch.float32, "i32": torch.int32}      # the score type of each device route
BUILDS = ("auto", "host", "device")
# What build="auto" does where the device route is open: decided by the one measurement of tools/cooc_build_rate.py in DESIGN 3.4d
AUTO_BUILDS_ON_DEVICE = True


class Countbased(ranking.ScratchRanker, Recommender):
    """Item Co-Occurrence.  order: 1 = C = X^T X; n = C <- C^T C repeated n - 1 times.  scratch_bytes: the [rows, items]
    scratch (fp32 or int32) of one device call - the rows of a predict_topk / predict_ranks call are chunked to it.  device: where C
    lives and the ranking runs; None keeps everything on the host.  build: where train() forms C - "host" (scipy), "device"
    (csrc/spgemm.h; ValueError where there is no device or device_build_ok refuses) or "auto" (the module docstring)."""

    def __init__(self, order=1, scratch_bytes=256 << 20, device="cuda:0", build="auto"):
        super().__init__()
        if build not in BUILDS:
            raise ValueError("build must be one of {}, not {!r}".format(BUILDS, build))
        if build == "device" and device is None:
            raise ValueError('build="device" needs a device')
        self.order = order
        self.scratch_bytes = int(scratch_bytes)
        self.device = device
        self.build = build
        self.built_on = None            # "host" / "device": where the last train() formed C (its last product)
        self._cooc = None
        self._shape = None
        self._dtype = None
        self._cmax = 0.0                # max |C| of the uploaded matrix: on_device() reads this, not the matrix
        self._dev = None

    def __str__(self):
        return "Count-based Predictor (order {})".format(self.order)

    @property
    def cooccurences(self):
        """C as a scipy CSR (the reference's spelling: drivers and notebooks read this attribute).  After a device build it is
        downloaded on first access and kept."""
        if self._cooc is None and self._dev is not None and self.built_on == "device":
            self._cooc = self._dev.to_scipy().astype(self._dtype)
        return self._cooc

    @cooccurences.setter
    def cooccurences(self, C):
        self._cooc = C

    def train(self, X):
        X = X.tocsr()
        self._cooc, self._dev, self._cmax, self._shape, self._dtype = None, None, 0.0, (X.shape[1], X.shape[1]), X.dtype
        self.built_on = None
        if self.build == "device" and not device_build_ok(X):
            raise ValueError('build="device": X is not a canonical CSR matrix of strictly positive whole numbers with '
                             "max_i sum_d x_di^2 < 2^31 (device_build_ok)")
        if self.build == "device" or (self.build == "auto" and AUTO_BUILDS_ON_DEVICE and self.device is not None and device_build_ok(X)):
            C, done = self._train_device(X)
            if C is None:
                return
        else:
            C, done = (X.T @ X).tocsr(), 1
        for _ in range(self.order - done):
            C = (C.T @ C).tocsr()
        C.sum_duplicates()
        C.sort_indices()
        self.cooccurences = C
        self.built_on = "host"
        # one upload, and only of a matrix the device route can ever take: whole numbers that fit int32
        if self.device is not None and _whole(C) and _abs_max(C) < INT32_LIMIT:
            self._dev = _hip.DeviceCooc(C, self.device)
            self._cmax = _abs_max(C)

    def _train_device(self, X):
        """C on the device: (None, order) when every product was formed there - self._dev is the result - or (the scipy matrix
        of the last order the device formed, that order) for train() to continue from on the host."""
        Xd = _hip.DeviceCooc(X, self.device)
        C = _hip.spgemm_i32(_hip.cooc_transpose(Xd), Xd)
        for done in range(1, self.order):
            if not _power_ok(C):
                if self.build == "device":
                    raise ValueError('build="device": max_i sum_j C_ij^2 >= 2^31 at order {}: the next product leaves int32'.format(done))
                return C.to_scipy().astype(X.dtype), done
            # X^T X is symmetric and so is every power of it, so C^T C = C . C and no transpose is needed on the device
            C = _hip.spgemm_i32(C, C)
        self._dev, self._cmax, self.built_on = C, float(C.abs_max()), "device"
        return None, self.order

    def predict(self, X):
        return X.tocsr() @ self.cooccurences

    # ---- ranking ---------------------------------------------------------------------------------------------------
    def _inputs(self, test_set):
        X = test_set.tocsr().astype(np.float64)
        X.sum_duplicates()
        X.sort_indices()
        if X.shape[1] != self._shape[0]:
            raise ValueError("the test set has {} columns, the model {} items".format(X.shape[1], self._shape[0]))
        return X

    def on_device(self, X, k=None):
        """Whether a call over the rows X (k: its list length) takes the fp32 device route - the "f32" of route(), which also
        names the int32 one."""
        n_items = self._shape[1]
        if self._dev is None or (k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, n_items)):
            return False
        return _route_ok(X, True, self._cmax)      # (device_route_ok's rule: an uploaded C is whole, max |C| kept by train())

    def _route_of(self, X, k=None):
        """device_route for the rows X (a canonical CSR) of a call with list length k, from what train() kept of C: its
        maximum and, through the uploaded matrix, its row maxima - C itself is never downloaded for this."""
        n_items = self._shape[1]
        if self._dev is None or (k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, n_items)):
            return None
        return _route(X, True, self._cmax, self._dev.row_abs_max)

    def route(self, test_set, k=None):
        """Which route predict_topk(test_set, k) - or, without k, predict_ranks(test_set, ...) - takes: "f32" or "i32" on the
        device (device_route), None on the host."""
        return self._route_of(self._inputs(test_set), k)

    def _host_rows(self, X):
        return ranking.host_rows(X, lambda r0, r1: (X[r0:r1] @ self.cooccurences).toarray())

    def _scratch(self, route, n_items):
        """The one buffer of a device call on `route`, for _device_chunks."""
        return lambda rows: {"scratch": torch.empty(rows, (n_items + 3) & ~3, dtype=_SCRATCH[route], device=self._dev.device)}

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None):
        """(item ids int32 [n, k], scaled scores float32 [n, k]) of the k best new items per test bag: predict ->
        remove_non_missing -> argtopk; id -1 / score 0 behind a row's last rankable item.  metrics: a list of bounded metric
        names - [(mean, std)] per name against y_true comes back instead (ranking.rank_metrics on the device route)."""
        X = self._inputs(test_set)
        n, n_items = X.shape
        if k < 1:
            raise ValueError("k must be positive")
        route = self._route_of(X, k) if n else None
        if not route:
            return ranking.host_finish_lists(ranking.host_topk(self._host_rows(X), n, k, _scaled), metrics, y_true, X.shape)
        topk, csr = getattr(_hip, "cooc_topk" if route == "f32" else "cooc_topk_i32"), _hip.DeviceCSR(X, self._dev.device)
        parts = self._device_chunks(n, n_items, self._scratch(route, n_items),
                                    lambda s0, rows, **b: topk(self._dev, csr, s0, rows, k, **b))
        return ranking.finish_lists(parts, k, metrics, y_true, X.shape)

    def predict_ranks(self, test_set, y_true, metrics=None):
        """CSR of int32 with y_true's (canonical) pattern: the 1-based rank of every held-out item in the full ranking of its
        test bag, in predict_topk's ordering.  A held-out item that is a known item ranks behind every rankable one, among
        the known items by id.  metrics: a list of metric names - [(mean, std)] per name comes back instead."""
        X = self._inputs(test_set)
        n, n_items = X.shape
        Ys = ranking.canonical_truth(y_true, X.shape, "the test set")
        route = self._route_of(X) if n else None
        if not route:
            return ranking.host_finish_ranks(ranking.host_ranks(self._host_rows(X), Ys), metrics)
        ranks = getattr(_hip, "cooc_ranks" if route == "f32" else "cooc_ranks_i32")
        csr, truth = _hip.DeviceCSR(X, self._dev.device), _hip.DeviceCSR(Ys, self._dev.device)
        return ranking.finish_ranks(self._device_chunks(
            n, n_items, self._scratch(route, n_items),
            lambda s0, rows, **b: ranks(self._dev, csr, s0, rows, truth, int(Ys.indptr[s0 + rows] - Ys.indptr[s0]), **b)), Ys, metrics)
