"""Most-popular baseline with its ranking on the device (the reference's MostPopular, baselines.py:46-58).

    scores[r] = counts,   counts_j = sum_d x_dj of the training set - the same vector for every row

`predict` is the reference's: the counts broadcast to the test set's shape.  `predict_topk` / `predict_ranks` are what
`Evaluation` asks for where a recommender offers them.  Every row ranks the same scores, so nothing is scored and nothing is
sorted per row: the items are ordered ONCE at train() - by (count descending, THE SMALLER ID AT EQUAL COUNTS), this project's
rule (aaerec/ranking.py; the reference leaves ties to np.argpartition's order, and item counts tie all the time) - and
csrc/popular.h answers a row from that order: its list is the first k items the row does not hold, the rank of a held-out item
its place in the order minus the known items ahead of it.  O(k + m) per list and O(m t) per row of ranks (m known items, t held
out): no [rows, items] scratch, no chunking of rows, no cap on k below the number of items.  Only [n, k] ids or nnz(truth) ranks
cross PCIe.  Scaled scores are the min-max scaling over all items - the global minimum and maximum count, known items included,
what remove_non_missing gives on the broadcast matrix - with the fp32 formula of the int32 co-occurrence route.

The order itself is plumbing: `torch.sort(counts, descending=True, stable=True)` on the device and a scatter for its inverse
(`_hip.DevicePopular`), once per train().

The device is used only where it is exact: the counts are whole numbers, every column keeps sum_d |x_dj| < 2^31 (they travel as
int32, and ids and ranks are integers from the counts through to the output), a device is named and one is present.  `route`
answers "device" or None; the host route (`ranking.host_topk` / `ranking.host_ranks` over the broadcast counts) answers
everything else - fractional or 64-bit counts, k > items, device=None - with the same rule and the same fp32 formula: callers see
no difference beyond speed.

The counts are formed where `count` says.  "host": scipy's column sum, as the reference forms it, uploaded once as int32.
"device": the training matrix goes up as int32 CSR and csrc/popular.h sums its columns with integer atomics (`_hip.pop_counts`);
`most_popular` is downloaded only when somebody reads it.  ValueError where `device_count_ok` refuses.  "auto" takes the device
when AUTO_COUNTS_ON_DEVICE says a measurement favoured it, a device is named and the guard passes.

This module is not `aaerec.baselines`: that name (RandomBaseline, the reference's own MostPopular and Countbased) keeps resolving
to the user's checkout of the reference through the package path (aaerec/__init__.py).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _hip, ranking
from .base import Recommender
from .cooc import INT32_LIMIT, _canonical, _scaled, _whole

COUNTS = ("auto", "host", "device")
# What count="auto" does where the device count is open: decided by the one measurement of tools/popular_rate.py in DESIGN 3.4g -
# scipy's column sum plus the upload of [items] counts took half the time of uploading the matrix and counting it there
AUTO_COUNTS_ON_DEVICE = False


def _column_abs_max(X):
    """max_j sum_d |x_dj| of the CSR matrix X as a float (0 without entries): float64 sums of whole numbers, exact - and
    monotone in every term - wherever the comparison with 2^31 can still go either way."""
    if not X.nnz:
        return 0.0
    return float(np.bincount(X.indices[:X.indptr[-1]], weights=np.abs(np.asarray(X.data[:X.indptr[-1]], dtype=np.float64)),
                             minlength=1).max())


def device_count_ok(X, device="cuda:0"):
    """True when the device counts the columns of X exactly as scipy does (csrc/popular.h): X is a canonical CSR matrix (columns
    strictly ascending within a row: an entry is then counted once, as scipy's sum counts it), every stored value a whole
    number, max_j sum_d |x_dj| < 2^31 (no partial sum of a column, in any order, leaves int32), and `device` names a device
    that is present."""
    if device is None or not torch.cuda.is_available():
        return False
    if not sp.issparse(X) or X.format != "csr":
        return False
    if X.shape[0] >= INT32_LIMIT or X.shape[1] >= INT32_LIMIT or X.shape[1] < 1 or not _canonical(X):
        return False
    return _whole(X) and _column_abs_max(X) < INT32_LIMIT


class MostPopular(Recommender):
    """Most Popular.  device: where the counts and their order live and the ranking runs; None keeps everything on the host.
    count: where train() sums the columns - "host" (scipy), "device" (csrc/popular.h; ValueError where device_count_ok
    refuses) or "auto" (the module docstring)."""

    def __init__(self, device="cuda:0", count="auto"):
        super().__init__()
        if count not in COUNTS:
            raise ValueError("count must be one of {}, not {!r}".format(COUNTS, count))
        if count == "device" and device is None:
            raise ValueError('count="device" needs a device')
        self.device = device
        self.count = count
        self.counted_on = None          # "host" / "device": where the last train() summed the columns
        self._mp = None
        self._dtype = None
        self._n_items = None
        self._dev = None

    def __str__(self):
        return "Most Popular baseline"

    @property
    def most_popular(self):
        """The item counts as the reference keeps them: np.matrix [1, items] of X.tocsr().sum(0)'s dtype.  After a device count
        they are downloaded on first access and kept."""
        if self._mp is None and self._dev is not None and self.counted_on == "device":
            self._mp = np.asmatrix(self._dev.counts.cpu().numpy().astype(self._dtype).reshape(1, -1))
        return self._mp

    @most_popular.setter
    def most_popular(self, counts):
        self._mp = counts

    def device_count_ok(self, X):
        """device_count_ok for this recommender's device."""
        return device_count_ok(X, self.device)

    def train(self, X):
        X = X.tocsr()
        self._mp, self._dev, self.counted_on = None, None, None
        self._n_items, self._dtype = X.shape[1], X[:0].sum(0).dtype            # (scipy's result type, from a sum over no rows)
        if self.count == "device" and not self.device_count_ok(X):
            raise ValueError('count="device": no device, or X is not a canonical CSR matrix of whole numbers with '
                             "max_j sum_d |x_dj| < 2^31 (device_count_ok)")
        if self.count == "device" or (self.count == "auto" and AUTO_COUNTS_ON_DEVICE and self.device_count_ok(X)):
            self._dev = _hip.DevicePopular(_hip.pop_counts(_hip.DeviceCooc(X, self.device)), self.device)
            self.counted_on = "device"
            return
        self.most_popular = X.sum(0)
        self.counted_on = "host"
        # one upload, and only of counts the device route can ever take: whole numbers whose columns fit int32
        if self.device is not None and torch.cuda.is_available() and self._n_items >= 1 and _whole(X) \
                and _column_abs_max(X) < INT32_LIMIT:
            self._dev = _hip.DevicePopular(np.asarray(self._mp), self.device)

    def predict(self, X):
        return np.broadcast_to(self.most_popular, X.size())

    # ---- ranking ---------------------------------------------------------------------------------------------------
    def _inputs(self, test_set):
        X = test_set.tocsr()
        X.sum_duplicates()
        X.sort_indices()
        if X.shape[1] != self._n_items:
            raise ValueError("the test set has {} columns, the model {} items".format(X.shape[1], self._n_items))
        return X

    def _route_of(self, n_rows, k=None):
        if self._dev is None or not n_rows or (k is not None and not 1 <= k <= self._n_items):
            return None
        return "device"

    def route(self, test_set, k=None):
        """Which route predict_topk(test_set, k) - or, without k, predict_ranks(test_set, ...) - takes: "device", or None on
        the host."""
        return self._route_of(self._inputs(test_set).shape[0], k)

    def _host_rows(self, X):
        counts = np.asarray(self.most_popular, dtype=np.float64).ravel()
        return ranking.host_rows(X, lambda r0, r1: np.broadcast_to(counts, (min(r1, X.shape[0]) - r0, counts.size)))

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None):
        """(item ids int32 [n, k], scaled scores float32 [n, k]) of the k most popular new items per test bag: predict ->
        remove_non_missing -> argtopk; id -1 / score 0 behind a row's last rankable item.  metrics: a list of bounded metric
        names - [(mean, std)] per name against y_true comes back instead (ranking.rank_metrics on the device route)."""
        X = self._inputs(test_set)
        n = X.shape[0]
        if k < 1:
            raise ValueError("k must be positive")
        if not self._route_of(n, k):
            return ranking.host_finish_lists(ranking.host_topk(self._host_rows(X), n, k, _scaled), metrics, y_true, X.shape)
        return ranking.finish_lists([_hip.pop_topk(self._dev, _hip.DeviceCSR(X, self._dev.device), 0, n, k)], k, metrics, y_true, X.shape)

    def predict_ranks(self, test_set, y_true, metrics=None):
        """CSR of int32 with y_true's (canonical) pattern: the 1-based rank of every held-out item in the full ranking of its
        test bag, in predict_topk's ordering.  A held-out item that is a known item ranks behind every rankable one, among
        the known items by id.  metrics: a list of metric names - [(mean, std)] per name comes back instead."""
        X = self._inputs(test_set)
        n = X.shape[0]
        Ys = ranking.canonical_truth(y_true, X.shape, "the test set")
        if not self._route_of(n):
            return ranking.host_finish_ranks(ranking.host_ranks(self._host_rows(X), Ys), metrics)
        csr, truth = _hip.DeviceCSR(X, self._dev.device), _hip.DeviceCSR(Ys, self._dev.device)
        return ranking.finish_ranks([_hip.pop_ranks(self._dev, csr, 0, n, truth, int(Ys.nnz))], Ys, metrics)
