"""Metric side of the hot path (mirrors reference aaerec/evaluation.py): argtopk 20-58,
RankingMetric/MRR/MAP/P 61-163, METRICS 166-180, remove_non_missing 183-199, evaluate 202-240,
Evaluation 263-404 (wandb hooks dropped)."""
import os
import random
import sys
from datetime import timedelta
from timeit import default_timer as timer

import numpy as np
import scipy.sparse as sp
from sklearn.preprocessing import minmax_scale

from . import rank_metrics_with_std as rm
from .datasets import corrupt_sets
from .transforms import lists2sparse


def argtopk(X, k):
    """Index pair (rows, cols) selecting the k largest entries of every row, descending.

    >>> X = np.arange(20).reshape(2, 10)
    >>> X[argtopk(X, 3)].tolist()
    [[9, 8, 7], [19, 18, 17]]
    >>> np.arange(6).reshape(2, 3)[argtopk(np.arange(6).reshape(2, 3), 100)].tolist()
    [[2, 1, 0], [5, 4, 3]]
    """
    assert len(X.shape) == 2, "X should be two-dimensional array-like"
    rows = np.arange(X.shape[0])[:, np.newaxis]
    if k is None or k >= X.size:
        return rows, np.argsort(X, axis=1)[:, ::-1]
    assert k > 0, "k should be positive integer or None"
    part = np.argpartition(X, -k, axis=1)[:, -k:]
    order = np.argsort(X[rows, part], axis=1)[:, ::-1]
    return rows, part[rows, order]


class RankingMetric:
    """Relevance of the top-k predictions, in rank order."""

    def __init__(self, *args, **kwargs):
        self.k = kwargs.pop("k", None)

    def __call__(self, y_true, y_pred, average=True):
        return y_true[argtopk(y_pred, self.k)]


class MRR(RankingMetric):
    """
    >>> MRR(2)(np.array([[1, 0, 0], [0, 0, 1]]), np.array([[0.2, 0.3, 0.1], [0.2, 0.5, 0.7]]))
    (0.75, 0.25)
    """

    def __init__(self, k=None):
        super().__init__(k=k)

    def __call__(self, y_true, y_pred, average=True):
        return rm.mean_reciprocal_rank(super().__call__(y_true, y_pred), average=average)


class MAP(RankingMetric):
    """
    >>> MAP(2)(np.array([[1, 0, 0], [0, 0, 1]]), np.array([[0.2, 0.3, 0.1], [0.2, 0.5, 0.7]]))
    (0.75, 0.25)
    """

    def __init__(self, k=None):
        super().__init__(k=k)

    def __call__(self, y_true, y_pred, average=True):
        rs = super().__call__(y_true, y_pred)
        if average:
            return rm.mean_average_precision(rs)
        return np.array([rm.average_precision(r) for r in rs])


class P(RankingMetric):
    """
    >>> P(2)(np.array([[1, 0, 1, 0], [1, 0, 1, 0]]), np.array([[.2, .3, .1, .05], [.2, .5, .7, .05]]))
    (0.5, 0.0)
    """

    def __init__(self, k=None):
        super().__init__(k=k)

    def __call__(self, y_true, y_pred, average=True):
        ps = (super().__call__(y_true, y_pred) > 0).mean(axis=1)
        return (ps.mean(), ps.std()) if average else ps


BOUNDED_METRICS = {"{}@{}".format(M.__name__.lower(), k): M(k) for M in (MRR, MAP, P) for k in (5, 10, 20)}
BOUNDED_METRICS["P@1"] = P(1)
UNBOUNDED_METRICS = {M.__name__.lower(): M() for M in (MRR, MAP)}
METRICS = {**BOUNDED_METRICS, **UNBOUNDED_METRICS}


def remove_non_missing(Y_pred, X_test, copy=True):
    """Row-wise min-max scaling to [0,1] (sklearn.preprocessing.minmax_scale(axis=1) semantics:
    constant rows map to 0), then zero the items already present in the input.

    >>> remove_non_missing(np.array([[0.6, 0.5, -1], [40, -20, 10]]), np.array([[1, 0, 1], [0, 1, 0]])).tolist()
    [[0.0, 0.9375, 0.0], [1.0, 0.0, 0.5]]
    """
    Y = minmax_scale(Y_pred, feature_range=(0, 1), axis=1, copy=copy)
    Y[X_test.nonzero()] = 0.0
    return Y


def evaluate(ground_truth, predictions, metrics, batch_size=None):
    """[(mean, std)] per metric; batch_size bounds the dense working set."""
    n = ground_truth.shape[0]
    assert predictions.shape[0] == n
    metrics = [m if callable(m) else METRICS[m] for m in metrics]
    dense = lambda a: a.toarray() if sp.issparse(a) else a   # noqa: E731
    if batch_size is None:
        gt, pr = dense(ground_truth), dense(predictions)
        return [metric(gt, pr) for metric in metrics]
    per_metric = [[] for _ in metrics]
    for start in range(0, n, int(batch_size)):
        stop = min(start + int(batch_size), n)
        gt, pr = dense(ground_truth[start:stop, :]), dense(predictions[start:stop, :])
        for acc, metric in zip(per_metric, metrics):
            acc.extend(metric(gt, pr, average=False))
    return [(np.mean(v), np.std(v)) for v in map(np.asarray, per_metric)]


# ---- metric names -----------------------------------------------------------------------------------------------------------
# A metric a rank-based route can answer is (kind, k): kind one of METRIC_KINDS, k a positive integer or None (unbounded: 'mrr',
# 'map').  The three kinds of the RecSys-2018 challenge (reference eval/mpd/mpd_metrics.py:43-144, as eval/evaluate_dev.py uses
# them) are functions of a row's sorted held-out ranks r_1 < ... < r_m and the list cap k alone:
#   r-prec@k = #{r_j <= min(m, k)} / m
#   ndcg@k   = sum_{r_j <= k} d[r_j] / sum_{i = 1 .. min(k, m)} d[i],  d[i] = 1 / log2(1 + i)
#   clicks@k = floor((r_1 - 1) / 10) if r_1 <= k, else k / 10 + 1
METRIC_KINDS = ("mrr", "map", "p", "ndcg", "r-prec", "clicks")
RANK_ABSENT = 2 ** 31 - 1       # the stored rank of a held-out item that a top-k list does not hold: never <= k, counts towards m


def metric_spec(name):
    """(kind, k) of a metric name: 'mrr', 'map' (k None), 'mrr@k', 'map@k', 'p@k' / 'P@k', 'ndcg@k', 'r-prec@k', 'clicks@k' with
    any integer k >= 1.  ValueError for anything else."""
    if not isinstance(name, str):
        raise ValueError("a metric name is a string, not {!r}".format(name))
    kind, at, tail = name.partition("@")
    kind = "p" if kind == "P" else kind
    if kind not in METRIC_KINDS:
        raise ValueError("unknown metric {!r}".format(name))
    if not at:
        if kind not in ("mrr", "map"):
            raise ValueError("metric {!r} needs a cap: {}@k".format(name, kind))
        return kind, None
    if not (tail.isascii() and tail.isdigit()) or int(tail) < 1:
        raise ValueError("the cap of metric {!r} must be an integer >= 1".format(name))
    return kind, int(tail)


def metric_name(kind, k=None):
    """The name metric_spec reads (kind, k) from ('p@k' in lower case)."""
    if kind not in METRIC_KINDS or (k is None and kind not in ("mrr", "map")) or (k is not None and int(k) < 1):
        raise ValueError("no metric ({!r}, {!r})".format(kind, k))
    return kind if k is None else "{}@{}".format(kind, int(k))


CHALLENGE_METRICS = {metric_name(kind, k): (kind, k) for kind in ("r-prec", "ndcg", "clicks") for k in (5, 10, 20, 500)}


def _is_metric_name(name):
    try:
        metric_spec(name)
    except ValueError:
        return False
    return True


def _specs(metrics):
    """[(kind, k)] of a list of names: a name of METRICS by its object (as ever), any other through metric_spec."""
    out = []
    for name in metrics:
        if isinstance(name, str) and name in METRICS:
            metric = METRICS[name]
            out.append(("mrr" if isinstance(metric, MRR) else "map" if isinstance(metric, MAP) else "p", metric.k))
        else:
            out.append(metric_spec(name))
    return out


def device_metrics_ok(row_lengths, specs, device="cuda:0"):
    """True when csrc/rank_metrics.h answers `specs` for rows of these lengths: a device is named and present, no row is longer
    than AAE_METRIC_ROW_MAX, every cap fits int32 and no ndcg cap exceeds the longest discount table (2^20)."""
    from . import _hip
    import torch
    if device is None or not torch.cuda.is_available():
        return False
    lengths = np.asarray(row_lengths)
    if lengths.size >= 2 ** 31 - 1 or (lengths.size and int(lengths.max()) > _hip.METRIC_ROW_MAX):
        return False
    return all(k is None or (k < RANK_ABSENT and (kind != "ndcg" or k <= _hip.METRIC_NDCG_K_MAX)) for kind, k in specs)


def _device_specs(specs):
    from . import _hip
    return [(_hip.METRIC_KINDS[kind], 0 if k is None else k) for kind, k in specs]


def _pairs(stats):
    return [(m, s) for m, s in np.asarray(stats, dtype=np.float64)]


def _host_ranks_from_lists(gt, topk_idx):
    """The int32 CSR with gt's (canonical) pattern: position + 1 of every truth entry in its row of topk_idx - the smaller one for
    an id listed twice - or RANK_ABSENT (what aae_ranks_from_lists computes)."""
    n, K = topk_idx.shape
    data = np.full(gt.nnz, RANK_ABSENT, dtype=np.int32)
    for r in range(n):
        lo, hi = gt.indptr[r], gt.indptr[r + 1]
        if lo == hi:
            continue
        ids = topk_idx[r]
        pos = np.flatnonzero(ids >= 0)
        first_ids, first_at = np.unique(ids[pos], return_index=True)           # (the first place of every id, ids ascending)
        at = np.searchsorted(first_ids, gt.indices[lo:hi])
        hit = (at < first_ids.size) & (first_ids[np.minimum(at, max(first_ids.size - 1, 0))] == gt.indices[lo:hi]) \
            if first_ids.size else np.zeros(hi - lo, dtype=bool)
        data[lo:hi][hit] = pos[first_at[at[hit]]] + 1
    return sp.csr_matrix((data, gt.indices.copy(), gt.indptr.copy()), shape=gt.shape)


def evaluate_topk(ground_truth, topk_idx, metrics, device=None, per_row=False):
    """The bounded ranking metrics ('mrr@k', 'map@k', 'p@k', 'P@1', 'ndcg@k', 'r-prec@k', 'clicks@k') from top-k item ids alone:
    a metric at k only ever looks at the relevance of the k best predictions (RankingMetric above),
    so [(mean, std)] equals evaluate() on the full score matrix.  topk_idx: [n, K] ids, best first,
    K >= the largest k asked for; -1 entries count as irrelevant.
    device: the lists and the truth go up, aae_ranks_from_lists turns them into ranks (RANK_ABSENT for a truth entry outside its
    list) and csrc/rank_metrics.h answers; per_row: the [metrics, n] values instead of [(mean, std)]."""
    gt = sp.csr_matrix(ground_truth)
    topk_idx = np.asarray(topk_idx)
    n, K = topk_idx.shape
    assert gt.shape[0] == n
    specs = _specs(metrics)
    for name, (kind, k) in zip(metrics, specs):
        if k is None or k > K:
            raise ValueError("metric {} needs the full ranking / more than the {} ids given".format(name, K))
    if device is None and not per_row and all(name in METRICS for name in metrics):
        rel = np.zeros((n, K), dtype=np.int64)
        for r in range(n):
            truth = set(gt.indices[gt.indptr[r]:gt.indptr[r + 1]].tolist())
            rel[r] = [1 if int(i) in truth else 0 for i in topk_idx[r]]
        out = []
        for name in metrics:
            metric = METRICS[name]
            rs = rel[:, :metric.k]
            if isinstance(metric, MRR):
                out.append(rm.mean_reciprocal_rank(rs))
            elif isinstance(metric, MAP):
                out.append(rm.mean_average_precision(rs))
            else:
                ps = (rs > 0).mean(axis=1)
                out.append((ps.mean(), ps.std()))
        return out
    gt = gt.copy()
    gt.sum_duplicates()
    gt.sort_indices()
    if n and K and device_metrics_ok(np.diff(gt.indptr), specs, device):
        from . import _hip
        truth = _hip.DeviceCSR(gt, device)
        ids = _hip.upload(np.ascontiguousarray(topk_idx, dtype=np.int32), device)
        ranks = _hip.ranks_from_lists(ids, truth, 0, n, int(gt.nnz))
        got = _hip.rank_metrics(truth.indptr, ranks, _device_specs(specs), per_row=per_row)
        return got if per_row else _pairs(got)
    return evaluate_ranks(_host_ranks_from_lists(gt, topk_idx), metrics, per_row=per_row)


def evaluate_ranks(ranks_csr, metrics, device=None, per_row=False):
    """Every metric of METRICS, bounded or not, from the ranks of the held-out items alone: ranks_csr [n, items] holds, for
    every stored entry, the 1-based rank of that held-out item in the full ranking of its row (predict_ranks).  With a row's
    sorted ranks r_1 < r_2 < ... < r_m:  RR = 1 / r_1,  AP = mean_j (j / r_j);  'mrr@k' / 'map@k' the same over the r_j <= k
    (0 if there are none),  'p@k' = #{r_j <= k} / k;  a row without held-out items scores 0 everywhere, as
    rank_metrics_with_std has it.  [(mean, std)] in float64 with the population std, as evaluate() - no per-row loop.
    Any name metric_spec reads is answered, the challenge's 'ndcg@k', 'r-prec@k', 'clicks@k' (see METRIC_KINDS above) among them;
    a row without held-out items has clicks@k = k / 10 + 1.  Equal ranks order by their place in the row (the lexsort is stable).
    A stored RANK_ABSENT counts towards m and is never <= k.  A rank below 1 raises ValueError.
    device: the ranks go up and csrc/rank_metrics.h answers (the host does where device_metrics_ok says no: the same definitions);
    per_row: the float64 [metrics, n] values instead of [(mean, std)]."""
    R = sp.csr_matrix(ranks_csr)
    n = R.shape[0]
    specs = _specs(metrics)
    if R.nnz and np.asarray(R.data[:R.indptr[-1]]).min() < 1:
        raise ValueError("a rank below 1: ranks are 1-based")
    if n and device_metrics_ok(np.diff(R.indptr), specs, device):
        from . import _hip
        indptr = _hip.upload(np.asarray(R.indptr, dtype=np.int64), device)
        ranks = _hip.upload(np.ascontiguousarray(R.data[:R.indptr[-1]], dtype=np.int32), device)
        got = _hip.rank_metrics(indptr, ranks, _device_specs(specs), per_row=per_row)
        return got if per_row else _pairs(got)
    lengths = np.diff(R.indptr)
    rows = np.repeat(np.arange(n), lengths)
    order = np.lexsort((R.data, rows))                       # (row after row, a row's ranks ascending)
    r = np.asarray(R.data)[order].astype(np.float64)
    j = (np.arange(r.size) - np.asarray(R.indptr, dtype=np.int64)[rows] + 1).astype(np.float64)
    has = lengths > 0
    first = np.zeros(n, dtype=np.float64)                    # r_1 of the rows that have one
    first[has] = r[np.asarray(R.indptr[:-1])[has]]
    m = lengths.astype(np.float64)
    out = []
    for kind, k in specs:
        inside = r != RANK_ABSENT if k is None else r <= k
        if kind == "mrr":
            ok = has & (first <= k) if k is not None else has & (first != RANK_ABSENT)
            per = np.where(ok, 1.0 / np.where(ok, first, 1.0), 0.0)
        elif kind == "map":
            # (the r_j <= k of a sorted row are its first ones: their j are their places among the hits)
            hits = np.bincount(rows[inside], minlength=n).astype(np.float64)
            total = np.bincount(rows[inside], weights=(j / r)[inside], minlength=n)
            per = np.where(hits > 0, total / np.where(hits > 0, hits, 1.0), 0.0)
        elif kind == "p":
            per = np.bincount(rows[inside], minlength=n).astype(np.float64) / k
        elif kind == "r-prec":
            within = r <= np.minimum(m, float(k))[rows]
            per = np.where(has, np.bincount(rows[within], minlength=n).astype(np.float64) / np.where(has, m, 1.0), 0.0)
        elif kind == "clicks":
            ok = has & (first <= k)
            per = np.where(ok, np.floor((np.where(ok, first, 1.0) - 1.0) / 10.0), k / 10.0 + 1.0)
        else:
            # ndcg: the discounts of the hits one by one, a table only as far as min(k, m) of the longest row - whatever k is
            top = max(min(k, int(lengths.max()) if n else 0), 1)
            ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(1 + np.arange(1, top + 1)))))[np.minimum(lengths, k)]
            gain = np.bincount(rows[inside], weights=1.0 / np.log2(1 + r[inside].astype(np.int64)), minlength=n)
            per = np.where(gain > 0, gain / np.where(ideal > 0, ideal, 1.0), 0.0)
        out.append(per)
    return np.asarray(out, dtype=np.float64).reshape(len(specs), n) if per_row else [(v.mean(), v.std()) for v in out]


def reevaluate(gold_file, predictions_file, metrics):
    return evaluate(sp.load_npz(gold_file), np.load(predictions_file), metrics)


def maybe_open(logfile, mode="a"):
    return open(logfile, mode) if logfile else sys.stdout


def maybe_close(fh):
    if fh is not sys.stdout:
        fh.close()


class Evaluation:
    """Year split -> vocabulary -> pruning -> drop `drop` items per test bag -> train/predict/score."""

    def __init__(self, dataset, year, metrics=METRICS, logfile=sys.stdout, logdir=None, topk=True, metrics_on="host"):
        self.dataset, self.year, self.metrics = dataset, year, metrics
        if metrics_on not in ("host", "device"):
            raise ValueError('metrics_on must be "host" or "device", not {!r}'.format(metrics_on))
        # metrics_on="device": on the two ranking branches of __call__ the recommender is asked for the metrics themselves
        # (predict_topk / predict_ranks(..., metrics=names)): lists or ranks stay on the device, csrc/rank_metrics.h turns them
        # into [(mean, std)] and only those doubles come back.  "host" (the default) brings ids or ranks back and scores them
        # with evaluate_topk / evaluate_ranks, as ever.
        self.metrics_on = metrics_on
        self.logfile, self.logdir = logfile, logdir
        # topk: a recommender that can rank on the device (predict_topk: the fused predict -> remove_non_missing -> top-k
        # pass, only [n, k] ids cross PCIe) is asked for its k best items instead of the dense [n, items] score matrix
        # whenever every requested metric is bounded at k (mrr@k, map@k, p@k, P@1: they only ever look at the k best
        # predictions - the numbers are those of the dense pipeline, tests/test_host_gpu.py) and no prediction dump (logdir)
        # is wanted.  With an unbounded name among them (mrr, map) a recommender that offers predict_ranks is asked for the
        # rank of every held-out item in the full ranking instead (evaluate_ranks).  topk=False keeps the reference's dense
        # pipeline for every recommender.
        self.topk = topk
        self.train_set = self.test_set = self.x_test = self.y_test = None

    def setup(self, seed=42, min_elements=1, max_features=None, min_count=None, drop=1):
        self.min_elements, self.max_features, self.min_count, self.drop = min_elements, max_features, min_count, drop
        fh = maybe_open(self.logfile)
        random.seed(seed)
        np.random.seed(seed)
        train_set, test_set = self.dataset.train_test_split(on_year=self.year)
        print("=" * 80, file=fh)
        print("Train:", train_set, file=fh)
        print("Test:", test_set, file=fh)
        print("Next Pruning:\n\tmin_count: {}\n\tmax_features: {}\n\tmin_elements: {}"
              .format(min_count, max_features, min_elements), file=fh)
        train_set = train_set.build_vocab(min_count=min_count, max_features=max_features, apply=True)
        test_set = test_set.apply_vocab(train_set.vocab)
        train_set.prune_(min_elements=min_elements)
        test_set.prune_(min_elements=min_elements)
        print("Train:", train_set, file=fh)
        print("Test:", test_set, file=fh)
        print("Drop parameter:", drop, file=fh)
        noisy, missing = corrupt_sets(test_set.data, drop=drop)
        assert len(noisy) == len(missing) == len(test_set)
        test_set.data = noisy
        print("-" * 80, file=fh)
        maybe_close(fh)
        self.y_test = lists2sparse(missing, test_set.size(1)).tocsr(copy=False)
        self.x_test = lists2sparse(noisy, train_set.size(1)).tocsr(copy=False)
        self.train_set, self.test_set = train_set, test_set
        return self

    def _bounded_k(self):
        """The largest k of the requested metrics when ALL of them are bounded names (<= RANK_K_MAX: what predict_topk ranks), else None."""
        from ._hip import RANK_K_MAX
        ks = []
        for m in self.metrics:
            if isinstance(m, str) and m in BOUNDED_METRICS:
                ks.append(BOUNDED_METRICS[m].k)
                continue
            try:                                    # (a bounded name beyond METRICS: 'ndcg@10', 'r-prec@500', 'mrr@50' ...)
                k = metric_spec(m)[1]
            except ValueError:
                return None
            if k is None:
                return None
            ks.append(k)
        return max(ks) if ks and max(ks) <= RANK_K_MAX else None

    def __call__(self, recommenders, batch_size=None):
        if any(v is None for v in (self.train_set, self.test_set, self.x_test, self.y_test)):
            raise UserWarning("Call .setup() before running the experiment")
        if self.logdir:
            os.makedirs(self.logdir, exist_ok=True)
            with open(os.path.join(self.logdir, "vocab.txt"), "w") as vfh:
                print(*self.train_set.index2token, sep="\n", file=vfh)
            sp.save_npz(os.path.join(self.logdir, "gold"), self.y_test)
        all_results = []
        for rec in recommenders:
            fh = maybe_open(self.logfile)
            print(rec, file=fh)
            maybe_close(fh)
            train_set, test_set = self.train_set.clone(), self.test_set.clone()
            t0 = timer()
            rec.train(train_set)
            fh = maybe_open(self.logfile)
            print("Training took {} seconds.".format(timedelta(seconds=timer() - t0)), file=fh)
            t1 = timer()
            kmax = self._bounded_k()
            if self.topk and kmax is not None and not self.logdir and hasattr(rec, "predict_topk"):
                if self.metrics_on == "device":
                    results = rec.predict_topk(test_set, k=kmax, y_true=self.y_test, metrics=list(self.metrics))
                else:
                    top_ids, _ = rec.predict_topk(test_set, k=kmax)
                print("Prediction took {} seconds.".format(timedelta(seconds=timer() - t1)), file=fh)
                t1 = timer()
                if self.metrics_on != "device":
                    results = evaluate_topk(self.y_test, top_ids, list(self.metrics))
            elif (self.topk and kmax is None and not self.logdir and hasattr(rec, "predict_ranks")
                  and all(isinstance(m, str) and (m in METRICS or _is_metric_name(m)) for m in self.metrics)):
                # an unbounded metric among them (mrr, map: what the reference's drivers ask for): the device ranks every
                # held-out item in the full ranking of its row, nnz(y_test) integers cross PCIe (csrc/rank_full.h)
                if self.metrics_on == "device":
                    results = rec.predict_ranks(test_set, self.y_test, metrics=list(self.metrics))
                else:
                    ranks = rec.predict_ranks(test_set, self.y_test)
                print("Prediction took {} seconds.".format(timedelta(seconds=timer() - t1)), file=fh)
                t1 = timer()
                if self.metrics_on != "device":
                    results = evaluate_ranks(ranks, list(self.metrics))
            else:
                y_pred = rec.predict(test_set)
                y_pred = y_pred.toarray() if sp.issparse(y_pred) else np.asarray(y_pred)
                y_pred = remove_non_missing(y_pred, self.x_test, copy=True)
                print("Prediction took {} seconds.".format(timedelta(seconds=timer() - t1)), file=fh)
                if self.logdir:
                    np.save(os.path.join(self.logdir, repr(rec)), y_pred)
                t1 = timer()
                results = evaluate(self.y_test, y_pred, metrics=self.metrics, batch_size=batch_size)
            print("Evaluation took {} seconds.".format(timedelta(seconds=timer() - t1)), file=fh)
            print("\nResults:\n", file=fh)
            for metric, (mean, std) in zip(self.metrics, results):
                print("- {}: {} ({})".format(metric, mean, std), file=fh)
            print("\nOverall time: {} seconds.".format(timedelta(seconds=timer() - t0)), file=fh)
            print("-" * 79, file=fh)
            maybe_close(fh)
            all_results.append(results)
        return all_results
