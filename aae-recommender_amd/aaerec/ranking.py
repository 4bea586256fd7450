"""What every recommender's predict_topk / predict_ranks shares between a test set and its lists or ranks (host only).

The ordering is one rule everywhere: the better score first, THE SMALLER ID AT EQUAL SCORES, known items left out; the rank of a
held-out item is 1 + the number of items ordered before it, a known item behind every rankable one.  The device kernels
(csrc/rank_long.h, rank_full.h) implement it; `host_topk` / `host_ranks` are its reference, which the baselines answer with
where the device route is closed.  The rest is the plumbing around either: the canonical ground truth, the rows of a call a chunk
at a time, and the tails that turn the parts of a chunked call into what `Evaluation` reads: `lists` / `ranks_csr` bring them to
the host, `rank_metrics` leaves them where they are and brings back the metrics alone (csrc/rank_metrics.h).
"""
import numpy as np
import scipy.sparse as sp
import torch


def canonical_truth(y_true, shape, what="the inputs"):
    """The ground truth of a predict_ranks call as a CSR of its own, duplicates summed and indices sorted: the pattern the
    ranks come back in.  shape: the call's (rows, items); what: how the ValueError names the other side."""
    Ys = sp.csr_matrix(y_true, copy=True) if not sp.issparse(y_true) else y_true.tocsr(copy=True)
    if Ys.shape != tuple(shape):
        raise ValueError("the ground truth has shape {}, {} {}".format(Ys.shape, what, tuple(shape)))
    Ys.sum_duplicates()
    Ys.sort_indices()
    return Ys


def chunk_rows(batch_size, cap):
    """Rows per device call of a model handle: what one fused predict -> rank launch takes (`cap`, the handle's *_max_rows:
    hundreds to thousands of rows, dec.lin3 is read once per call), the training batch size otherwise."""
    return max(batch_size, min(cap, 2048))


def row_chunks(n_rows, chunk):
    """(start, rows) of a call over n_rows rows, `chunk` at a time."""
    for start in range(0, n_rows, chunk):
        yield start, min(chunk, n_rows - start)


def lists(parts, k):
    """(ids int32 [n, k], scores float32 [n, k]) on the host from the (ids, scores) device parts of a chunked call."""
    if not parts:
        return np.zeros((0, k), dtype=np.int32), np.zeros((0, k), dtype=np.float32)
    return torch.cat([p[0] for p in parts]).cpu().numpy(), torch.cat([p[1] for p in parts]).cpu().numpy()


def _ranks_csr(data, Ys):
    return sp.csr_matrix((data, Ys.indices.copy(), Ys.indptr.copy()), shape=Ys.shape)


def ranks_csr(parts, Ys):
    """The int32 CSR of ranks with the pattern of the canonical truth Ys from the device parts of a chunked call (CSR order)."""
    return _ranks_csr(torch.cat(parts).cpu().numpy().astype(np.int32, copy=False) if parts else np.zeros(0, dtype=np.int32), Ys)


def rank_metrics(parts, Ys, metrics, k=None, reduce_on="device"):
    """[(mean, std)] per metric name from the device parts of a chunked call and the canonical truth Ys, without a CSR of ranks
    on the host: the parts are concatenated where they are and csrc/rank_metrics.h answers; 16 bytes per metric come back.
    reduce_on="host": the device forms the per-row values alone and [metrics, rows] doubles come back, which numpy reduces as the
    host route reduces its own - the pairs are then the host route's to the bit wherever a row's value is (one held-out item a
    row, the drivers' drop=1: one term, always; longer rows sum their terms in ascending j on both sides, csrc/rank_metrics.h
    ARITHMETIC, except numpy's pairwise mean of eight or more hits), where the device's own reduction agrees to rounding.
    k None: parts are the int32 rank parts of a predict_ranks call (CSR order of Ys).  k given: parts are the (ids, scores) parts
    of a predict_topk call with lists of k ids; aae_ranks_from_lists turns them into ranks, and an unbounded name or one beyond
    k raises the ValueError of evaluation.evaluate_topk.  Where the device route is closed (evaluation.device_metrics_ok: a row
    of more than AAE_METRIC_ROW_MAX held-out items, an ndcg cap beyond 2^20) the host answers under the same definitions.
    A rank below 1 raises ValueError on both routes."""
    from . import _hip, evaluation as ev
    specs = ev._specs(metrics)
    if k is not None:
        for name, (_, cap) in zip(metrics, specs):
            if cap is None or cap > k:
                raise ValueError("metric {} needs the full ranking / more than the {} ids given".format(name, k))
    device = (parts[0] if k is None else parts[0][0]).device if parts else None
    if not parts or not Ys.shape[0] or not ev.device_metrics_ok(np.diff(Ys.indptr), specs, device):
        if k is None:
            return ev.evaluate_ranks(ranks_csr(parts, Ys), metrics)
        return ev.evaluate_topk(Ys, lists(parts, k)[0], metrics)
    if k is None:
        ranks = torch.cat(parts).to(torch.int32).contiguous()
        if ranks.numel() and int(ranks.min()) < 1:
            raise ValueError("a rank below 1: ranks are 1-based")
        indptr = _hip.upload(np.asarray(Ys.indptr, dtype=np.int64), device)
    else:
        truth = _hip.DeviceCSR(Ys, device)
        ids = torch.cat([p[0] for p in parts]).contiguous()
        ranks, indptr = _hip.ranks_from_lists(ids, truth, 0, Ys.shape[0], int(Ys.nnz), k=k), truth.indptr
    if reduce_on == "host":
        return [(v.mean(), v.std()) for v in _hip.rank_metrics(indptr, ranks, ev._device_specs(specs), per_row=True)]
    return ev._pairs(_hip.rank_metrics(indptr, ranks, ev._device_specs(specs)))


# What predict_ranks / predict_topk return, by route and by whether metrics were asked for (metrics=None: ranks / lists as ever)
def finish_ranks(parts, Ys, metrics=None, reduce_on="device"):
    """The device route of a predict_ranks call: the CSR of ranks, or [(mean, std)] of `metrics` (reduce_on: rank_metrics)."""
    return ranks_csr(parts, Ys) if metrics is None else rank_metrics(parts, Ys, metrics, reduce_on=reduce_on)


def finish_lists(parts, k, metrics=None, y_true=None, shape=None, reduce_on="device"):
    """The device route of a predict_topk call: (ids, scores), or [(mean, std)] of `metrics` against y_true [shape]."""
    if metrics is None:
        return lists(parts, k)
    return rank_metrics(parts, list_truth(y_true, shape), metrics, k=k, reduce_on=reduce_on)


def list_truth(y_true, shape):
    if y_true is None:
        raise ValueError("predict_topk(..., metrics=names) needs the ground truth: y_true=")
    return canonical_truth(y_true, shape, "the test set")


def host_finish_ranks(R, metrics=None):
    """The host route of a predict_ranks call (host_ranks) likewise."""
    if metrics is None:
        return R
    from .evaluation import evaluate_ranks
    return evaluate_ranks(R, metrics)


def host_finish_lists(pair, metrics=None, y_true=None, shape=None):
    """The host route of a predict_topk call (host_topk) likewise."""
    if metrics is None:
        return pair
    from .evaluation import evaluate_topk
    return evaluate_topk(list_truth(y_true, shape), pair[0], metrics)


# ---- the host reference ranker -------------------------------------------------------------------------------------------
def _order_row(s, known):
    """Item ids of one row, best first: score descending, the smaller id at equal scores, known items left out."""
    ids = np.lexsort((np.arange(s.size), -s))
    return ids[~np.isin(ids, known)] if len(known) else ids


def host_rows(X, scores, width=None):
    """(row number, its scores float64 [items], its known item ids) over the rows of the canonical CSR X, a bounded block at a
    time.  scores(r0, r1): the [r1 - r0, items] scores of rows [r0, r1) (r1 may lie past the end); width: the columns of the
    widest matrix a block forms, X's own by default."""
    step = max(1, (64 << 20) // (8 * max(1, width or X.shape[1])))
    for r0 in range(0, X.shape[0], step):
        S = np.asarray(scores(r0, r0 + step), dtype=np.float64)
        for j in range(S.shape[0]):
            yield r0 + j, S[j], X.indices[X.indptr[r0 + j]:X.indptr[r0 + j + 1]]


def host_topk(rows, n_rows, k, scaled):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) of the k best new items of every row of `rows` (host_rows);
    id -1 / score 0 behind a row's last rankable item.  scaled(s, best): the min-max-scaled scores of the items `best` of a
    row - the caller's formula, so that it rounds where its device route rounds."""
    ids = np.full((n_rows, k), -1, dtype=np.int32)
    val = np.zeros((n_rows, k), dtype=np.float32)
    for r, s, known in rows:
        best = _order_row(s, known)[:k]
        ids[r, :best.size] = best
        val[r, :best.size] = scaled(s, best)
    return ids, val


def host_ranks(rows, Ys):
    """The int32 CSR of 1-based ranks of the stored entries of the canonical truth Ys over `rows` (host_rows)."""
    data = np.zeros(Ys.nnz, dtype=np.int32)
    ids = np.arange(Ys.shape[1])
    for r, s, known in rows:
        lo, hi = Ys.indptr[r], Ys.indptr[r + 1]
        if lo == hi:
            continue
        s = s.copy()
        s[known] = -np.inf
        for e in range(lo, hi):
            t = Ys.indices[e]
            data[e] = 1 + np.count_nonzero((s > s[t]) | ((s == s[t]) & (ids < t)))
    return _ranks_csr(data, Ys)


class ScratchRanker:
    """A recommender that ranks a dense [rows, items] scratch on the device, the rows of a call chunked to `self.scratch_bytes`.
    A subclass says per ranking method which buffers one call takes and what the call is."""

    def _chunk_rows(self, n_items):
        return max(1, self.scratch_bytes // (4 * ((n_items + 3) & ~3)))

    def _device_chunks(self, n_rows, n_items, buffers, call):
        """[call(start, rows, **buffers)] over the n_rows rows of a call.  buffers(rows): the scratch tensors of the largest
        chunk by keyword, allocated once."""
        chunk = self._chunk_rows(n_items)
        kept = buffers(min(chunk, n_rows))
        return [call(start, rows, **kept) for start, rows in row_chunks(n_rows, chunk)]
