#!/usr/bin/env python3
"""What turning held-out ranks or top-k lists into metrics costs, on the host and on the device, on the same synthetic data:

    ranks host    evaluation.evaluate_ranks(R, names): NumPy over the CSR of ranks;
    ranks device  evaluation.evaluate_ranks(R, names, device=...): the ranks uploaded, csrc/rank_metrics.h, [names, 2] doubles back;
    lists host    evaluation.evaluate_topk(Y, ids, names): for the names of METRICS the per-row Python loop it always was;
    lists device  evaluation.evaluate_topk(Y, ids, names, device=...): ids and truth uploaded, aae_ranks_from_lists, the same
                  kernels, [names, 2] doubles back;
    resident      ranking.rank_metrics on ranks / lists that are already on the device, as a recommender's predict_ranks /
                  predict_topk(metrics=names) has them: no upload of ranks or ids, only the truth's row pointers (or the truth).

Two sizes: --rows-lists rows with lists of --k ids and 1 to 20 held-out items each, and --rows-single rows with one held-out
item and lists of 10.  The ranks of a size are those its lists imply (RANK_ABSENT outside the list), so every route of a size
scores the same rows.  Every figure is the median wall time of --repeats runs behind one warm-up, copies included.

    python tools/metric_rate.py --rows-lists 10000 --k 500 --rows-single 100000
"""
import argparse
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import scipy.sparse as sp
import torch
from aaerec import _hip, evaluation as E, ranking

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--rows-lists", type=int, default=10000)
ap.add_argument("--k", type=int, default=500)
ap.add_argument("--rows-single", type=int, default=100000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


def case(n, K, most, seed):
    """(ids int32 [n, K], truth CSR [n, items]): a row's list is K items drawn at random, its 1 .. most held-out items half from the
    list, half from anywhere."""
    r = np.random.default_rng(seed)
    ids = r.integers(0, a.items, size=(n, K)).astype(np.int32)           # (an id drawn twice counts at its first place)
    rows = []
    for i in range(n):
        m = int(r.integers(1, most + 1))
        inside = r.choice(ids[i], size=min(K, (m + 1) // 2), replace=False)
        rows.append(np.unique(np.concatenate([inside, r.integers(0, a.items, size=m - inside.size)])))
    indptr = np.concatenate([[0], np.cumsum([x.size for x in rows])]).astype(np.int64)
    Y = sp.csr_matrix((np.ones(indptr[-1]), np.concatenate(rows).astype(np.int32), indptr), shape=(n, a.items))
    return ids, Y


def timed(fn):
    def once():
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    once()
    runs = [once() for _ in range(a.repeats)]
    return med([t for t, _ in runs]), runs[-1][1]


def report(label, n, K, most, names, seed):
    ids, Y = case(n, K, most, seed)
    R = E._host_ranks_from_lists(Y, ids)
    print("{}: {} rows, lists of {}, {} held-out items, {} metrics".format(label, n, K, Y.nnz, len(names)))
    t_rh, ref = timed(lambda: E.evaluate_ranks(R, names))
    print("  ranks host     {:9.3f} ms".format(t_rh * 1e3))
    old = [nm for nm in names if nm in E.METRICS]
    t_lh, _ = timed(lambda: E.evaluate_topk(Y, ids, old))
    print("  lists host     {:9.3f} ms   ({} names of METRICS: the per-row loop)".format(t_lh * 1e3, len(old)))
    t_ln, _ = timed(lambda: E.evaluate_topk(Y, ids, names))
    print("  lists host     {:9.3f} ms   (all names: through host ranks)".format(t_ln * 1e3))
    if not torch.cuda.is_available():
        print("  no device: the device routes are not timed")
        return
    t_rd, got = timed(lambda: E.evaluate_ranks(R, names, device=a.device))
    print("  ranks device   {:9.3f} ms   (upload of {} ranks included)".format(t_rd * 1e3, R.nnz))
    t_ld, got_l = timed(lambda: E.evaluate_topk(Y, ids, names, device=a.device))
    print("  lists device   {:9.3f} ms   (upload of [{}, {}] ids and the truth included)".format(t_ld * 1e3, n, K))
    d_ranks = [_hip.upload(np.ascontiguousarray(R.data, dtype=np.int32), a.device)]
    d_lists = [(_hip.upload(ids, a.device), None)]
    Ys = ranking.canonical_truth(Y, Y.shape)
    t_rr, _ = timed(lambda: ranking.rank_metrics(d_ranks, Ys, names))
    t_lr, _ = timed(lambda: ranking.rank_metrics(d_lists, Ys, names, k=K))
    print("  resident ranks {:9.3f} ms\n  resident lists {:9.3f} ms".format(t_rr * 1e3, t_lr * 1e3))
    # (a difference is taken relative to the larger of the metric's mean and std: where every row scores the same, the std is
    #  rounding noise around 0 on either side and a ratio of two such numbers says nothing)
    def worst(pairs):
        diffs = [(max(abs(g[0] - w[0]), abs(g[1] - w[1])) / max(abs(w[0]), abs(w[1]), 1e-300), nm) for g, w, nm in zip(pairs, ref, names)]
        return max(diffs)
    print("  largest difference from the host's (mean, std), relative to the metric's size: ranks {:.2e} ({}), lists {:.2e} ({})".format(
        *worst(got), *worst(got_l)))


bounded = lambda K: [nm for nm in list(E.BOUNDED_METRICS) + list(E.CHALLENGE_METRICS) if E.metric_spec(nm)[1] <= K]    # noqa: E731
report("lists", a.rows_lists, a.k, 20, bounded(a.k), 1)
report("single", a.rows_single, 10, 1, bounded(10), 2)
