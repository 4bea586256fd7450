#!/usr/bin/env python3
"""The truncated-SVD baseline's predict -> rank: the device route (aaerec.lowrank.SVDRecommender.predict_topk / predict_ranks:
csrc/lowrank.h projects, the fp32 GEMM reconstructs into a [rows, items] scratch, the dense rank kernels rank there, [rows, k]
ids or one rank a row go to the host) against the reference's route on the same box (predict -> remove_non_missing -> argtopk,
what Evaluation does with a recommender that has no predict_topk) at --items items, for every --dims and every --k, plus the
full ranking of one held-out item a row.  The model is not fitted - that is scikit-learn's on either route and not what is
timed: components_ is a random [dims, items] matrix with a power-law spectrum.  Rows: bags of 2-12 items from a skewed (1 /
rank) popularity.  Prints wall times (median of --repeats, one warm-up each) and rows/s of both routes.

    python tools/svd_rank_rate.py --items 100000 --rows 500 --dims 100 1000 --k 10 500
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
from aaerec.evaluation import argtopk, remove_non_missing
from aaerec.lowrank import SVDRecommender

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--dims", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--k", type=int, nargs="+", default=[10, 500])
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


class Set:
    def __init__(self, X):
        self.X = X

    def tocsr(self):
        return self.X


def corpus(n, items, seed):
    r = np.random.default_rng(seed)
    ids = np.random.default_rng(7).permutation(items)
    p = 1.0 / (np.arange(items) + 10.0)
    lens = r.integers(2, 13, size=n)
    draws = ids[r.choice(items, size=int(lens.sum()), p=p / p.sum())]
    X = sp.csr_matrix((np.ones(draws.size), draws, np.concatenate([[0], np.cumsum(lens)])), shape=(n, items))
    X.sum_duplicates()
    X.data[:] = 1.0
    return X


def wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(what, t_dev, t_host):
    d, h = med(t_dev), med(t_host)
    print(f"{what}: device {d:.2f} ms = {a.rows / d * 1e3:.0f} rows/s ({[round(x, 2) for x in sorted(t_dev)]}) | "
          f"host {h:.1f} ms = {a.rows / h * 1e3:.0f} rows/s ({[round(x, 1) for x in sorted(t_host)]}) -> host / device = {h / d:.1f}x", flush=True)


T = corpus(a.rows, a.items, 2)
held = np.random.default_rng(3).integers(0, a.items, a.rows)
Y = sp.csr_matrix((np.ones(a.rows), (np.arange(a.rows), held)), shape=T.shape)
for dims in a.dims:
    rec = SVDRecommender(dims)
    rec.svd.components_ = np.random.default_rng(dims).standard_normal((dims, a.items)) * ((1.0 + np.arange(dims)) ** -1.5)[:, None]
    rec.n_classes = a.items
    t0 = time.perf_counter()
    assert rec.on_device(max(a.k)), "no device route: nothing to compare"
    print(f"dims {dims}, {a.rows} rows x {a.items} items; table upload {time.perf_counter() - t0:.2f} s", flush=True)
    for k in a.k:
        line(f"  top-{k}", wall(lambda: rec.predict_topk(Set(T), k=k), a.repeats),
             wall(lambda: argtopk(remove_non_missing(rec.predict(Set(T)), T, copy=False), k), a.repeats))

    def host_ranks():
        S = remove_non_missing(rec.predict(Set(T)), T, copy=False)
        return 1 + (S > S[np.arange(a.rows), held][:, None]).sum(axis=1)

    line("  full ranking of one held-out item a row", wall(lambda: rec.predict_ranks(Set(T), Y), a.repeats), wall(host_ranks, a.repeats))
