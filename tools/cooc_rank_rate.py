#!/usr/bin/env python3
"""The item co-occurrence baseline's predict -> rank: the device route (Countbased.predict_topk: csrc/cooc.h into a
[rows, items] scratch, ranked there by rank_long_dense_kernel, [rows, k] ids to the host) against the host route of the same
commit (Countbased.predict -> toarray -> remove_non_missing -> argtopk, what Evaluation does with a recommender that has no
predict_topk) on a synthetic corpus: documents of 2-12 items from a skewed (1 / rank) popularity over --items, --docs of them
to train on, --rows to rank.  Prints both wall times (median of --repeats, one warm-up each), their ratio, and the same for the
full ranking (predict_ranks against argsort-free host ranks of one held-out item a row).  --scale S multiplies the training
values by the whole number S (C by S^2), which moves the same corpus from the fp32 device route past 2^24 onto the int32 one;
the route taken (Countbased.route) is printed.

    python tools/cooc_rank_rate.py --items 100000 --docs 50000 --rows 500 --k 10
    python tools/cooc_rank_rate.py --items 100000 --docs 50000 --rows 500 --k 10 --scale 256
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
from aaerec.cooc import Countbased
from aaerec.evaluation import argtopk, remove_non_missing

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--docs", type=int, default=50000)
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--scale", type=int, default=1, help="whole-number factor on the training values: C grows by its square")
a = ap.parse_args()
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


class Set:
    def __init__(self, X):
        self.X = X

    def tocsr(self):
        return self.X


def corpus(n, items, seed):
    r = np.random.default_rng(seed)
    ids = np.random.default_rng(7).permutation(items)                  # popularity rank -> id, the same for both sets
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


X, T = corpus(a.docs, a.items, 1), corpus(a.rows, a.items, 2)
X.data *= a.scale
rec = Countbased()
t0 = time.perf_counter()
rec.train(Set(X))
C = rec.cooccurences
print(f"train (scipy X^T X + one upload): {time.perf_counter() - t0:.2f} s; C: {C.nnz} entries, max {int(C.max())}, "
      f"longest row {int(np.diff(C.indptr).max())}; scale {a.scale}; route of the top-{a.k} call: {rec.route(Set(T), a.k)}, "
      f"of the ranks call: {rec.route(Set(T))}", flush=True)
assert rec.route(Set(T), a.k) and rec.route(Set(T)), "the corpus left both device routes: nothing to compare"


def host_topk():
    return argtopk(remove_non_missing(rec.predict(Set(T)).toarray(), T, copy=False), a.k)


t_dev, t_host = wall(lambda: rec.predict_topk(Set(T), k=a.k), a.repeats), wall(host_topk, a.repeats)
print(f"top-{a.k}, {a.rows} rows x {a.items} items: device {med(t_dev):.2f} ms (repeats {[round(x, 2) for x in sorted(t_dev)]}) | "
      f"host {med(t_host):.1f} ms ({[round(x, 1) for x in sorted(t_host)]}) -> host / device = {med(t_host) / med(t_dev):.1f}x", flush=True)

held = np.random.default_rng(3).integers(0, a.items, a.rows)
Y = sp.csr_matrix((np.ones(a.rows), (np.arange(a.rows), held)), shape=T.shape)


def host_ranks():
    S = remove_non_missing(rec.predict(Set(T)).toarray(), T, copy=False)
    return 1 + (S > S[np.arange(a.rows), held][:, None]).sum(axis=1)


t_dev, t_host = wall(lambda: rec.predict_ranks(Set(T), Y), a.repeats), wall(host_ranks, a.repeats)
print(f"full ranking of one held-out item a row: device {med(t_dev):.2f} ms ({[round(x, 2) for x in sorted(t_dev)]}) | "
      f"host {med(t_host):.1f} ms ({[round(x, 1) for x in sorted(t_host)]}) -> host / device = {med(t_host) / med(t_dev):.1f}x", flush=True)
