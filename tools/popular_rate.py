#!/usr/bin/env python3
"""The most-popular baseline's train() and predict -> rank on a synthetic corpus: documents of 2-12 items from a skewed (1 / rank)
popularity over --items, --docs of them to train on, --rows to rank.  Three routes for every ranking call:

    device  MostPopular(device=...).predict_topk / predict_ranks: csrc/popular.h over the one item order, [rows, k] ids or
            nnz(truth) ranks to the host;
    host    the host route of the same commit, MostPopular(device=None): ranking.host_topk / host_ranks over the broadcast counts;
    dense   what Evaluation does with a recommender that has no predict_topk / predict_ranks - the parent commit's pipeline
            for this baseline: predict -> remove_non_missing -> argtopk (for the ranks: a count over the masked dense matrix).

and train() with the columns summed on the host (scipy, then one upload) and on the device (the matrix uploaded as int32 CSR,
aae_pop_counts), the order built on the device either way.  Every figure is the median wall time of --repeats runs behind one
warm-up.  The two train() figures decide aaerec.popular.AUTO_COUNTS_ON_DEVICE.

    python tools/popular_rate.py --items 100000 --docs 50000 --rows 500
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
from aaerec.popular import MostPopular
from aaerec.evaluation import argtopk, remove_non_missing

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--docs", type=int, default=50000)
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 500])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


class Set:
    def __init__(self, X):
        self.X = X

    def tocsr(self):
        return self.X

    def size(self):
        return self.X.shape


def corpus(n, items, seed):
    r = np.random.default_rng(seed)
    ids = np.random.default_rng(7).permutation(items)                  # popularity rank -> id, the same for both sets
    p = 1.0 / (np.arange(items) + 10.0)
    lens = r.integers(2, 13, size=n)
    draws = ids[r.choice(items, size=int(lens.sum()), p=p / p.sum())]
    X = sp.csr_matrix((np.ones(draws.size), draws, np.concatenate([[0], np.cumsum(lens)])), shape=(n, items))
    X.sum_duplicates()
    X.sort_indices()
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


def line(what, **routes):
    parts = ["{} {:.2f} ms ({})".format(name, med(t), ", ".join("%.2f" % x for x in sorted(t))) for name, t in routes.items()]
    print(what + ": " + " | ".join(parts), flush=True)


X, T = corpus(a.docs, a.items, 1), corpus(a.rows, a.items, 2)
print(f"{a.items} items, {a.docs} training rows ({X.nnz} entries), {a.rows} test rows of 2-12 items; median of {a.repeats} behind a warm-up",
      flush=True)

by_host, by_dev = MostPopular(device=a.device, count="host"), MostPopular(device=a.device, count="device")
line("train(), upload included", host_counts=wall(lambda: by_host.train(Set(X)), a.repeats),
     device_counts=wall(lambda: by_dev.train(Set(X)), a.repeats))
host = MostPopular(device=None)
host.train(Set(X))
assert by_dev.route(Set(T), max(a.ks)) == "device" and by_dev.route(Set(T)) == "device" and host.route(Set(T), 10) is None
np.testing.assert_array_equal(np.asarray(by_dev.most_popular), np.asarray(host.most_popular))


def dense_scores():
    return remove_non_missing(np.asarray(host.predict(Set(T))), T, copy=True)


for k in a.ks:
    got, _ = by_dev.predict_topk(Set(T), k=k)
    np.testing.assert_array_equal(got, host.predict_topk(Set(T), k=k)[0])
    line(f"predict_topk, k = {k}", device=wall(lambda: by_dev.predict_topk(Set(T), k=k), a.repeats),
         host=wall(lambda: host.predict_topk(Set(T), k=k), a.repeats),
         dense=wall(lambda: argtopk(dense_scores(), k), a.repeats))

held = np.random.default_rng(3).integers(0, a.items, a.rows)
Y = sp.csr_matrix((np.ones(a.rows), (np.arange(a.rows), held)), shape=T.shape)
np.testing.assert_array_equal(by_dev.predict_ranks(Set(T), Y).data, host.predict_ranks(Set(T), Y).data)


def dense_ranks():
    S = dense_scores()
    return 1 + (S > S[np.arange(a.rows), held][:, None]).sum(axis=1)


line("predict_ranks, one held-out item a row", device=wall(lambda: by_dev.predict_ranks(Set(T), Y), a.repeats),
     host=wall(lambda: host.predict_ranks(Set(T), Y), a.repeats), dense=wall(dense_ranks, a.repeats))
