#!/usr/bin/env python3
"""The random baseline's predict -> rank on synthetic test rows: --rows bags of 2-12 known items over --items.  Three routes for
every ranking call:

    device     RandomBaseline(seed, device=...).predict_topk / predict_ranks: csrc/randrank.h regenerates the draws per pass,
               [rows, k] ids or nnz(truth) ranks to the host;
    host       the host route of the same commit, RandomBaseline(seed, device=None): aaerec.randbase.draw_scores into
               ranking.host_topk / host_ranks, a block of rows at a time;
    reference  the reference's way: numpy.random.rand(rows, items) in float64 -> remove_non_missing -> argtopk (for the ranks: a
               count over the masked dense matrix).  Other numbers than the two routes above - only the time is compared.

Every figure is the median wall time of --repeats runs behind one warm-up.  One line per size and call; DESIGN 3.4i keeps them.

    python tools/random_rate.py --items 5000 100000 --rows 500
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
from aaerec.randbase import RandomBaseline
from aaerec.evaluation import argtopk, remove_non_missing

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, nargs="+", default=[5000, 100000])
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--ks", type=int, nargs="+", default=[10, 500])
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--seed", type=int, default=7)
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


def rows_of(n, items, seed):
    r = np.random.default_rng(seed)
    lens = r.integers(2, 13, size=n)
    X = sp.csr_matrix((np.ones(int(lens.sum())), r.integers(0, items, size=int(lens.sum())), np.concatenate([[0], np.cumsum(lens)])),
                      shape=(n, items))
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


print(f"{a.rows} test rows of 2-12 known items; median of {a.repeats} behind a warm-up", flush=True)
for items in a.items:
    T = rows_of(a.rows, items, 2)
    dev, host = RandomBaseline(seed=a.seed, device=a.device), RandomBaseline(seed=a.seed, device=None)
    assert dev.route(Set(T), min(max(a.ks), items)) == "device" and dev.route(Set(T)) == "device" and host.route(Set(T), 10) is None

    def dense_scores():
        return remove_non_missing(np.random.rand(*T.shape), T, copy=True)

    for k in a.ks:
        if k > items:
            continue
        got = dev.predict_topk(Set(T), k=k)
        want = host.predict_topk(Set(T), k=k)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        line(f"{items} items, predict_topk, k = {k}", device=wall(lambda: dev.predict_topk(Set(T), k=k), a.repeats),
             host=wall(lambda: host.predict_topk(Set(T), k=k), a.repeats),
             reference=wall(lambda: argtopk(dense_scores(), k), a.repeats))

    held = np.random.default_rng(3).integers(0, items, a.rows)
    Y = sp.csr_matrix((np.ones(a.rows), (np.arange(a.rows), held)), shape=T.shape)
    np.testing.assert_array_equal(dev.predict_ranks(Set(T), Y).data, host.predict_ranks(Set(T), Y).data)

    def dense_ranks():
        S = dense_scores()
        return 1 + (S > S[np.arange(a.rows), held][:, None]).sum(axis=1)

    line(f"{items} items, predict_ranks, one held-out item a row", device=wall(lambda: dev.predict_ranks(Set(T), Y), a.repeats),
         host=wall(lambda: host.predict_ranks(Set(T), Y), a.repeats), reference=wall(dense_ranks, a.repeats))
