#!/usr/bin/env python3
"""The item co-occurrence baseline's train(): C = X^T X (and C <- C . C for --order n) built on the device by the exact int32
sparse product of csrc/spgemm.h (Countbased(build="device"): X and X^T up, Count, scan, Fill, C stays in HBM) against the host
build of the same commit (build="host": scipy's product, canonicalised, one upload) on cooc_rank_rate.py's synthetic corpus:
documents of 2-12 items from a skewed (1 / rank) popularity over --items, --docs of them.  Prints the wall time of train() for
both (median of --repeats behind one warm-up, every value), nnz(C), the rows each kernel takes per product, and whether the
two matrices are equal.

    python tools/cooc_build_rate.py --items 100000 --docs 50000 --order 1
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
from aaerec import _hip
from aaerec.cooc import Countbased, device_build_ok

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--docs", type=int, default=50000)
ap.add_argument("--order", type=int, default=1)
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
    ids = np.random.default_rng(7).permutation(items)                  # popularity rank -> id
    p = 1.0 / (np.arange(items) + 10.0)
    lens = r.integers(2, 13, size=n)
    draws = ids[r.choice(items, size=int(lens.sum()), p=p / p.sum())]
    X = sp.csr_matrix((np.ones(draws.size), draws, np.concatenate([[0], np.cumsum(lens)])), shape=(n, items))
    X.sum_duplicates()
    X.data[:] = 1.0
    return X


def wall(rec, reps):
    rec.train(Set(X))
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        rec.train(Set(X))
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return out


X = corpus(a.docs, a.items, 1)
assert device_build_ok(X), "the corpus left the guard of the device build: nothing to compare"
host, dev = Countbased(a.order, build="host"), Countbased(a.order, build="device")
t_host, t_dev = wall(host, a.repeats), wall(dev, a.repeats)
assert dev.built_on == "device" and dev._cooc is None
print(f"train(), {a.docs} documents x {a.items} items ({X.nnz} entries), order {a.order}: device {med(t_dev):.1f} ms "
      f"(repeats {[round(x, 1) for x in sorted(t_dev)]}) | host {med(t_host):.1f} ms ({[round(x, 1) for x in sorted(t_host)]}) "
      f"-> host / device = {med(t_host) / med(t_dev):.2f}x", flush=True)

A, B = _hip.DeviceCooc(X.T.tocsr(), "cuda:0"), _hip.DeviceCooc(X, "cuda:0")
for o in range(a.order):
    u = _hip.spgemm_bound(A, B)
    C = _hip.spgemm_i32(A, B)
    print(f"product {o + 1}: {int((u <= _hip.SPGEMM_HASH_PRODUCTS).sum())} hash rows, {int((u > _hip.SPGEMM_HASH_PRODUCTS).sum())} tile rows, "
          f"{int(u.sum())} products (largest row {int(u.max())}) -> nnz(C) = {C.nnz}, max {C.abs_max()}, "
          f"longest row {int(C.indptr.diff().max())}", flush=True)
    A = B = C
Ch, Cd = host.cooccurences, dev.cooccurences
same = np.array_equal(Ch.indptr, Cd.indptr) and np.array_equal(Ch.indices, Cd.indices) and np.array_equal(Ch.data, Cd.data)
print(f"device C == host C (indptr, indices, values): {same}", flush=True)
assert same
