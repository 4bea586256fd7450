#!/usr/bin/env python3
"""The truncated-SVD baseline's fit: SVDRecommender(fit="device") - the randomized range finder with its sparse products on the
device (csrc/sptrans.h, aae_spmm_f32), torch.linalg.qr there, the SVD of the small matrix B on the host - against fit="host"
(scikit-learn's TruncatedSVD.fit) of the same commit, on cooc_rank_rate.py's synthetic corpus: --rows documents of 2-12 items
from a skewed (1 / rank) popularity over --items.  Prints the wall seconds of fit() for both at every --dims (one run each behind
one small warm-up fit that loads the solver libraries), the device time broken down into upload, transpose, products,
orthonormalisation, download, host SVD and explained variance (each phase closed by a synchronisation), and how far the two
fits' singular values are apart.

    python tools/svd_fit_rate.py --items 100000 --rows 200000 --dims 100 1000
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
from aaerec.lowrank import SVDRecommender

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--dims", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--skip-host", action="store_true", help="time the device fit alone")
a = ap.parse_args()


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


X = corpus(a.rows, a.items, 1)
print(f"{a.rows} rows x {a.items} items, {X.nnz} entries, longest column {int(np.bincount(X.indices).max())}", flush=True)
SVDRecommender(8, fit="device", random_state=a.seed).fit(corpus(2000, 500, 2))       # warm-up: solver libraries, allocator
for dims in a.dims:
    dev = SVDRecommender(dims, fit="device", random_state=a.seed)
    dev.fit_seconds = {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    dev.fit(X)
    torch.cuda.synchronize(); t_dev = time.perf_counter() - t0
    assert dev.fitted_on == "device", "the device fit fell back to the host: nothing to compare"
    phases = ", ".join(f"{k} {v:.3f}" for k, v in dev.fit_seconds.items())
    print(f"dims {dims}: fit='device' {t_dev:.2f} s  ({phases}; orthonormalisation on the {'host' if dev.qr_on_host else 'device'})", flush=True)
    if a.skip_host:
        continue
    host = SVDRecommender(dims, fit="host", device=None, random_state=a.seed)
    t0 = time.perf_counter()
    host.fit(X)
    t_host = time.perf_counter() - t0
    s_h, s_d = host.svd.singular_values_, dev.svd.singular_values_
    print(f"dims {dims}: fit='host' {t_host:.2f} s -> host / device = {t_host / t_dev:.2f}x; "
          f"max |sigma_dev - sigma_host| / sigma_1 = {np.abs(s_d - s_h).max() / s_h[0]:.2e}", flush=True)
