#!/usr/bin/env python3
"""DenoisingAutoEncoder's corruption on its two routes, in one process, alternating (corrupt_draws, aaerec/dae.py):

    torch   the parent commit's route: corrupt='gauss' builds a [rows, items] torch.randn block, scales it and hands it to
            aae_set_input_noise (dense_input_kernel reads it back); corrupt='zeros' thins with values * (rand_like >= p);
    step    the draws of the device generator: aae_set_input_noise_gen (the step draws its noise, csrc/dae_corrupt.h) and
            aae_dae_thin.

1. a corrupt='gauss' training step at --rows x --items, hidden --hidden (C3's shape by default), ms/step over windows of --steps
   steps, the routes taking turns window by window behind a warm-up window each;
2. one whole-corpus thinning of --docs x --items with about --row-nnz entries a row, ms/call over windows of --calls calls.

Every figure is the median of --repeats windows with the windows' spread; a window is a host clock around work that ends in a
device synchronise.  DESIGN.md 4 holds the figures of the commit they were taken on.

    python tools/dae_corrupt_rate.py
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
from aaerec.dae import DenoisingAutoEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--rows", type=int, default=100)
ap.add_argument("--hidden", type=int, default=200)
ap.add_argument("--code", type=int, default=50)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--docs", type=int, default=100000)
ap.add_argument("--row-nnz", type=int, default=60)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--noise-factor", type=float, default=0.2)
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dae_corrupt_rate.py times the GPU: no device, no figure")
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


def corpus(n, items, mean_len, seed):
    r = np.random.default_rng(seed)
    lens = r.integers(mean_len // 2, mean_len + mean_len // 2 + 1, size=n)
    X = sp.csr_matrix((np.ones(int(lens.sum()), dtype=np.float32), r.integers(0, items, size=int(lens.sum())),
                       np.concatenate([[0], np.cumsum(lens)])), shape=(n, items))
    X.sum_duplicates()
    X.sort_indices()
    X.data[:] = 1.0
    return X


def windows(routes, reps):
    """routes: name -> fn(); one warm-up call each, then `reps` rounds in which the routes take turns -> name -> [ms]."""
    out = {name: [] for name in routes}
    for fn in routes.values():
        fn()
    for _ in range(reps):
        for name, fn in routes.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def line(what, per, times):
    print(what + ": " + " | ".join("{} {:.4f} ms ({})".format(name, med(t) / per, ", ".join("%.4f" % (x / per) for x in sorted(t)))
                                   for name, t in times.items()), flush=True)


# ---- 1. the corrupt='gauss' step ---------------------------------------------------------------------------------------------
X = corpus(20 * a.rows, a.items, 20, 1)
models = {}
for draws in ("torch", "step"):
    m = DenoisingAutoEncoder(n_hidden=a.hidden, n_code=a.code, batch_size=a.rows, corrupt="gauss", noise_factor=a.noise_factor,
                             verbose=False, device=a.device, rng_mode="device", seed=7, corrupt_draws=draws)
    torch.manual_seed(0)
    m._build(a.items, 0)
    m.train()
    models[draws] = (m, _hip.DeviceCSR(X, m.hip.device))


def steps_of(draws):
    m, csr = models[draws]

    def run():
        for s in range(a.steps):
            m._run_step(csr, (s % 20) * a.rows, a.rows, None, None)
    return run


print(f"corrupt='gauss' step: {a.rows} rows x {a.items} items, hidden {a.hidden}, code {a.code}, noise_factor {a.noise_factor}; "
      f"median of {a.repeats} windows of {a.steps} steps, routes alternating", flush=True)
line("ms/step", a.steps, windows({d: steps_of(d) for d in models}, a.repeats))
for m, _ in models.values():
    assert np.isfinite(m.hip.losses()[0])

# ---- 2. thinning a whole corpus ----------------------------------------------------------------------------------------------
hip = models["step"][0].hip
big = _hip.DeviceCSR(corpus(a.docs, a.items, a.row_nnz, 2), hip.device)
p = a.noise_factor


def thin_torch():
    for _ in range(a.calls):
        out = big.values * (torch.rand_like(big.values) >= p).to(big.values.dtype)
    return out


def thin_step():
    for _ in range(a.calls):
        out = hip.dae_thin(big, p).values
    return out


kept = {name: float((fn() != 0).float().mean()) for name, fn in (("torch", thin_torch), ("step", thin_step))}
print(f"thinning {a.docs} x {a.items}, {big.values.numel()} entries, p = {p}; kept share {kept}; median of {a.repeats} windows of "
      f"{a.calls} calls, routes alternating", flush=True)
line("ms/call", a.calls, windows({"torch": thin_torch, "step": thin_step}, a.repeats))
