#!/usr/bin/env python3
"""IRGAN's phases on a synthetic problem, device route and host route of the same commit: --users users over --items items, 2 to 12
items each (skewed popularity), batch_size 16, emb_dim 5.  Timed, each the median wall time of --repeats runs behind one warm-up:

    generate_for_d   one pass over every user with positives (the negatives of every line);
    D steps          --steps consecutive D steps (the first batches of one epoch);
    G steps          --steps consecutive G steps (the first users), draws from the keyed generator;
    predict_topk     --rows test rows, k = 10.

The host route is aaerec/irgan.py's NumPy restatement in float32 with the same sampler.  Its generate_for_d is timed over the
first --host-users users only (it costs milliseconds per user) and printed as such.  A phase that was not run says NOT MEASURED.

    python tools/irgan_rate.py --users 10000 --items 100000
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
from aaerec import _hip, irgan as I

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=10000)
ap.add_argument("--items", type=int, default=100000)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--rows", type=int, default=500)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--host-users", type=int, default=200)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


def wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(what, **routes):
    parts = []
    for name, t in routes.items():
        parts.append("{} NOT MEASURED".format(name) if t is None else
                     "{} {:.2f} ms ({})".format(name, med(t), ", ".join("%.2f" % x for x in sorted(t))))
    print(what + ": " + " | ".join(parts), flush=True)


rng = np.random.default_rng(1)
p = 1.0 / (np.arange(a.items) + 10.0)
ids = np.random.default_rng(7).permutation(a.items)
X = {u: np.unique(ids[rng.choice(a.items, size=int(rng.integers(2, 13)), p=p / p.sum())]).tolist() for u in range(a.users)}


def model(device, X):
    m = I.IRGAN(a.users, a.items, batch_size=16, emb_dim=5, lr=0.001, verbose=False, device=device, seed=11)
    m._set_positives(X)
    m._engine = m._make_engine(*m._init)
    return m


dev = model(a.device, X)
assert dev.route() == "device"
e = dev._engine
n_lines = int(dev._lines.shape[0])
steps = min(a.steps, (n_lines + 15) // 16, len(dev._order))
print(f"{a.users} users, {a.items} items, {n_lines} lines; {steps} steps a phase; median of {a.repeats} behind a warm-up", flush=True)
host = hx = None
if not a.no_host:
    hx = {u: X[u] for u in list(X)[:a.host_users]}
    host_small = model(None, hx)            # generate_for_d over the first users only
    host = model(None, X)
    host._engine.set_lines(dev._lines)

line("generate_for_d, every user", device=wall(lambda: e.sample_neg(dev, dev.seed, 0), a.repeats))
line(f"generate_for_d, the first {a.host_users} users",
     device=wall(lambda: _hip.irgan_sample_neg(e.G, e.order[:a.host_users], e.line_off[:a.host_users + 1], e.max_pos, I.TEMPERATURE, 11, 0,
                                               e.lines, e.scratch), a.repeats),
     host=None if a.no_host else wall(lambda: host_small._engine.sample_neg(host_small, 11, 0), a.repeats))
if host is not None:
    host._engine.set_lines(e.lines.cpu().numpy())
line(f"{steps} D steps", device=wall(lambda: _hip.irgan_d_steps(e.D, e.lines, 16, steps, dev.lr, I.MOMENTUM, dev.lam_d, e.scratch), a.repeats),
     host=None if a.no_host else wall(lambda: I.host_d_steps(host._engine.D, host._engine.lines, 16, dev.lr, I.MOMENTUM, dev.lam_d,
                                                             n_steps=steps), a.repeats))
order = dev._order[:steps]
counter = [0]


def g_device():
    counter[0] += 1
    e.g_steps(dev, order, None, 11, counter[0], False)


def g_host():
    counter[0] += 1
    host._engine.g_steps(host, order, None, 11, counter[0], False)


line(f"{steps} G steps", device=wall(g_device, a.repeats), host=None if a.no_host else wall(g_host, a.repeats))
rows = np.arange(min(a.rows, a.users))
known = sp.csr_matrix((np.ones(sum(len(X[u]) for u in rows)), np.concatenate([X[u] for u in rows]),
                       np.concatenate([[0], np.cumsum([len(X[u]) for u in rows])])), shape=(rows.size, a.items))
line(f"predict_topk, {rows.size} rows, k = 10", device=wall(lambda: dev.predict_topk(rows, known, k=10), a.repeats),
     host=None if a.no_host else wall(lambda: host.predict_topk(rows, known, k=10), a.repeats))
