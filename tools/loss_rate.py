#!/usr/bin/env python3
"""The held-out loss at the headline shape (C3: 100 000 items, hidden 200, LR_ROWS = 1 000 test rows): rows/s of
1. AutoEncoder.eval_loss on the fused route (aae_predict_loss: the loss epilogue of the rank kernel, no score matrix),
2. the same on the dense route (a second model created under NO_RANK_FUSED with the same parameters: logits into the
   [max_batch][n_items] scratch, one workgroup per row),
3. predict() + F.binary_cross_entropy(pred + 1e-12, X + 1e-12) on the host - the only route before eval_loss,
and predict() alone beside them.  One process, one device, the same rows for all: each route LR_WARMUP untimed calls, then
LR_REPEATS timed ones (wall time around a call that ends with its number on the host), median / min / max.  The VAE's
eval_loss (aae_vae_predict_loss: + the KL rows) is timed the same way on a VAE of the same widths."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import torch
from aaerec import _hip
from aaerec.aae import AutoEncoder
from aaerec.vae import VAE
from tools.synth import init_params, throughput_corpus

N, h, c, B = int(os.environ.get("LR_ITEMS", 100000)), int(os.environ.get("LR_HIDDEN", 200)), 50, 100
ROWS, REPS, WARM = int(os.environ.get("LR_ROWS", 1000)), int(os.environ.get("LR_REPEATS", 7)), int(os.environ.get("LR_WARMUP", 2))


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return sorted(t)


def line(name, t, value):
    m = t[len(t) // 2]
    print(f"{name:46s} median {m * 1e3:9.2f} ms = {ROWS / m:10.0f} rows/s   (min {t[0] * 1e3:.2f}, max {t[-1] * 1e3:.2f} ms; "
          f"{REPS} calls behind {WARM})   value {value!r}", flush=True)
    return m


def model(dense):
    if dense:
        _hip.set_option("NO_RANK_FUSED", "1")
    try:
        m = AutoEncoder(n_hidden=h, n_code=c, n_epochs=1, batch_size=B, lr=0.001, verbose=False, seed=1)
        m.fit(X)                       # (builds the handle for these rows; one epoch)
    finally:
        _hip.set_option("NO_RANK_FUSED", None)
    p = init_params(N, h, c, seed=3)
    p["dec.lin3.weight"] = p["dec.lin3.weight"] * 8.0
    m.hip.load_params(p)
    return m


def host_route(m):
    pred = torch.as_tensor(m.predict(X))
    T = torch.as_tensor(np.asarray(X.todense(), dtype=np.float32))
    return float(torch.nn.functional.binary_cross_entropy(pred + 1e-12, T + 1e-12).item())


X = throughput_corpus(ROWS, N, seed=1234).tocsr()
X.data[:] = 1.0
print(f"{N} items, hidden {h}, code {c}, max_batch {B}, {ROWS} rows ({X.nnz / ROWS:.1f} items a row) on {torch.cuda.get_device_name(0)}", flush=True)
fused, dense = model(False), model(True)
print(f"loss_max_rows: fused handle {fused.hip.loss_max_rows()}, dense handle {dense.hip.loss_max_rows()}", flush=True)
t_f = line("eval_loss, fused route (aae_predict_loss)", timed(lambda: fused.eval_loss(X)), fused.eval_loss(X))
t_d = line("eval_loss, dense route (NO_RANK_FUSED)", timed(lambda: dense.eval_loss(X)), dense.eval_loss(X))
t_p = line("predict() alone (scores to the host)", timed(lambda: fused.predict(X)), None)
t_h = line("predict() + torch BCE on the host", timed(lambda: host_route(fused)), host_route(fused))
print(f"  -> the host route takes {t_h / t_f:.1f}x the fused route, the dense route {t_d / t_f:.1f}x", flush=True)
v = VAE(N, N, n_hidden=h, n_code=c, batch_size=B, verbose=False, seed=1)
line("VAE.eval_loss (aae_vae_predict_loss)", timed(lambda: v.eval_loss(X)), v.eval_loss(X))
