#!/usr/bin/env python3
"""predict -> rank at the headline shape (C3: 100 000 items, hidden 200): docs/s of the library call alone on a resident
test corpus (aae_predict_topk over `rows` documents per call, launch to completion) and of
AdversarialAutoEncoder.predict_topk (host loop, [n, k] results copied to the host) - fused path and, with
AAE_NO_RANK_FUSED=1 in a second process, the r1-r3 two-kernel path.  Per-call HIP-event time of the rank kernel itself
(AAE_K_RANK) against its floors: 2 rows N (h+1) flop on the matrix cores, 4 N (h+1) bytes of dec.lin3 from HBM.
RR_K=500 (any k up to 1024) ranks long lists (csrc/rank_long.h) and adds, per rows-per-call, the median of RR_REPEATS timed
regions of that call, of the k = 32 call on the same rows, and of the only other way to the same lists: predict() per
max_batch rows, the dense matrix copied to the host, remove_non_missing + argtopk there.
RR_MODE=ranks times the full ranking instead (csrc/rank_full.h): predict_ranks with RR_TRUTH held-out items per row (default
1), ranks on the host, per rows-per-call against the k = 32 list call and the dense route to the same ranks (predict() per
max_batch rows, remove_non_missing, a full argsort on the host); it fails unless the new call is 10x faster than that route."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import torch
from aaerec.aae import AdversarialAutoEncoder
from aaerec._hip import DeviceCSR
from tools.synth import throughput_corpus
N, h, c, B = int(os.environ.get("RR_ITEMS", 100000)), int(os.environ.get("RR_HIDDEN", 200)), 50, 100
DOCS = int(os.environ.get("RR_DOCS", 8192))
K_RANK = 9
K = int(os.environ.get("RR_K", 10))
X = throughput_corpus(DOCS, N, seed=1234)
m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=B, n_epochs=1, verbose=False, seed=1)
for _ in zip(range(20), m.fit_steps(X)):
    pass
m._fit_finish()
hip = m.hip
csr = DeviceCSR(X, hip.device)
cap = hip.rank_max_rows(K)
print(f"rank_max_rows({K}) = {cap}", flush=True)
ROWS = [int(x) for x in os.environ.get("RR_ROWS", "100,256,512,1024,2048").split(",")]
if os.environ.get("RR_MODE") == "ranks":
    from aaerec.evaluation import remove_non_missing
    T = int(os.environ.get("RR_TRUTH", 1))
    r = np.random.default_rng(0)
    tr = [np.sort(r.choice(N, size=T, replace=False)) for _ in range(DOCS)]
    truth = DeviceCSR.from_arrays(np.arange(DOCS + 1, dtype=np.int64) * T, np.concatenate(tr), np.ones(DOCS * T, dtype=np.float32), N, hip.device)
    print(f"rank_full_max_rows = {hip.rank_full_max_rows()}, {T} held-out item(s) per row", flush=True)

    def region(fn, n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    med = lambda t: sorted(t)[len(t) // 2]                                                          # noqa: E731
    reps_ = int(os.environ.get("RR_REPEATS", 5))
    for rows in ROWS:
        def dense_route():
            full = np.concatenate([hip.predict(csr, s, min(B, rows - s)).cpu().numpy() for s in range(0, rows, B)])
            return np.argsort(remove_non_missing(full, X[:rows], copy=False), axis=1)
        hip.predict_ranks(csr, 0, rows, truth).cpu()
        t_full = [region(lambda: hip.predict_ranks(csr, 0, rows, truth).cpu(), 5) for _ in range(reps_)]
        t_32 = [region(lambda: hip.predict_topk(csr, 0, min(rows, cap), 32)[0].cpu(), 5) for _ in range(reps_)] if rows <= cap else [float("nan")]
        dense_route()
        t_host = [region(dense_route, 1) for _ in range(reps_)]
        print(f"rows/call {rows:5d}: predict_ranks median {med(t_full):.3f} ms (repeats {[round(x, 3) for x in sorted(t_full)]}) | predict_topk k=32: "
              f"{med(t_32):.3f} ms -> {med(t_full) / med(t_32):.2f}x | dense route (predict + host argsort): {med(t_host):.1f} ms "
              f"({[round(x, 1) for x in sorted(t_host)]}) -> {med(t_host) / med(t_full):.1f}x slower", flush=True)
        assert med(t_host) >= 10.0 * med(t_full), "predict_ranks is not 10x faster than the dense route"
    sys.exit(0)
for rows in [r for r in ROWS if r <= cap]:
    reps = max(3, 4096 // rows)
    for timed in (False, True):
        torch.cuda.synchronize()
        if timed:
            hip.profile_enable(True, kernels=(K_RANK,))
        t0 = time.perf_counter()
        for i in range(reps):
            hip.predict_topk(csr, (i * rows) % (DOCS - rows + 1), rows, K)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
    hip.profile_enable(False)
    ms, n = hip.profile_read(K_RANK)
    line = f"rows/call {rows:5d}: {dt * 1e3:8.3f} ms/call  {rows / dt:10.0f} docs/s  ({dt / rows * 1e5 * 1e3:6.1f} us per 100 docs)"
    if n:
        us = ms / n * 1e3
        fl, by = 2.0 * rows * N * (h + 1), 4.0 * N * (h + 1)
        line += f" | rank kernel {us:7.1f} us = {fl / us * 1e-6:6.1f} TFLOP/s ({fl / us * 1e-6 / 157.3:.2f} of fp32 MFMA, {fl / us * 1e-6 / 416.7:.2f} of the emulated product), {by / us * 1e-3:6.0f} GB/s"
    print(line, flush=True)
    if K > 32:
        from aaerec.evaluation import remove_non_missing, argtopk

        def host_route():
            full = np.concatenate([hip.predict(csr, s, min(B, rows - s)).cpu().numpy() for s in range(0, rows, B)])
            y = remove_non_missing(full, X[:rows], copy=False)
            return argtopk(y, K)

        def region(fn, n):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3
        reps_ = int(os.environ.get("RR_REPEATS", 5))
        hip.rank_long_stats()
        t_long = sorted(region(lambda: hip.predict_topk(csr, 0, rows, K)[0].cpu(), 5) for _ in range(reps_))
        st = hip.rank_long_stats()
        t_32 = sorted(region(lambda: hip.predict_topk(csr, 0, rows, 32)[0].cpu(), 5) for _ in range(reps_))
        host_route()
        t_host = sorted(region(host_route, 1) for _ in range(reps_))
        med = lambda t: t[len(t) // 2]                                                              # noqa: E731
        print(f"    k={K} x {rows} rows, ids on the host: median {med(t_long):.3f} ms (repeats {[round(x, 3) for x in t_long]}) | k=32: {med(t_32):.3f} ms "
              f"({[round(x, 3) for x in t_32]}) -> {med(t_long) / med(t_32):.2f}x | predict + host argtopk: {med(t_host):.1f} ms ({[round(x, 1) for x in t_host]}) "
              f"-> {med(t_host) / med(t_long):.1f}x slower | collected per row: mean {st['entries'] / max(1, st['rows']):.1f} max {st['max_entries']} overflow rows {st['overflow_rows']}", flush=True)
for name, fn in (((f"predict_topk through the model (k={K})", lambda: m.predict_topk(X, k=K)),) if "RR_ROWS" not in os.environ else ()):
    out = fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"{name:46s} {DOCS / dt:9.0f} docs/s", flush=True)
