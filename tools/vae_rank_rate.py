#!/usr/bin/env python3
"""The VAE's predict -> rank at the headline shape (C3: 100 000 items, hidden 200, VR_DOCS = 10 000 test rows).
1. VAERecommender through Evaluation, topk=True (predict_topk on the device: aae_vae_predict_topk) against topk=False (the
   reference's dense pipeline: the [n, items] matrix to the host, minmax_scale / argpartition there) - the same build, the
   same trained model, bounded metrics; whole-call wall time, median of VR_REPEATS.
2. The fused call alone (aae_vae_predict_topk, rows per call = what the handle takes, ids on the host) against aae_vae_predict
   per max_batch rows + remove_non_missing + argtopk on the host, and against the AAE's aae_predict_topk at the same shape.
3. The hidden half's chain program on the 4-row kernel (chain4.h, the rank calls) against the same layers on the 16-row kernel
   (chain.h, aae_vae_predict's program, which also stores mu / logvar / eps / zc) at 128 / 1024 / 4096 rows: HIP-event time of
   the chain launch (AAE_K_CHAIN), median of VR_REPEATS launches behind 3 warm-up launches.  The two launches do not do the
   same work: chain.h's program has the four extra stores, and the rank call pays a memset and two interleave4 launches for
   its weight copies OUTSIDE the timed launch - their cost is printed beside the pair (the same call's wall time with and
   without them is not separable from the host; they are timed as the wall time of a decode-form call on ONE row, whose
   chain program is a single 51 -> 200 layer, against the same call's chain launch).
4. (--cond-inc a,b,..: this part alone) aae_vae_step and aae_vae_predict_topk behind a constant condition block of each
   width, at VR_ITEMS items, VR_HIDDEN hidden units, code 50 and --batch rows per step: ms/step as the median of --repeats
   timed runs of --steps steps behind --warmup steps, the rank call's ms per call of --batch rows beside it.  A decoder
   input n_code + cond_inc + 1 beyond 208 columns runs fc3 in k-parts of 208 (csrc/abi_chains.h): 0 and 150 are one slot,
   332 two parts (the reference's main.py), 932 five (mpd.py).
5. (--hidden a,b,.. --code x,y,..: this part alone) aae_vae_step by the width of the hidden layer and of the code, one handle
   per (hidden, code) pair, cfg.vae_wide on: a pair beyond a chain slot (hidden > 207 or 2 code > 208) runs the per-layer route
   (csrc/abi_output_layer.h vae_*_layers), a narrow one the chain programs - unless its entry of --layer-route (0 / 1 per pair)
   forces the per-layer route (option NO_CHAIN), which makes a narrow pair the A/B of the two routes.  All handles are built
   first and take turns inside every repeat; ms/step as in part 4, and aae_vae_predict_topk(k = 10) in rows/s beside it.
VR_PARTS=1,2,3 selects the parts."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import scipy.sparse as sp
import torch
from aaerec import _hip
from aaerec._hip import DeviceCSR, HipAAE, K_CHAIN
from aaerec.evaluation import Evaluation, argtopk, remove_non_missing
from aaerec.vae import VAERecommender
from tools.synth import throughput_corpus

N, h, c, B = int(os.environ.get("VR_ITEMS", 100000)), int(os.environ.get("VR_HIDDEN", 200)), 50, 100
DOCS, REPS = int(os.environ.get("VR_DOCS", 10000)), int(os.environ.get("VR_REPEATS", 3))
_ap = argparse.ArgumentParser()
_ap.add_argument("--cond-inc", default="", help="comma-separated condition widths: time aae_vae_step at each (part 4 alone)")
_ap.add_argument("--hidden", default="", help="comma-separated hidden widths: time aae_vae_step at each (hidden, code) pair (part 5 alone)")
_ap.add_argument("--code", default="", help="comma-separated code widths, one per --hidden entry")
_ap.add_argument("--layer-route", default="", help="comma-separated 0 / 1 per pair: 1 forces the per-layer route at a narrow size")
_ap.add_argument("--batch", type=int, default=1000)
_ap.add_argument("--steps", type=int, default=50)
_ap.add_argument("--warmup", type=int, default=20)
_ap.add_argument("--repeats", type=int, default=7)
ARGS = _ap.parse_args()
PARTS = [5] if ARGS.hidden else [4] if ARGS.cond_inc else [int(x) for x in os.environ.get("VR_PARTS", "1,2,3").split(",")]
med = lambda t: sorted(t)[len(t) // 2]                                                                  # noqa: E731


def region(fn, n=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


class Set:
    """What Evaluation and a recommender read of a Bags."""
    def __init__(self, X):
        self.X = X

    def tocsr(self):
        return self.X

    def size(self, dim=0):
        return self.X.shape[dim]

    def clone(self):
        return self

    def get_attributes(self, keys):
        return []


class Trained(VAERecommender):
    def train(self, training_set):          # (trained once: both Evaluation runs score the same model)
        if self.model is None:
            super().train(training_set)


if 1 in PARTS or 2 in PARTS:
    X = throughput_corpus(DOCS, N, seed=1234)
    r = np.random.default_rng(0)
    held = r.integers(0, N, DOCS)          # (one held-out item per row; one that the row names ranks behind the rankable ones)
    Y = sp.csr_matrix((np.ones(DOCS, dtype=np.float32), (np.arange(DOCS), held)), shape=X.shape)
    rec = Trained(n_hidden=h, n_code=c, n_epochs=1, batch_size=B, lr=0.001, verbose=False, seed=1)
    rec.train(Set(X))
    hip = rec.model.hip

if 1 in PARTS:
    metrics = ["mrr@10", "map@10", "p@5", "P@1"]
    times = {}
    for topk in (True, False):
        ev = Evaluation(None, 0, metrics=metrics, logfile=os.devnull, topk=topk)
        ev.train_set, ev.test_set, ev.x_test, ev.y_test = Set(X), Set(X), X, Y
        if topk:
            ev([rec], batch_size=1000)
        times[topk] = [region(lambda: ev([rec], batch_size=1000)) for _ in range(REPS)]
        print(f"Evaluation(topk={topk}) of VAERecommender, {DOCS} test rows x {N} items: median {med(times[topk]) / 1e3:.3f} s "
              f"(repeats {[round(x / 1e3, 3) for x in sorted(times[topk])]})", flush=True)
    print(f"  -> the dense pipeline takes {med(times[False]) / med(times[True]):.1f}x the device ranking", flush=True)

if 2 in PARTS:
    csr = DeviceCSR(X, hip.device)
    rows = min(hip.vae_rank_max_rows(10), 2048, DOCS)
    print(f"vae_rank_max_rows(10) = {hip.vae_rank_max_rows(10)}, vae_rank_full_max_rows = {hip.vae_rank_full_max_rows()}; {rows} rows per call", flush=True)

    def host_route():
        full = np.concatenate([hip.vae_predict(csr, s, min(B, rows - s)).cpu().numpy() for s in range(0, rows, B)])
        return argtopk(remove_non_missing(full, X[:rows], copy=False), 10)
    hip.vae_predict_topk(csr, 0, rows, 10)[0].cpu()
    t_fused = [region(lambda: hip.vae_predict_topk(csr, 0, rows, 10)[0].cpu(), 5) for _ in range(REPS)]
    host_route()
    t_host = [region(host_route) for _ in range(REPS)]
    print(f"aae_vae_predict_topk, {rows} rows, ids on the host: median {med(t_fused):.3f} ms (repeats {[round(x, 3) for x in sorted(t_fused)]}) | "
          f"aae_vae_predict + host ranking: {med(t_host):.1f} ms ({[round(x, 1) for x in sorted(t_host)]}) -> {med(t_host) / med(t_fused):.1f}x", flush=True)
    aae = HipAAE(N, h, c, max_batch=B, rng_mode="device", seed=1)
    arows = min(rows, aae.rank_max_rows(10))
    acsr = DeviceCSR(X, aae.device)
    aae.predict_topk(acsr, 0, arows, 10)[0].cpu()
    t_aae = [region(lambda: aae.predict_topk(acsr, 0, arows, 10)[0].cpu(), 5) for _ in range(REPS)]
    print(f"aae_predict_topk (AAE handle, same shape), {arows} rows: median {med(t_aae):.3f} ms (repeats {[round(x, 3) for x in sorted(t_aae)]})"
          f" -> the VAE call takes {med(t_fused) / rows / (med(t_aae) / arows):.3f}x per row", flush=True)

if 3 in PARTS:
    Ns, R = 4096, 4096
    dev = HipAAE(Ns, h, c, max_batch=R, max_nnz=R * 64, rng_mode="device", seed=1, dropout=(0.0, 0.0), vae=True)
    Xs = throughput_corpus(R, Ns, seed=5)
    scsr = DeviceCSR(Xs, dev.device)
    reps = max(REPS, 9)
    print("part 3: the chain.h program also stores mu / logvar / eps / zc; the rank call derives its weight copies (a memset + two "
          "interleave4 launches) outside the timed chain launch", flush=True)
    zc1 = torch.zeros(1, c, device=dev.device)
    dev.vae_decode_topk(zc1, scsr, 0, 10)
    t_call = med([region(lambda: dev.vae_decode_topk(zc1, scsr, 0, 10), 20) for _ in range(reps)]) * 1e3
    print(f"   a one-row decode-form call, launch to completion: {t_call:.1f} us wall (derive + chain + mask + rank + merge: the derive's three "
          "launches are at most this)", flush=True)
    for rows in (128, 1024, 4096):
        if rows > dev.vae_rank_max_rows(10):
            print(f"{rows} rows: beyond vae_rank_max_rows(10) = {dev.vae_rank_max_rows(10)} of this handle", flush=True)
            continue
        out = {}
        for name, fn in (("chain4.h (4 rows per workgroup, rank call)", lambda: dev.vae_predict_topk(scsr, 0, rows, 10)),
                         ("chain.h (16 rows per workgroup, aae_vae_predict)", lambda: dev.vae_predict(scsr, 0, rows))):
            for _ in range(3):
                fn()
            t = []
            for _ in range(reps):
                torch.cuda.synchronize()
                dev.profile_enable(True, kernels=(K_CHAIN,))
                fn()
                torch.cuda.synchronize()
                dev.profile_enable(False)
                ms, n = dev.profile_read(K_CHAIN)
                t.append(ms / max(n, 1) * 1e3)
            out[name] = med(t)
            print(f"{rows:5d} rows, hidden-half program on {name}: median {med(t):.1f} us (repeats {[round(x, 1) for x in sorted(t)]})", flush=True)

if 4 in PARTS:
    Bt = ARGS.batch
    Xt = throughput_corpus(Bt * 8, N, seed=77)
    for inc in [int(x) for x in ARGS.cond_inc.split(",")]:
        dev = HipAAE(N, h, c, cond_inc=inc, max_batch=Bt, rng_mode="device", seed=1, dropout=(0.0, 0.0), vae=True)
        tcsr = DeviceCSR(Xt, dev.device)
        cond = torch.randn(Bt, inc, device=dev.device) * 0.4 if inc else None
        it = [0]

        def one_step():
            dev.vae_step(tcsr, (it[0] % 8) * Bt, Bt, cond=cond)
            it[0] += 1
        region(one_step, ARGS.warmup)
        t_step = [region(one_step, ARGS.steps) for _ in range(ARGS.repeats)]
        rows = min(Bt, dev.vae_rank_max_rows(10))
        crow = None if cond is None else cond[:rows]
        region(lambda: dev.vae_predict_topk(tcsr, 0, rows, 10, cond=crow), 3)
        t_rank = [region(lambda: dev.vae_predict_topk(tcsr, 0, rows, 10, cond=crow), 10) for _ in range(ARGS.repeats)]
        print(f"cond_inc {inc:4d} (decoder input {c + inc + 1:4d} columns, {(c + inc + 1 + 207) // 208} part(s)), {N} items, hidden {h}, "
              f"batch {Bt}: aae_vae_step median {med(t_step):.4f} ms/step (min {min(t_step):.4f}, max {max(t_step):.4f}, "
              f"{ARGS.repeats} runs of {ARGS.steps}) | aae_vae_predict_topk(k=10), {rows} rows: median {med(t_rank):.3f} ms "
              f"(min {min(t_rank):.3f}, max {max(t_rank):.3f}); vae_rank_max_rows(10) = {dev.vae_rank_max_rows(10)}", flush=True)
        dev.close()

if 5 in PARTS:
    Bt = ARGS.batch
    hs, cs = [int(x) for x in ARGS.hidden.split(",")], [int(x) for x in ARGS.code.split(",")]
    forced = [int(x) for x in ARGS.layer_route.split(",")] if ARGS.layer_route else [0] * len(hs)
    assert len(hs) == len(cs) == len(forced), "--hidden, --code and --layer-route name one entry per pair"
    Xt = throughput_corpus(Bt * 8, N, seed=77)
    runs = []
    for hh, cc, f in zip(hs, cs, forced):
        if f:
            _hip.set_option("NO_CHAIN", "1")
        try:
            dev = HipAAE(N, hh, cc, max_batch=Bt, rng_mode="device", seed=1, dropout=(0.0, 0.0), vae=True, vae_wide=True)
        finally:
            _hip.set_option("NO_CHAIN", None)
        tcsr = DeviceCSR(Xt, dev.device)
        it = [0]

        def one_step(dev=dev, tcsr=tcsr, it=it):
            dev.vae_step(tcsr, (it[0] % 8) * Bt, Bt)
            it[0] += 1
        rows = min(Bt, dev.vae_rank_max_rows(10))
        rank = lambda dev=dev, tcsr=tcsr, rows=rows: dev.vae_predict_topk(tcsr, 0, rows, 10)      # noqa: E731
        region(one_step, ARGS.warmup)
        region(rank, 3)
        layer = bool(f) or hh > 207 or 2 * cc > 208
        runs.append(dict(h=hh, c=cc, layer=layer, step=one_step, rank=rank, rows=rows, t_step=[], t_rank=[]))
    for _ in range(ARGS.repeats):
        for q in runs:
            q["t_step"].append(region(q["step"], ARGS.steps))
            q["t_rank"].append(region(q["rank"], 10))
    for q in runs:
        print(f"hidden {q['h']:4d} code {q['c']:3d} on the {'per-layer' if q['layer'] else 'chain'} route, {N} items, batch {Bt}: aae_vae_step median "
              f"{med(q['t_step']):.4f} ms/step (min {min(q['t_step']):.4f}, max {max(q['t_step']):.4f}, {ARGS.repeats} runs of {ARGS.steps}) | "
              f"aae_vae_predict_topk(k=10), {q['rows']} rows: median {med(q['t_rank']):.3f} ms = {q['rows'] / med(q['t_rank']) * 1e3:.0f} rows/s "
              f"(min {min(q['t_rank']):.3f}, max {max(q['t_rank']):.3f})", flush=True)
