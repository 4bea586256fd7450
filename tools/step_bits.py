"""Same bits across two builds of the library: every way into the training step, a few steps each, one hash per case.

Two builds that claim the same bits (AAE_HIP_LIB names the library, as everywhere) must print the same lines.  Run it twice on
the first build as well: a case whose two runs on ONE build differ is unstable by itself (the single-launch output layer sums its
loss partials in bucket order) and says nothing about the second build.

A line per case:
    case <name> all=<hash> params=<hash> adam=<hash> losses=<hash> predict=<hash> arrays=<n>
all is over everything: every array of state_dict(), the four Adam states (both moments of every layer and the step counts),
the loss series and a predict of the first batch; the other four hashes say which part moved.  arrays counts what was hashed.

Widths every kernel family is compiled for (hidden 200, code 50), 2 000 items, rows 24 (one row block) / 130 (two row blocks, the
bucket build on the side stream; blocked_output) / 512 (the four-wave gather); data from tools/synth.py, fixed seeds, device rng.
At rows 24 and 130 the AAE step also runs on each of the other layer-chain kernels (X16_ROWS, CHAIN16, CHAIN_KSLICES) and with the
categorical and bernoulli priors (softmax and sigmoid encoder outputs); at rows 24 with GELU, on the chain and the per-layer path.

    python tools/step_bits.py [--list] [--only SUBSTRING] [--mark]
--mark launches a cumsum kernel of torch's between the cases, so that a kernel trace of the run can be cut by case.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import torch

from aaerec import _hip
from aaerec._hip import AaeHipError, DeviceCSR, HipAAE
from tools.synth import init_params, throughput_corpus

N, H, CODE, STEPS, NBATCH = 2000, 200, 50, 4, 8
ROWS = (24, 130, 512)


class Ctx:
    """What a case gets: the row count, the corpus on the device (NBATCH batches of `rows`), seeded host randomness."""

    def __init__(self, rows):
        self.B = rows
        self.X = throughput_corpus(NBATCH * rows, N, median_len=20, seed=7)
        self.csr = None
        self.rng = np.random.RandomState(11)

    def start(self, s):
        return (s % NBATCH) * self.B

    def model(self, options=(), params=None, **kw):
        """options: names (set to "1") or (name, value) pairs, in force while the handle is created"""
        options = [(o, "1") if isinstance(o, str) else o for o in options]
        for o, v in options:
            _hip.set_option(o, v)
        try:
            kw.setdefault("blocked_output", self.B > 112)
            m = HipAAE(N, H, CODE, max_batch=self.B, rng_mode="device", seed=1, **kw)
        finally:
            for o, _ in options:
                _hip.set_option(o, None)
        m.load_params(params if params is not None else init_params(N, H, CODE, cond_inc=kw.get("cond_inc", 0), seed=3))
        if self.csr is None:
            self.csr = DeviceCSR(self.X, m.device)
        return m


class Digest:
    def __init__(self):
        self.h = {k: hashlib.sha256() for k in ("all", "params", "adam", "losses", "predict")}
        self.arrays = 0

    def add(self, part, a):
        b = np.ascontiguousarray(a).tobytes()
        self.h[part].update(b)
        self.h["all"].update(b)
        self.arrays += 1

    def state(self, m):
        sd = m.state_dict()
        for k in sorted(sd):
            self.add("params", sd[k])
        for which in ("enc", "dec", "gen", "disc"):
            st = m.adam_state(which)
            for k in sorted(st):
                if k == "step":
                    self.add("adam", np.int64(st[k]))
                else:
                    self.add("adam", st[k][0])
                    self.add("adam", st[k][1])

    def line(self, name):
        return f"case {name} " + " ".join(f"{k}={v.hexdigest()[:16]}" for k, v in self.h.items()) + f" arrays={self.arrays}"


def finish(d, m, predict):
    """the handle's state and a predict of the first batch (a handle that cannot predict: the refusal's text)"""
    torch.cuda.synchronize()
    d.state(m)
    try:
        d.add("predict", predict().float().cpu().numpy())
    except AaeHipError as e:
        d.add("predict", np.frombuffer(str(e).encode(), dtype=np.uint8))


# ---- the cases: each takes (ctx, digest) ------------------------------------------------------------------------------
def plain_step(options=(), cond_inc=0, **kw):
    def run(cx, d):
        m = cx.model(options, cond_inc=cond_inc, **kw)
        cond = torch.as_tensor(cx.rng.rand(NBATCH * cx.B, cond_inc).astype(np.float32), device=m.device) if cond_inc else None
        for s in range(STEPS):
            r0 = cx.start(s)
            m.step(cx.csr, r0, cx.B, cond=None if cond is None else cond[r0:r0 + cx.B])
            d.add("losses", m.losses())
        if kw.get("grad_mode") == "export":
            for which in (_hip.O_DEC, _hip.O_DISC, _hip.O_GEN):
                m.apply_updates(which)
        finish(d, m, lambda: m.predict(cx.csr, 0, cx.B, cond=None if cond is None else cond[:cx.B]))
    return run


def hinted_step(options=()):
    """The next batch named ahead on steps 0 and 1 (the lists built ahead are taken over, the advance rides in the gather),
    not on step 2 (step 3 opens without), a wrong one on step 3 - and a fifth step to meet that hint."""
    def run(cx, d):
        m = cx.model(options)
        for s in range(STEPS + 1):
            if s in (0, 1):
                m.prefetch(cx.csr, cx.start(s + 1), cx.B)
            if s == 3:
                m.prefetch(cx.csr, cx.start(s + 3), cx.B)
            m.step(cx.csr, cx.start(s), cx.B)
            d.add("losses", m.losses())
        finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))
    return run


def split_phases(cx, d):
    m = cx.model()
    for s in range(STEPS):
        z = m.ae_encode(cx.csr, cx.start(s), cx.B)
        dzc = m.ae_decode_backward(z)
        m.ae_encoder_backward(dzc[:, :CODE])
        m.disc_gen()
        d.add("losses", m.losses())
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


def output_layer_cut(cx, d):
    m = cx.model()
    for s in range(STEPS):
        m.ae_forward(cx.csr, cx.start(s), cx.B)
        m.output_layer_step()
        m.ae_backward()
        m.disc_gen()
        d.add("losses", m.losses())
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


def output_layer_alone(cx, d):
    m = cx.model()
    dh2 = m.dh2_rows(cx.B)
    dh2.zero_()
    dh2[:, :H] = torch.as_tensor(cx.rng.rand(cx.B, H).astype(np.float32), device=m.device)
    dh2[:, H] = 1.0
    for s in range(STEPS):
        m.output_layer_step(cx.csr, cx.start(s), cx.B)
        d.add("losses", m.losses())
        d.add("predict", m.da2_rows(cx.B).cpu().numpy())
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


_RCCL = []


def rccl_world1(lib):
    """the collectives table of a one-rank communicator the library creates (aae_rccl_init), shared by the cases"""
    if not _RCCL:
        ident, tab = C.create_string_buffer(128), _hip.AaeCollectives()
        _hip._check(lib.aae_rccl_unique_id(ident))
        _hip._check(lib.aae_rccl_init(ident, 1, 0, C.byref(tab)))
        _RCCL.append(tab)
    return _RCCL[0]


def shard_step(cx, d):
    m = cx.model()
    m.set_first_layer_external(True)
    coll = rccl_world1(m.lib)
    for s in range(STEPS):
        nxt = (cx.start(s + 1), None, cx.B) if s < STEPS - 1 else None
        m.shard_step(coll, cx.csr, cx.start(s), cx.B, 1.0, next_rows=nxt)
        d.add("losses", m.losses())
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


def dp_step(cx, d):
    m = cx.model(grad_mode="export", dp_world=1)
    sl = cx.model()
    m.set_first_layer_external(True)
    sl.set_grad_scale(1.0)
    coll = rccl_world1(m.lib)
    m.dp_reserve(cx.B, 1)
    for s in range(STEPS):
        nxt = (cx.start(s + 1), None) if s < STEPS - 1 else None
        m.dp_step(sl, coll, cx.csr, cx.start(s), cx.B, cx.csr, cx.start(s), cx.B, next_global=nxt)
        d.add("losses", m.losses())
        d.add("losses", sl.losses())
    torch.cuda.synchronize()
    d.state(sl)
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


def decoder_step(cx, d):
    m = cx.model()
    zin = torch.as_tensor(cx.rng.randn(NBATCH * cx.B, CODE).astype(np.float32), device=m.device)
    for s in range(STEPS):
        r0 = cx.start(s)
        dz = m.decoder_step(cx.csr, r0, cx.B, zin[r0:r0 + cx.B])
        d.add("losses", m.losses())
        d.add("predict", dz.cpu().numpy())
    finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))


def vae_model(cx):
    p = init_params(N, H, CODE, seed=3)
    wide = init_params(N, H, 2 * CODE, seed=4)
    p["enc.lin3.weight"], p["enc.lin3.bias"] = wide["enc.lin3.weight"], wide["enc.lin3.bias"]       # [fc21; fc22]
    return cx.model(params=p, vae=True, dropout=(0.0, 0.0))


def vae_step(cx, d):
    m = vae_model(cx)
    for s in range(STEPS):
        m.vae_step(cx.csr, cx.start(s), cx.B)
        d.add("losses", m.losses())
    finish(d, m, lambda: m.vae_predict(cx.csr, 0, cx.B))


def vae_trio(cx, d):
    m = vae_model(cx)
    for s in range(STEPS):
        z = m.vae_encode(cx.csr, cx.start(s), cx.B, train=True)
        dzc = m.vae_decode_backward(z)
        m.vae_encoder_backward(dzc[:, :CODE])
        d.add("losses", m.losses())
    finish(d, m, lambda: m.vae_predict(cx.csr, 0, cx.B))


def vae_eval_calls(cx, d):
    """vae_predict and vae_encode(train=False) between the steps: neither opens a step"""
    m = vae_model(cx)
    for s in range(STEPS):
        m.vae_step(cx.csr, cx.start(s), cx.B)
        d.add("losses", m.losses())
        d.add("predict", m.vae_predict(cx.csr, cx.start(s + 1), cx.B).float().cpu().numpy())
        d.add("predict", m.vae_encode(cx.csr, cx.start(s + 2), cx.B, train=False).cpu().numpy())
    finish(d, m, lambda: m.vae_predict(cx.csr, 0, cx.B))


def dense_noise(gen):
    def run(cx, d):
        m = cx.model(ae_only=True, dense_noise=True)
        for s in range(STEPS):
            if gen:
                m.set_input_noise_gen(0.1)
            else:
                m.set_input_noise(torch.as_tensor(0.1 * cx.rng.randn(cx.B, N).astype(np.float32), device=m.device))
            m.step(cx.csr, cx.start(s), cx.B)
            d.add("losses", m.losses())
        finish(d, m, lambda: m.predict(cx.csr, 0, cx.B))
    return run


def cases(rows):
    out = []
    paths = [("default", ()), ("split_any", ("SPLIT_ANY",)), ("split_any_no_late_join", ("SPLIT_ANY", "NO_LATE_JOIN"))]
    if rows == 24:
        paths.append(("no_chain", ("NO_CHAIN",)))
    for kind, kw in (("aae", {}), ("ae", {"ae_only": True})):
        for tag, options in paths:
            out.append((f"step_{kind}_{tag}", plain_step(options, **kw)))
    # the other layer-chain kernels (default: the 4-row one below 128 rows), the priors other than gauss - with them the softmax
    # and sigmoid encoder outputs - and one activation class that only the 16-row fp32 kernel and the per-layer path carry
    x16, chain16, no_chain = ("x16", (("X16_ROWS", "16"),)), ("chain16", (("CHAIN16", "1"),)), ("no_chain", ("NO_CHAIN",))
    if rows in (24, 130):
        for tag, options in (x16, chain16, ("kslices", (("CHAIN_KSLICES", "1"),))):
            out.append((f"step_aae_{tag}", plain_step(options)))
        for prior in ("categorical", "bernoulli"):
            for tag, options in [("default", ()), x16, chain16] + [no_chain] * (rows == 24):
                out.append((f"step_aae_{prior}_{tag}", plain_step(options, prior=prior)))
    if rows == 24:
        for tag, options in (("default", ()), no_chain):
            out.append((f"step_aae_gelu_{tag}", plain_step(options, activation="GELU")))
    out += [("step_cond20", plain_step(cond_inc=20)),
            ("step_hints", hinted_step()), ("step_hints_early_any", hinted_step(("EARLY_ANY",))),
            ("step_bf16", plain_step(dtype="bf16")),
            ("step_export_apply_updates", plain_step(grad_mode="export")),
            ("split_phases", split_phases), ("output_layer_cut", output_layer_cut), ("output_layer_alone", output_layer_alone),
            ("shard_step_world1", shard_step), ("dp_step_world1", dp_step), ("decoder_step", decoder_step),
            ("vae_step", vae_step), ("vae_trio", vae_trio), ("vae_eval_calls", vae_eval_calls),
            ("dense_noise_given", dense_noise(False)), ("dense_noise_drawn", dense_noise(True))]
    return [(f"b{rows}.{name}", fn) for name, fn in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--mark", action="store_true")
    a = ap.parse_args()
    failed = 0
    print("library", _hip.LIB_PATH, flush=True)
    for rows in ROWS:
        todo = [(n, fn) for n, fn in cases(rows) if a.only in n]
        if a.list:
            print("\n".join(n for n, _ in todo))
            continue
        if not todo:
            continue
        cx = Ctx(rows)
        for name, fn in todo:
            if a.mark:
                torch.cuda.synchronize()
                torch.ones(3, device="cuda").cumsum(0)
                torch.cuda.synchronize()
            d = Digest()
            try:
                fn(cx, d)
                print(d.line(name), flush=True)
            except AaeHipError as e:
                failed += 1
                print(f"case {name} REFUSED {e}", flush=True)
    if _RCCL:
        _hip._check(_hip.load_library().aae_rccl_destroy(C.byref(_RCCL[0])))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
