"""The generator and the step loop of the randomised differential tests, shared by tests/test_fuzz_gpu.py (fp32 mode),
tests/test_fuzz_paths_cpu.py / tests/test_fuzz_paths_gpu.py (fp32 mode on the forced paths, tests/fuzz_path_cases.py) and
tests/test_bf16_fuzz_cpu.py / tests/test_bf16_fuzz_gpu.py (bf16 mode, tests/bf16_cases.py): random model shapes and options,
the batches of a three-step run with a shorter last batch, and the comparison of the device with the oracle.  One
implementation: a configuration and its inputs are the same draws of the same generator whoever asks.  Importing this module
needs NumPy alone; the device and the oracle are imported where they are used."""
import numpy as np

ACTS = ["ReLU", "SELU", "Tanh", "Sigmoid", "ELU", "LeakyReLU"]
# r6: the fourteen further activation classes (csrc/device_common.h; the general program kernel chain_kernel<.., true> and the
# per-layer epilogues carry them)
ACTS_R6 = ["Softplus", "Hardtanh", "ReLU6", "CELU", "Softsign", "Hardsigmoid", "LogSigmoid", "Softshrink", "Hardshrink", "Identity",
           "GELU", "SiLU", "Mish", "Hardswish"]

# A decoder input [z | condition | 1] wider than a row of the layer-chain kernel's LDS slots (208 columns): dec.lin1 runs as
# two k-parts, its dX as two column parts (csrc/abi_chains.h: add_dec_in_fwd / add_dec_in_dx).  C4's shape (code 50 +
# 300-d condition), the narrowest wide input (209 columns: the second part is the bias column alone), the widest (416),
# a part boundary inside the condition / right behind z, a batch beyond one fused launch.
WIDE = [dict(N=300, h=40, c=50, B=37, inc=300), dict(N=120, h=200, c=10, B=100, inc=198), dict(N=500, h=64, c=100, B=64, inc=315),
        dict(N=257, h=207, c=207, B=5, inc=33), dict(N=900, h=100, c=50, B=150, inc=300), dict(N=64, h=7, c=2, B=3, inc=206),
        dict(N=200, h=30, c=300, B=9, inc=0), dict(N=150, h=20, c=210, B=6, inc=100)]      # (a code wider than a slot: layer by layer)

# The library's execution paths a handle can be forced onto (aae_set_option, read once at aae_create): option name and value
PATHS = {"default": None, "kslices": ("CHAIN_KSLICES", 1), "chain16": ("CHAIN16", 1), "no_chain": ("NO_CHAIN", 1),
         "x16": ("X16_ROWS", 16), "split_any": ("SPLIT_ANY", 1), "blocked_any": ("BLOCKED_ANY", 1)}

# The profile's kernel ids of the output layer's forms (aaerec._hip K_DEC_BCE_FWD, K_DEC_FUSED, K_DEC_CRIT, K_DEC_OPT): the
# three-kernel path's first GEMM, the single launch, the split form's critical and deferred launches
OUT_KERNELS = (1, 5, 7, 8)
FUSED_ROWS, LAUNCH_ROWS, ROW_BLOCK = 109, 112, 104


def output_form(path, rows):
    """The form an fp32 handle of the fuzz's sizes (hidden width below 208, fewer than 16384 items, whole-step gradients) takes
    for a batch of `rows` rows, restating csrc/abi_chains.h output_form (the library's one decision; its Split and Blocked are
    'split' here): 'split' (critical + deferred launch; row-blocked beyond 112 rows), 'single' or 'three' (the three
    GEMMs).  The single-launch LDS image of dh2 fits up to 109 rows; a batch of 110 .. 112 rows is one row block that does not
    fit; beyond 112 rows only a blocked_output handle - the fuzz creates one on BLOCKED_ANY - stays on the fused kernels, as
    row blocks of ceil(rows / ceil(rows / 104)) rows."""
    if rows <= FUSED_ROWS:
        return "split" if path == "split_any" else "single"
    if rows <= LAUNCH_ROWS or path != "blocked_any":
        return "three"
    nblk = -(-rows // ROW_BLOCK)
    return "split" if -(-rows // nblk) <= FUSED_ROWS and nblk <= 16 else "three"


def assert_output_form(path, counters, tag):
    """counters: per step (rows, launches of OUT_KERNELS) as check_configuration / check_decoder record them.  On SPLIT_ANY and
    BLOCKED_ANY every step must have taken output_form()'s form and no other: a forced path that fell back silently fails here."""
    ran = {"split": (0, 0, 1, 1), "single": (0, 1, 0, 0), "three": (1, 0, 0, 0)}
    for step, (rows, counts) in enumerate(counters):
        want = ran[output_form(path, rows)]
        assert tuple(min(n, 1) for n in counts) == want, (f"{tag} {path} step {step}, {rows} rows: launches of (bce_fwd, single, critical, "
                                                         f"deferred) {counts}, expected the {output_form(path, rows)} form {want}")


def _forced_handle(path, make):
    """make(blocked_output) with `path`'s option set around the creation (a handle reads its switches once, at creation)"""
    from aaerec import _hip
    opt = PATHS[path]
    if opt:
        _hip.set_option(opt[0], opt[1])
    try:        # (BLOCKED_ANY lifts the size cap of the row-blocked output layer; the form itself is the handle's blocked_output)
        return make(path == "blocked_any")
    finally:
        if opt:
            _hip.set_option(opt[0], None)


def _count_output_launches(dev, counters, rows):
    counters.append((rows, tuple(dev.profile_read(k)[1] for k in OUT_KERNELS)))


def config(seed, tiny=False):
    r = np.random.default_rng((3000 if tiny else 1000) + seed)
    dims = dict(N=int(r.integers(2, 40)), h=int(r.integers(1, 9)), c=int(r.integers(1, 7)), B=int(r.integers(1, 6)),
                inc=int(r.choice([0, 0, 1, 3]))) if tiny else \
        dict(N=int(r.integers(17, 2500)), h=int(r.integers(3, 208)), c=int(r.integers(2, 100)),
             B=int(r.integers(1, 105)), inc=int(r.choice([0, 0, 5, 30, 64])))
    cfg = dict(**dims, act=str(r.choice(ACTS)),
               prior=str(r.choice(["gauss", "gauss", "categorical", "bernoulli"])),
               opt=str(r.choice(["adam", "adam", "sgd"])), drop=bool(r.integers(0, 2)), norm=bool(r.integers(0, 4)),
               scale=float(r.choice([0.0, 0.0, 2.0])), cut=bool(r.integers(0, 2)))
    cfg["inc"] = max(0, min(cfg["inc"], 206 - cfg["c"]))
    if not tiny and r.random() < 0.2:         # batches past the fused output-layer kernel's 104 rows: the three-kernel path
        cfg["B"] = int(r.integers(105, 260))
        cfg["N"] = min(cfg["N"], 1200)
    cfg["long_rows"] = bool(r.random() < 0.15)       # documents with hundreds of items (per-row chunking, >1024 entries per tile)
    cfg["window"] = bool(r.random() < 0.3)           # the batch is a permutation window into a larger resident corpus
    if not tiny and r.random() < 0.2:         # a condition that makes the decoder's input wider than a chain slot (two k-parts)
        cfg["inc"] = int(r.integers(208 - cfg["c"], 415 - cfg["c"]))
    return cfg, r


def wide_config(case, cut, seed=None):
    """WIDE[case] with the options cycling over the cases; the generator its batches are drawn from (seed: 7000 + case)."""
    r = np.random.default_rng(7000 + case if seed is None else seed)
    cfg = dict(**WIDE[case], act=ACTS[case % len(ACTS)], prior=["gauss", "categorical", "gauss"][case % 3],
               opt=["adam", "adam", "sgd"][case % 3], drop=bool(case % 2 == 0), norm=bool(case % 3), scale=0.0, cut=cut,
               long_rows=False, window=bool(case % 2), predict=True)
    return cfg, r


def close_enough(got, want, tol, dmax, tag):
    """Element-wise |got - want| <= tol, except for what a single activation kink / an Adam-eps gradient can move (see
    the note in check_configuration): one hidden unit taking the other branch of its activation
    for one document changes that unit's whole weight-gradient ROW, so up to two rows' worth of elements (at least 8,
    at most 1 % of a large tensor) may exceed tol - none by more than dmax."""
    d = np.abs(got - want)
    allowed = max(8, 0.01 * d.size, 2 * (d.shape[-1] if d.ndim > 1 else 1))
    assert (d > tol).sum() <= allowed and d.max() <= dmax, f"{tag}: {(d > tol).sum()} of {d.size} off (allowed {allowed:.0f}), max {d.max():.2e}"


def model_kwargs(cfg):
    """(constructor arguments HipAAE and OracleAAE share, the dropout rates, the two learning rates)"""
    p = (0.2, 0.3) if cfg["drop"] else (0.0, 0.0)
    lr = (0.05, 0.02) if cfg["opt"] == "sgd" else (2e-3, 1e-3)
    kw = dict(gen_lr=lr[0], reg_lr=lr[1], dropout=p, activation=cfg["act"], prior=cfg["prior"], optimizer=cfg["opt"],
              normalize_inputs=cfg["norm"], prior_scale=cfg["scale"] or None)
    return kw, p, lr


def steps(cfg, r):
    """The three batches of a configuration, the last one shorter: per step a dict with the resident corpus (`corpus`: indptr,
    indices, values - the batch itself unless the configuration draws a window), the permutation window into it (`pick`, or
    None), the batch as the oracle takes it (`ip`, `idx`, `val`), the dropout keep-masks, the prior's draw and the condition
    block.  Every draw comes from r, in one fixed order."""
    N, h, c, B, inc = cfg["N"], cfg["h"], cfg["c"], cfg["B"], cfg["inc"]
    p = (0.2, 0.3) if cfg["drop"] else (0.0, 0.0)
    for s in range(3):
        Bs = B if s < 2 else max(1, B - int(r.integers(0, min(B, 17))))          # a shorter last batch
        max_len = int(min(N, 600)) if cfg["long_rows"] else int(min(N + 1, 12))
        n_docs = 3 * Bs if cfg["window"] else Bs
        rows = [np.sort(r.choice(N, size=int(r.integers(0 if B > 2 else 1, max_len)), replace=False)) for _ in range(n_docs)]
        if not any(len(x) for x in rows):
            rows[0] = np.array([int(r.integers(0, N))])
        ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
        idx = np.concatenate(rows).astype(np.int32)
        val = np.ones(len(idx), dtype=np.float32)
        corpus = (ip, idx, val)
        pick = None
        if cfg["window"]:                      # rows = a window of a permutation, as fit() passes it
            pick = r.permutation(n_docs)[:Bs].astype(np.int32)
            rows = [rows[j] for j in pick]
            ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
            idx = np.concatenate(rows).astype(np.int32) if ip[-1] else np.zeros(0, dtype=np.int32)
            val = np.ones(len(idx), dtype=np.float32)
        masks = None
        if cfg["drop"]:
            masks = [(r.random((Bs, h)) > (p[j % 2])).astype(np.uint8) for j in range(12)]
        if cfg["prior"] == "gauss":
            zr = r.standard_normal((Bs, c)).astype(np.float32)
        elif cfg["prior"] == "categorical":
            zr = np.eye(c, dtype=np.float32)[r.integers(0, c, size=Bs)]
        else:
            zr = np.zeros((Bs, c), dtype=np.float32)             # the reference's randint(0, 1) bernoulli prior
        cond = (r.standard_normal((Bs, inc)) * 0.4).astype(np.float32) if inc else None
        yield dict(s=s, Bs=Bs, corpus=corpus, pick=pick, ip=ip, idx=idx, val=val, masks=masks, zr=zr, cond=cond)


def cut_fits(cfg):
    """(the cut form is the layer-chain models')"""
    return cfg["h"] + 1 <= 208 and cfg["c"] + 1 <= 208 and cfg["c"] + cfg["inc"] + 1 <= 416


def cut_refused(cfg, path):
    """aae_ae_forward on a handle whose hidden layers run layer by layer: AAE_ESTATE.  That is NO_CHAIN, and a
    decoder input wider than a slot on anything but the 4-row chain kernel - which carries neither the r6 classes nor CHAIN16."""
    wide = cfg["c"] + cfg["inc"] + 1 > 208
    return path == "no_chain" or (wide and (cfg["act"] in ACTS_R6 or path == "chain16"))


def bf16_param_stats(got, want, lr, n_steps):
    """Per tensor of a bf16 run against the rounded oracle, as tests/test_bf16_gpu.py counts them: the share of elements beyond
    1e-4 max(1, lr / 1e-3), the share allowed (1 % of a tensor; at least 8 elements or two rows' worth, as close_enough), the
    largest difference and its bound 3 lr steps n_opt (the encoder takes two optimiser steps per partial_fit)."""
    stats = {}
    for k, w in want.items():
        d = np.abs(got[k].astype(np.float64) - w)
        allowed = max(8, 0.01 * d.size, 2 * (d.shape[-1] if d.ndim > 1 else 1)) / d.size
        n_opt = 2 if k.startswith("enc.") else 1
        stats[k] = (float((d > 1e-4 * max(1.0, lr / 1e-3)).mean()), allowed, float(d.max()), 3.0 * lr * n_steps * n_opt)
    return stats


SGD_TOL = 5e-5        # (the fp32 fuzz's; tests/bf16_cases.py has the measurement that keeps it for bf16 mode)


def check_configuration(cfg, r, seed, bf16=False, path="default", counters=None, max_batch=None):
    """Three steps of the device against the oracle, the parameters after them, and predict where the configuration asks, on
    a handle forced onto `path`.  bf16: a dtype = 'bf16' handle against OracleAAE(bf16=True) at the tolerances of
    tests/test_bf16_gpu.py; returns the observed (share, maximum) per tensor.  counters: a list that receives, per step,
    (rows, launches of OUT_KERNELS) from the handle's profile.  max_batch: the handle's, where it is to be larger than the
    configuration's batch."""
    import pytest
    import torch
    from aaerec import _hip
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    N, h, c, B, inc = cfg["N"], cfg["h"], cfg["c"], cfg["B"], cfg["inc"]
    params = init_params(N, h, c, cond_inc=inc, seed=seed)
    kw, p, lr = model_kwargs(cfg)
    R = max_batch or B
    if bf16:
        dev = _forced_handle(path, lambda blocked: HipAAE(N, h, c, cond_inc=inc, max_batch=R, rng_mode="inject", dtype="bf16", blocked_output=blocked, **kw))
    elif path != "default":
        dev = _forced_handle(path, lambda blocked: HipAAE(N, h, c, cond_inc=inc, max_batch=R, rng_mode="inject", blocked_output=blocked, **kw))
    else:
        dev = HipAAE(N, h, c, cond_inc=inc, max_batch=R, rng_mode="inject", **kw)
    dev.load_params(params)
    if counters is not None:
        dev.profile_enable(True, kernels=OUT_KERNELS)
    tag = f"{cfg}" if path == "default" else f"{cfg} {path}"
    ora = O.OracleAAE(params, conditions=[O.ConcatConst(inc)] if inc else [], bf16=bf16, **kw)
    for st in steps(cfg, r):
        s, Bs, ip, idx, val, masks, zr, cond = (st[k] for k in ("s", "Bs", "ip", "idx", "val", "masks", "zr", "cond"))
        csr = DeviceCSR.from_arrays(*st["corpus"], N, dev.device)
        sel = torch.as_tensor(st["pick"], device=dev.device) if st["pick"] is not None else None
        cdev = torch.as_tensor(cond, device=dev.device) if inc else None
        cut = cfg["cut"] and cut_fits(cfg)
        if cut and cut_refused(cfg, path):
            # the library refuses the cut form here: the status and the message, and then the whole step on the same handle
            with pytest.raises(_hip.AaeHipError, match=r"error -4: aae_ae_forward needs the layer-chain kernels"):
                dev.ae_forward(csr, 0, Bs, rows=sel, cond=cdev, masks=masks, z_real=zr)
            cut = False
        if cut:
            dev.ae_forward(csr, 0, Bs, rows=sel, cond=cdev, masks=masks, z_real=zr)
            dev.output_layer_step()
            dev.ae_backward()
            dev.disc_gen()
        else:
            dev.step(csr, 0, Bs, rows=sel, cond=cdev, masks=masks, z_real=zr)
        want = ora.partial_fit(ip, idx, val, zr, masks, [cond] if inc else None)
        if bf16:
            np.testing.assert_allclose(dev.losses(), want, rtol=2e-4, atol=2e-6, err_msg=f"{cfg} {path} step {s}")
        else:
            np.testing.assert_allclose(dev.losses(), want, rtol=5e-5, atol=2e-6, err_msg=f"{tag} step {s}")
        if counters is not None:
            _count_output_launches(dev, counters, Bs)
    got = dev.state_dict()
    stats = None
    if bf16 and cfg["opt"] == "sgd":
        # no Adam, no step whose size ignores the gradient's: the fp32 bound as it stands
        for k, w in ora.p.items():
            close_enough(got[k], w, SGD_TOL, 3 * max(lr), f"{cfg} {path} {k}")
        stats = {k: (float((np.abs(got[k] - w) > SGD_TOL).mean()), None, float(np.abs(got[k] - w).max()), 3 * max(lr)) for k, w in ora.p.items()}
    elif bf16:
        # tests/test_bf16_gpu.py: an fp32 summation-order difference that straddles a bf16 rounding boundary of an operand moves
        # it by 2^-8 relative, and Adam's first steps move a parameter by ~lr whatever the size of its gradient
        stats = bf16_param_stats(got, ora.p, max(lr), 3)
        for k, (frac, allowed, mx, bound) in stats.items():
            assert frac <= allowed and mx <= bound, (cfg, path, k, frac, allowed, mx, bound)
    else:
        # Parameters: 5e-5 absolute.  Two fp32 effects can move single elements further without anything being wrong, and
        # a random search over hundreds of configurations does find them (tools/debug/fuzz_case.py prints both):
        # a pre-activation within ~1e-7 of an activation kink (ReLU / LeakyReLU / SELU at 0) takes the other branch under a
        # different summation order, and Adam turns a gradient of the order of its eps (1e-8) into a step of the order of
        # the learning rate.  So: at most 1 % of a tensor's elements (8 for the small ones) may exceed the tolerance, none by
        # more than 3 lr.
        for k, w in ora.p.items():
            close_enough(got[k], w, 5e-5, 3 * max(lr), f"{tag} {k}")
    if cfg.get("predict"):                     # the last batch's reconstructions with the trained weights (no dropout)
        out = dev.predict(csr, 0, Bs, cond=cdev) if sel is None else None
        if out is not None:
            want = ora.predict(ip, idx, val, [cond] if inc else None)
            np.testing.assert_allclose(out.cpu().numpy(), want, atol=5e-4 if bf16 else 1e-4, err_msg=f"{cfg} predict")
    dev.close()
    return stats


def batch(r, N, Bs, B, max_len=12):
    rows = [np.sort(r.choice(N, size=int(r.integers(0 if B > 2 else 1, min(N, max_len))), replace=False)) for _ in range(Bs)]
    if not any(len(x) for x in rows):
        rows[0] = np.array([int(r.integers(0, N))])
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    return ip, idx, np.ones(len(idx), dtype=np.float32)


def decoder_config(seed):
    """(the draws every case of the sibling models' test opens with)"""
    r = np.random.default_rng(9000 + seed)
    N, h, B = int(r.integers(17, 1500)), int(r.integers(3, 208)), int(r.integers(1, 150))
    act = str(r.choice(["ReLU", "Tanh", "SELU", "ELU"]))
    return r, N, h, B, act


def decoder_steps(r, N, h, B, seed):
    """The decoder-only case's own draws: the input width, dropout on or off, then per step the batch, the input block and the
    two keep-masks; at last the input block of decode().  A generator: the first item is (c, p)."""
    c = int(r.integers(2, 200))
    p = (0.2, 0.2) if r.integers(0, 2) else (0.0, 0.0)
    yield c, p
    for s in range(3):
        ip, idx, val = batch(r, N, B, B)
        zin = (r.standard_normal((B, c)) * 0.5).astype(np.float32)
        masks = [(r.random((B, h)) > 0.2).astype(np.uint8) for _ in range(2)] if p[0] else None
        yield ip, idx, val, zin, masks
    yield (r.standard_normal((B, c)) * 0.5).astype(np.float32)


def check_decoder(r, N, h, B, act, seed, bf16=False, dz_tol=None, decode_tol=None, path="default", counters=None):
    """aae_decoder_step (DecodingRecommender: decoder only, input block from the conditions, dL/d(input) returned) against
    OracleDecoder; bf16: both in bf16 mode, at the tolerances of tests/test_bf16_gpu.py.  path, counters: as check_configuration's
    (fp32 handles)."""
    import torch
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    it = decoder_steps(r, N, h, B, seed)
    c, p = next(it)
    params = init_params(N, h, c, seed=seed)
    mk = dict(max_batch=B, rng_mode="inject", gen_lr=2e-3, reg_lr=2e-3, dropout=p, activation=act, **(dict(dtype="bf16") if bf16 else {}))
    dev = HipAAE(N, h, c, **mk) if path == "default" else _forced_handle(path, lambda blocked: HipAAE(N, h, c, blocked_output=blocked, **mk))
    dev.load_params(params)
    if counters is not None:
        dev.profile_enable(True, kernels=OUT_KERNELS)
    ora = O.OracleDecoder(params, lr=2e-3, dropout=p, activation=act, conditions=[O.ConcatConst(c)], **(dict(bf16=True) if bf16 else {}))
    for s in range(3):
        ip, idx, val, zin, masks = next(it)
        dz = dev.decoder_step(DeviceCSR.from_arrays(ip, idx, val, N, dev.device), 0, B,
                              torch.as_tensor(zin, device=dev.device), masks=masks)
        want = ora.partial_fit([zin], ip, idx, val, masks)
        if bf16:
            np.testing.assert_allclose(dev.losses()[0], want, rtol=2e-4, atol=2e-6)
            if s == 0:      # (dL/d(input) while both sides still hold the same parameters: tests/bf16_cases.py DZ_TOL)
                d = np.abs(dz.cpu().numpy().astype(np.float64) - ora.last_dzin)
                print(f"BF16FUZZ decoder seed {seed} dz worst {d.max() / float(np.abs(ora.last_dzin).max()):.3e} of max |dz| (tolerance {dz_tol:.1e})")
                assert d.max() <= dz_tol * float(np.abs(ora.last_dzin).max()), (d.max(), float(np.abs(ora.last_dzin).max()))
        else:
            np.testing.assert_allclose(dev.losses()[0], want, rtol=5e-5, atol=2e-6)
            np.testing.assert_allclose(dz.cpu().numpy(), ora.last_dzin, rtol=5e-4, atol=1e-7)     # (entries are sums with cancellation, ~1e-4 in size)
        if counters is not None:
            _count_output_launches(dev, counters, B)
    got = dev.state_dict()
    zp = next(it)
    stats = None
    if bf16:
        stats = bf16_param_stats(got, ora.p, 2e-3, 3)
        for k, (frac, allowed, mx, bound) in stats.items():
            assert frac <= allowed and mx <= bound, (f"decoder N={N} h={h} c={c} B={B}", k, frac, allowed, mx, bound)
        out = dev.decode(torch.as_tensor(zp, device=dev.device)).cpu().numpy()
        print(f"BF16FUZZ decoder seed {seed} decode worst {np.abs(out - ora.predict([zp])).max():.3e} (tolerance {decode_tol:.1e})")
        np.testing.assert_allclose(out, ora.predict([zp]), atol=decode_tol)
        dev.close()
    else:
        for k, w in ora.p.items():
            close_enough(got[k], w, 5e-5, 6e-3, f"decoder N={N} h={h} c={c} B={B} {k}")
        np.testing.assert_allclose(dev.decode(torch.as_tensor(zp, device=dev.device)).cpu().numpy(), ora.predict([zp]), atol=2e-5)
    return stats


def vae_draws(r, seed, N, h, B):
    """The VAE case's own draws behind decoder_config's: code and condition widths, torch-initialised fc1 .. fc4, then per step
    the batch, eps and the condition block.  -> (c, inc, the parameters by the reference's names, the three steps)"""
    import torch
    c, inc = int(r.integers(2, 100)), int(r.choice([0, 0, 9, 40]))
    inc = min(inc, 206 - c)
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        k = 1.0 / np.sqrt(i)
        return ((torch.rand(o, i, generator=g) * 2 - 1) * k).numpy(), ((torch.rand(o, generator=g) * 2 - 1) * k).numpy()
    vp = {}
    for name, (o, i) in (("fc1", (h, N)), ("fc21", (c, h)), ("fc22", (c, h)), ("fc3", (h, c + inc)), ("fc4", (N, h))):
        vp[name + ".weight"], vp[name + ".bias"] = lin(o, i)
    steps_ = []
    for s in range(3):
        Bs = B if s < 2 else max(1, B - int(r.integers(0, min(B, 9))))
        ip, idx, val = batch(r, N, Bs, B)
        eps = r.standard_normal((Bs, c)).astype(np.float32)
        cond = (r.standard_normal((Bs, inc)) * 0.4).astype(np.float32) if inc else None
        steps_.append((Bs, ip, idx, val, eps, cond))
    return c, inc, vp, steps_


def check_vae(r, N, h, B, act, seed, path="default"):
    """aae_vae_step (VAE) against OracleVAE over decoder_config's draws, on a handle forced onto `path`."""
    import pytest
    import torch
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    c, inc, vp, steps_ = vae_draws(r, seed, N, h, B)
    dev = _forced_handle(path, lambda blocked: HipAAE(N, h, c, cond_inc=inc, max_batch=B, rng_mode="inject", gen_lr=2e-3, reg_lr=2e-3, dropout=(0.0, 0.0),
                                                      activation=act, vae=True))
    dev.load_params({"enc.lin1.weight": vp["fc1.weight"], "enc.lin1.bias": vp["fc1.bias"],
                     "enc.lin3.weight": np.vstack([vp["fc21.weight"], vp["fc22.weight"]]),
                     "enc.lin3.bias": np.concatenate([vp["fc21.bias"], vp["fc22.bias"]]),
                     "dec.lin1.weight": vp["fc3.weight"], "dec.lin1.bias": vp["fc3.bias"],
                     "dec.lin3.weight": vp["fc4.weight"], "dec.lin3.bias": vp["fc4.bias"]})
    ora = O.OracleVAE(vp, lr=2e-3, activation=act, conditions=[O.ConcatConst(inc)] if inc else [])
    if path == "no_chain":
        # the VAE's hidden half is a layer program and nothing else: layer by layer the library refuses the step - the status and
        # the message, and the parameters as they were loaded
        from aaerec import _hip
        Bs, ip, idx, val, eps, cond = steps_[0]
        with pytest.raises(_hip.AaeHipError, match=r"error -4: VAE mode needs the layer-chain kernels"):
            dev.vae_step(DeviceCSR.from_arrays(ip, idx, val, N, dev.device), 0, Bs,
                         cond=torch.as_tensor(cond, device=dev.device) if inc else None, eps=eps)
        assert np.array_equal(dev.state_dict()["dec.lin3.weight"], vp["fc4.weight"])
        return
    for Bs, ip, idx, val, eps, cond in steps_:
        dev.vae_step(DeviceCSR.from_arrays(ip, idx, val, N, dev.device), 0, Bs,
                     cond=torch.as_tensor(cond, device=dev.device) if inc else None, eps=eps)
        want = ora.partial_fit(ip, idx, val, eps, [cond] if inc else None)
        l = dev.losses()
        np.testing.assert_allclose((l[0] + l[1]) / Bs, want, rtol=5e-5)
    got = dev.state_dict()
    want = {"enc.lin1.weight": ora.p["fc1.weight"], "enc.lin3.weight": np.vstack([ora.p["fc21.weight"], ora.p["fc22.weight"]]),
            "dec.lin1.weight": ora.p["fc3.weight"], "dec.lin3.weight": ora.p["fc4.weight"], "dec.lin3.bias": ora.p["fc4.bias"]}
    for k, w in want.items():
        close_enough(got[k], w, 5e-5, 6e-3, f"vae N={N} h={h} c={c} inc={inc} B={B} {k}")
