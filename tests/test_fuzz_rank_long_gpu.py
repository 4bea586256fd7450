"""Randomised long-list ranking (k in 33..1024; csrc/rank_long.h) in the style of tests/test_fuzz_gpu.py's rank case: random
shapes and execution paths (hidden widths inside and beyond the layer-chain kernels, so both the fused and the dense form),
a few training steps, then the on-device top-k against the oracle's eval-mode predict."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _batch(r, N, B, max_len):
    rows = [np.sort(r.choice(N, size=int(r.integers(1, max_len + 1)), replace=False)) for _ in range(B)]
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), np.ones(int(ip[-1]), dtype=np.float32)


@pytest.mark.parametrize("seed", range(int(os.environ.get("AAE_FUZZ_SEEDS", "12"))))
def test_random_long_lists_match_oracle(seed):
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    r = np.random.default_rng(9000 + seed)
    wide = seed % 4 == 3
    N = int(r.integers(60, 6000))
    h = int(r.integers(208, 260)) if wide else int(r.integers(8, 200))
    c = int(r.integers(2, 40))
    B = int(r.integers(2, 40))
    act = str(r.choice(["ReLU", "Tanh", "ELU", "GELU"]))
    params = init_params(N, h, c, seed=seed)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * 5.0
    kw = dict(gen_lr=2e-3, reg_lr=1e-3, dropout=(0.0, 0.0), activation=act)
    ora = O.OracleAAE(params, **kw)
    dev = HipAAE(N, h, c, max_batch=B, rng_mode="inject", **kw)
    dev.load_params(params)
    for s in range(3):
        ip, idx, val = _batch(r, N, B, 6)
        zr = r.standard_normal((B, c)).astype(np.float32)
        dev.step(DeviceCSR.from_arrays(ip, idx, val, N, dev.device), 0, B, z_real=zr)
        ora.partial_fit(ip, idx, val, zr)
    ip, idx, val = _batch(r, N, B, 6)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
    pred = ora.predict(ip, idx, val)
    k = int(min(r.integers(33, 1025), N - 6))
    excl = bool(r.integers(0, 2))
    ids, vals = dev.predict_topk(csr, 0, B, k, exclude_known=excl)
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    for b in range(B):
        known = set(idx[ip[b]:ip[b + 1]].tolist())
        assert len(set(ids[b].tolist())) == k and (np.diff(vals[b]) <= 1e-6).all(), (seed, b)     # k distinct items, best first
        score = pred[b].copy()
        if excl:
            assert not (set(ids[b].tolist()) & known)
            score[list(known)] = -1.0
        kth = np.sort(score)[-k]
        assert (score[ids[b]] >= kth - 1e-4).all(), f"seed {seed} N={N} h={h} act={act} row {b}: not the top {k} (exclude_known={excl})"
        lo, hi = pred[b].min(), pred[b].max()
        np.testing.assert_allclose(vals[b], (pred[b][ids[b]] - lo) / (hi - lo), atol=5e-4)
