"""The bf16 fuzz without a GPU: what the case lists of tests/bf16_cases.py hold, and that the reference alone stays inside a
quarter of every cap tests/test_bf16_fuzz_gpu.py holds the device to.

Each case runs through OracleAAE(bf16=True) and through its twin (bf16_cases._Twin: the same rounding points, float64
accumulation of every dense product, hidden activations moved by 4 units in the last place wherever the class evaluates a
library function, the sign by a hash of the argument).  The two differ the way two correct implementations of the mode may:
a pre-rounding value that moves by fp32 units lands on the other side of a bf16 rounding boundary for about 1e-4 of the
elements, that operand moves by 2^-8 relative, and Adam turns what this does to a near-zero gradient into a step of ~lr.

Asserted per case: losses within a quarter of (rtol 2e-4, atol 2e-6); Adam parameters - at most a quarter of the allowed share
(1 % of a tensor, at least 8 elements or two rows' worth) beyond 1e-4 max(1, lr / 1e-3), no element beyond a quarter of
3 lr steps n_opt; SGD parameters - close_enough at a quarter of 5e-5, of the elements set aside and of 3 max(lr); predict
within 5e-3 / 10 (the share of it the pair uses is printed: at most 0.36, bf16_cases.py); the decoder-only bounds within a
quarter, being 4 x these very figures.

Measured (the figures each case prints), largest over the lists: losses 0.24 of their bound (r6 CELU layer by layer),
share 0.17 of the allowed (WIDE[1] on its replaced seed; 0.14 r6 Identity), maximum 0.21 of its bound (r6 Identity layer by
layer), SGD 9.7e-6."""
import numpy as np
import pytest

import bf16_cases as C
import fuzz_cases as F

STEP_CASES = C.all_step_cases()


def test_the_lists_hold_what_the_gpu_test_is_meant_to_run():
    assert len(C.REGULAR) == 28 and len(C.TINY) == 12 and len(C.R6) == 28 and len(C.WIDE) == 16 and len(C.DECODER) == 8
    assert len(set(C.REGULAR)) == 28 and len(set(C.TINY)) == 12 and len(set(C.R6)) == 28 and len(set(C.DECODER)) == 8
    cfgs = [(group, path, mk()[0]) for group, cid, mk, seed, path in STEP_CASES]
    # every path at least 4 times, and - among the regular cases - with dropout and with SGD at least once
    for path in F.PATHS:
        assert sum(p == path for g, p, c in cfgs) >= 4, path
        assert sum(p == path for s, p in C.REGULAR) == 4, path
        assert any(c["drop"] for g, p, c in cfgs if g == "regular" and p == path), ("no dropout case on", path)
        assert any(c["opt"] == "sgd" for g, p, c in cfgs if g == "regular" and p == path), ("no SGD case on", path)
    # every one of the 20 classes; each r6 class on both of its paths
    assert {c["act"] for g, p, c in cfgs} == set(F.ACTS + F.ACTS_R6)
    assert {(n, p) for s, n, p in C.R6} == {(n, p) for n in F.ACTS_R6 for p in ("default", "no_chain")}
    # batches beyond the fused output-layer kernel's 104 rows, and beyond one fused launch's 112 under BLOCKED_ANY
    assert any(c["B"] > 104 for g, p, c in cfgs)
    assert any(c["B"] > 112 for g, p, c in cfgs if p == "blocked_any")
    # tiny really is: one hidden unit, a code of one, two items, one document all occur in F.config(.., tiny=True)'s ranges
    tiny = [c for g, p, c in cfgs if g == "tiny"]
    assert all(c["h"] <= 8 and c["c"] <= 6 and c["B"] <= 5 and c["N"] < 40 for c in tiny)
    assert {p for s, p in C.TINY} == {"default", "no_chain"}
    # the wide group: both step forms of all eight shapes, decoder inputs of 209 .. 416 columns or a code beyond a slot
    assert {(k, cut) for k, cut in C.WIDE} == {(k, cut) for k in range(8) for cut in (False, True)}
    assert all(c["c"] + c["inc"] + 1 > 208 for g, p, c in cfgs if g == "wide")
    # refusals the GPU test asserts instead of skipping do occur: the cut form layer by layer
    assert any(c["cut"] and F.cut_fits(c) and F.cut_refused(c, p) for g, p, c in cfgs)
    # at most 1 in 10 seeds replaced
    assert 10 * len(C.REPLACED) <= len(STEP_CASES) + len(C.DECODER)
    assert C.DZ_TOL == 4 * C.DZ_PAIR_MAX and C.DECODE_TOL == 4 * C.DECODE_PAIR_MAX and C.PREDICT_TOL == 5e-3 / 10
    assert C.SGD_PAIR_MAX <= F.SGD_TOL / 4


FP32_DIGEST = [(753, 41, 59, 27, 0, "Tanh", 59804, 166, 0.0), (38, 1, 1, 5, 1, "Sigmoid", 442, 29, -3.8137),
               (552, 192, 47, 67, 0, "SELU", 96882, 353, 67.0), (900, 100, 50, 150, 300, "ELU", 387734, 867, 150.0)]


def test_the_fp32_fuzz_draws_what_it_drew():
    """The generator moved into tests/fuzz_cases.py: the fp32 tests' configurations and first batches, pinned by a digest of
    the values the parent commit's tests/test_fuzz_gpu.py drew (seed 3, seed 3 tiny, 503, WIDE[4])."""
    def digest(cfg, r):
        st = next(F.steps(cfg, r))
        return (cfg["N"], cfg["h"], cfg["c"], cfg["B"], cfg["inc"], cfg["act"], int(st["idx"].sum()), int(st["ip"][-1]),
                round(float(st["zr"].sum()), 4))
    got = [digest(*F.config(3)), digest(*F.config(3, tiny=True)), digest(*F.config(503)), digest(*F.wide_config(4, False))]
    assert got == FP32_DIGEST, got


@pytest.mark.parametrize("group,cid,mk,seed,path", [pytest.param(*c, id=f"{c[0]}-{c[1]}") for c in STEP_CASES if not (c[0] == "wide" and c[1].endswith("cut"))])
def test_oracle_and_twin_stay_within_a_quarter_of_every_cap(group, cid, mk, seed, path):
    """(a wide case's two step forms are one computation to the oracle: once)"""
    cfg, r = mk()
    la, lb, ora, twin, pred = C.run_pair(cfg, r, seed)
    kw, p, lr = F.model_kwargs(cfg)
    loss = float(np.max(np.abs(la - lb) / (2e-4 * np.abs(la) + 2e-6)))
    if cfg["opt"] == "sgd":
        worst = 0.0
        for k, w in ora.p.items():
            d = np.abs(twin.p[k] - w)
            allowed = max(8, 0.01 * d.size, 2 * (d.shape[-1] if d.ndim > 1 else 1))
            left = np.sort(d.ravel())[::-1][min(d.size - 1, int(allowed / 4)):]
            worst = max(worst, float(left[0]))
            assert (d > F.SGD_TOL / 4).sum() <= allowed / 4 and d.max() <= 3 * max(lr) / 4, (cfg, k, int((d > F.SGD_TOL / 4).sum()), allowed, d.max())
        print(f"BF16PAIR {group} {cid} sgd: losses {loss:.3f} of the bound; parameters {worst:.2e} beside a quarter of the elements set aside")
        assert worst <= C.SGD_PAIR_MAX
    else:
        stats = F.bf16_param_stats(twin.p, ora.p, max(lr), 3)
        share, mx = max(f / a for f, a, m, b in stats.values()), max(m / b for f, a, m, b in stats.values())
        print(f"BF16PAIR {group} {cid} adam: losses {loss:.3f} of the bound; share {share:.3f} of the allowed; maximum {mx:.3f} of its bound")
        for k, (f, a, m, b) in stats.items():
            assert f <= a / 4 and m <= b / 4, (cfg, k, f, a, m, b)
    assert loss <= 0.25, (cfg, la, lb)
    if pred is not None:
        d = float(np.abs(pred[0] - pred[1]).max())
        print(f"BF16PAIR {group} {cid} predict {d / C.PREDICT_TOL:.3f} of the bound")
        assert d <= C.PREDICT_TOL


@pytest.mark.parametrize("seed", C.DECODER)
def test_decoder_oracle_and_twin_stay_within_a_quarter_of_every_cap(seed):
    la, lb, ora, twin, dz, pred, info = C.run_decoder_pair(seed)
    loss = float(np.max(np.abs(la - lb) / (2e-4 * np.abs(la) + 2e-6)))
    stats = F.bf16_param_stats(twin.p, ora.p, 2e-3, 3)
    share, mx = max(f / a for f, a, m, b in stats.values()), max(m / b for f, a, m, b in stats.values())
    a, b = dz[0]
    d0 = float(np.abs(a.astype(np.float64) - b).max() / np.abs(a).max())
    dp = float(np.abs(pred[0] - pred[1]).max())
    print(f"BF16PAIR decoder {seed} {info}: losses {loss:.3f} of the bound; share {share:.3f} of the allowed; maximum {mx:.3f} of its bound; "
          f"first step's dz {d0:.2e} of max |dz|; decode {dp:.2e}")
    assert loss <= 0.25
    for k, (f, al, m, bd) in stats.items():
        assert f <= al / 4 and m <= bd / 4, (info, k, f, al, m, bd)
    assert d0 <= C.DZ_TOL / 4 and dp <= C.DECODE_TOL / 4


def test_oracle_decoder_in_bf16_mode_rounds_what_the_autoencoders_decoder_rounds():
    """OracleDecoder(bf16=True) against the decoder half of OracleAAE(bf16=True).ae_step on the same input block and batch:
    the same loss and the same decoder parameters after the step, bit for bit (one restatement: _mlp_fwd / _mlp_bwd); and it
    differs from the fp32 OracleDecoder, so the flag does something."""
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    r = np.random.default_rng(5)
    N, h, c, B = 90, 21, 9, 13
    params = init_params(N, h, c, seed=5)
    ip, idx, val = F.batch(r, N, B, B)
    kw = dict(activation="Tanh", dropout=(0.0, 0.0))
    aae = O.OracleAAE(params, gen_lr=2e-3, bf16=True, **kw)
    loss_a = aae.ae_step(ip, idx, val, None)
    z = aae.last["z"]
    dec = O.OracleDecoder(params, lr=2e-3, conditions=[O.ConcatConst(c)], bf16=True, **kw)
    loss_d = dec.partial_fit([z], ip, idx, val)
    assert loss_a == loss_d
    for k, w in dec.p.items():
        assert np.array_equal(w, aae.p[k]), k
    plain = O.OracleDecoder(params, lr=2e-3, conditions=[O.ConcatConst(c)], **kw)
    assert plain.bf16 is False and plain.partial_fit([z], ip, idx, val) != loss_d
