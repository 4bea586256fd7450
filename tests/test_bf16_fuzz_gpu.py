"""Randomised differential test of bf16 mode: HipAAE(.., dtype='bf16') against OracleAAE(.., bf16=True) - every matrix-core
product with both operands rounded to bf16, everything else fp32: the mode's definition - over the configurations of the fp32
fuzz's generator (tests/fuzz_cases.py: one implementation for both), on every execution path a handle can be forced onto.

  regular   28 seeds, the path cycling: default (the column-owner chain4 of bf16 mode), CHAIN_KSLICES, CHAIN16, NO_CHAIN (kGemmBf16
            and its per-layer epilogues), X16_ROWS = 16 (chain16x3_kernel<true>), SPLIT_ANY, BLOCKED_ANY (blocked_output handles)
  tiny      12 seeds of degenerate sizes, default path and layer by layer
  r6        each of the fourteen further activation classes on chain_kernel<true, true> and layer by layer
  wide      the eight decoder inputs wider than a chain slot, whole step and the cut at the output layer, predict
  decoder   aae_decoder_step against OracleDecoder(bf16=True)

Three steps, the last one shorter; the cut at the output layer where the configuration draws it - where the library refuses it
(AAE_ESTATE: hidden layers that run layer by layer) the test asserts the status and the message and takes the whole step.
Tolerances: tests/test_bf16_gpu.py's, and tests/bf16_cases.py for the two it has none for; tests/test_bf16_fuzz_cpu.py shows
that the reference alone stays inside a quarter of each.  Every case prints the observed share and maximum per tensor
(BF16FUZZ lines; DESIGN.md's table holds the worst per group).

  corner    the first regular BLOCKED_ANY case above 112 rows once more on a handle created with max_batch = 1700 (more than 16 row
            blocks of 104 rows): its batches run the row-blocked form, not the three GEMMs - the launch counters say so."""
import pytest

import bf16_cases as C
import fuzz_cases as F

pytestmark = pytest.mark.gpu


def _report(group, cid, path, stats):
    for k, (frac, allowed, mx, bound) in stats.items():
        print(f"BF16FUZZ {group} {cid} {path} {k}: share {frac:.5f}" + (f" (allowed {allowed:.5f})" if allowed is not None else "") + f" max {mx:.3e} (bound {bound:.1e})")


@pytest.mark.parametrize("seed,path", C.REGULAR)
def test_bf16_random_configuration_matches_the_rounded_oracle(seed, path):
    cfg, r = C.regular_config(seed)
    _report("regular", seed, path, F.check_configuration(cfg, r, seed, bf16=True, path=path))


CORNER = [(seed, path) for seed, path in C.REGULAR if path == "blocked_any" and C.regular_config(seed)[0]["B"] > F.LAUNCH_ROWS][:1]


@pytest.mark.parametrize("seed,path", CORNER)
def test_bf16_row_blocked_batch_on_a_handle_with_a_larger_max_batch_matches_the_rounded_oracle(seed, path):
    assert len(CORNER) == 1         # (test_bf16_fuzz_cpu.py: the lists hold a BLOCKED_ANY batch above 112 rows)
    cfg, r = C.regular_config(seed)
    counters = []
    _report("corner", seed, path, F.check_configuration(cfg, r, seed, bf16=True, path=path, counters=counters, max_batch=1700))
    # (a bf16 handle's single launch keeps no LDS image of dh2: every batch above 112 rows of at most 16 row blocks is row-blocked)
    for step, (rows, counts) in enumerate(counters):
        assert rows > F.LAUNCH_ROWS and tuple(min(n, 1) for n in counts) == (0, 0, 1, 1), (f"step {step}, {rows} rows: launches of (bce_fwd, "
                                                                                           f"single, critical, deferred) {counts}")


@pytest.mark.parametrize("seed,path", C.TINY)
def test_bf16_degenerate_sizes_match_the_rounded_oracle(seed, path):
    cfg, r = C.tiny_config(seed)
    _report("tiny", seed, path, F.check_configuration(cfg, r, seed, bf16=True, path=path))


@pytest.mark.parametrize("seed,name,path", C.R6)
def test_bf16_further_activation_class_matches_the_rounded_oracle(seed, name, path):
    cfg, r = C.r6_config(seed, name)
    _report("r6", name, path, F.check_configuration(cfg, r, seed, bf16=True, path=path))


@pytest.mark.parametrize("case,cut", C.WIDE)
def test_bf16_condition_wider_than_a_chain_slot_matches_the_rounded_oracle(case, cut):
    cfg, r = F.wide_config(case, cut, C.WIDE_SEED[case])
    _report("wide", case, "cut" if cut else "step", F.check_configuration(cfg, r, C.WIDE_SEED[case], bf16=True))


@pytest.mark.parametrize("seed", C.DECODER)
def test_bf16_decoder_step_matches_the_rounded_oracle(seed):
    r, N, h, B, act = F.decoder_config(seed)
    _report("decoder", seed, "default", F.check_decoder(r, N, h, B, act, seed, bf16=True, dz_tol=C.DZ_TOL, decode_tol=C.DECODE_TOL))


def test_bf16_refuses_the_vae():
    """(the combinations bf16 mode refuses) aae_arena_bytes / aae_create: AAE_EINVAL and the reason."""
    from aaerec import _hip
    with pytest.raises(_hip.AaeHipError, match=r"error -1: bf16 arithmetic is not available in VAE mode"):
        _hip.HipAAE(100, 20, 5, max_batch=8, rng_mode="inject", vae=True, dtype="bf16")
