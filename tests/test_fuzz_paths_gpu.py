"""Randomised differential test of the fp32 step on every execution path a handle can be forced onto: HipAAE created under
CHAIN_KSLICES, CHAIN16, NO_CHAIN, X16_ROWS = 16, SPLIT_ANY or BLOCKED_ANY (a blocked_output handle) against OracleAAE, over the
configurations of the fp32 fuzz's generator (tests/fuzz_cases.py: one implementation for all three fuzz tests) at the fp32 fuzz's
own tolerances - losses rtol 5e-5 / atol 2e-6, parameters close_enough(.., 5e-5, 3 max(lr)), predict atol 1e-4, the decoder's and
the VAE's figures as tests/test_fuzz_gpu.py has them.

  regular   24 seeds, the path cycling over the six forced paths
  tiny      12 seeds of degenerate sizes on SPLIT_ANY, NO_CHAIN and X16_ROWS
  r6        each of the fourteen further activation classes once, over NO_CHAIN, X16_ROWS, CHAIN16 and SPLIT_ANY
  wide      the eight decoder inputs wider than a chain slot on SPLIT_ANY, whole step and the cut at the output layer, predict
  decoder   aae_decoder_step on SPLIT_ANY and NO_CHAIN; aae_vae_step on X16_ROWS, and its refusal on NO_CHAIN

SPLIT_ANY and BLOCKED_ANY are what bring these shapes to the three-term fp32 instantiations of dec_crit_x3_kernel,
dec_opt_x3_kernel and dec_opt_blocks_x3_kernel.  A forced path can fall back silently, so every case on those two paths reads the
profile's launch counters after each step: a batch of at most 109 rows on SPLIT_ANY and a batch above 112 rows on BLOCKED_ANY must
have run the critical and the deferred launch and neither the single launch nor the three-kernel path's first GEMM; the cases
that legitimately take another form are named in fuzz_path_cases.FALLBACK with the reason, and assert that form
(fuzz_cases.output_form).  tests/test_fuzz_paths_cpu.py shows that the reference alone stays inside a quarter of each tolerance.

  corner    the regular BLOCKED_ANY cases above 112 rows once more on a handle created with max_batch = 1700 - more than the 16 row
            blocks of 104 rows a row-blocked batch can have: its batches of 113 .. 1664 rows run the row-blocked form like any
            other blocked_output handle's (dec_opt_blocks_x3_kernel), at the same tolerances."""
import pytest

import fuzz_cases as F
import fuzz_path_cases as P

pytestmark = pytest.mark.gpu


def _check(group, cid, cfg, r, seed, path):
    counted = path in ("split_any", "blocked_any")
    counters = [] if counted else None
    F.check_configuration(cfg, r, seed, path=path, counters=counters)
    if counted:
        F.assert_output_form(path, counters, f"{group} {cid}")
        forms = [F.output_form(path, rows) for rows, _ in counters]
        print(f"FUZZPATH {group} {cid}: rows {[rows for rows, _ in counters]} forms {forms} launches (bce_fwd, single, critical, deferred) {[c for _, c in counters]}")
        assert ((group, cid) in P.FALLBACK) == (forms[0] != "split"), (group, cid, forms)


@pytest.mark.parametrize("seed,path", P.REGULAR)
def test_fp32_random_configuration_on_a_forced_path_matches_oracle(seed, path):
    cfg, r = F.config(seed)
    _check("regular", f"{seed}-{path}", cfg, r, seed, path)


CORNER_MAX_BATCH = 1700      # > 16 row blocks x 104 rows
CORNER = [(seed, path) for seed, path in P.REGULAR if path == "blocked_any" and F.config(seed)[0]["B"] > F.LAUNCH_ROWS]


@pytest.mark.parametrize("seed,path", CORNER)
def test_fp32_row_blocked_batch_on_a_handle_with_a_larger_max_batch_matches_oracle(seed, path):
    assert len(CORNER) >= 2         # (fuzz_path_cases.regular_ok)
    cfg, r = F.config(seed)
    counters = []
    F.check_configuration(cfg, r, seed, path=path, counters=counters, max_batch=CORNER_MAX_BATCH)
    F.assert_output_form(path, counters, f"corner {seed}")
    forms = [F.output_form(path, rows) for rows, _ in counters]
    print(f"FUZZPATH corner {seed}: rows {[rows for rows, _ in counters]} forms {forms} launches (bce_fwd, single, critical, deferred) {[c for _, c in counters]}")
    assert forms == ["split"] * 3, forms


@pytest.mark.parametrize("seed,path", P.TINY)
def test_fp32_degenerate_sizes_on_a_forced_path_match_oracle(seed, path):
    cfg, r = F.config(seed, tiny=True)
    _check("tiny", f"{seed}-{path}", cfg, r, seed, path)


@pytest.mark.parametrize("seed,name,path", P.R6)
def test_fp32_further_activation_class_on_a_forced_path_matches_oracle(seed, name, path):
    cfg, r = P.r6_config(seed, name)
    _check("r6", f"{name}-{path}", cfg, r, seed, path)


@pytest.mark.parametrize("case,cut", P.WIDE)
def test_fp32_condition_wider_than_a_chain_slot_on_the_split_form_matches_oracle(case, cut):
    cfg, r = F.wide_config(case, cut)
    _check("wide", f"{case}-{'cut' if cut else 'step'}", cfg, r, 7000 + case, "split_any")


@pytest.mark.parametrize("seed,path", P.DECODER)
def test_fp32_decoder_step_on_a_forced_path_matches_oracle(seed, path):
    r, N, h, B, act = F.decoder_config(seed)
    counters = [] if path == "split_any" else None
    F.check_decoder(r, N, h, B, act, seed, path=path, counters=counters)
    if counters is not None:
        F.assert_output_form(path, counters, f"decoder {seed}")
        assert (("decoder", f"{seed}-{path}") in P.FALLBACK) == (F.output_form(path, B) != "split")


@pytest.mark.parametrize("seed,path", P.VAE)
def test_fp32_vae_step_on_a_forced_path_matches_oracle(seed, path):
    r, N, h, B, act = F.decoder_config(seed)
    F.check_vae(r, N, h, B, act, seed, path=path)
