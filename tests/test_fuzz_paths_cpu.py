"""The fp32 fuzz on the forced paths without a GPU: what the case lists of tests/fuzz_path_cases.py hold, and that the reference
alone stays inside a quarter of every cap tests/test_fuzz_paths_gpu.py holds the device to.

Each step case runs through OracleAAE and through its twin with rounding off (bf16_cases._Twin, bf16=False: float64
accumulation of every dense product the two share, hidden activations moved by 4 units in the last place wherever the class
evaluates a library function).  The two differ the way two correct fp32 implementations may: another summation order, and a
transcendental within its error bound.

Asserted per case, each at a QUARTER of the fp32 fuzz's cap: losses (rtol 5e-5, atol 2e-6); parameters - the elements beyond 5e-5
against the share close_enough sets aside, the largest difference against 3 max(lr); predict against 1e-4.

Measured (the FUZZPAIR lines), largest over the lists: losses 0.004 of their bound (tiny 210 layer by layer); no element of any
tensor beyond 5e-5 in any case; the largest difference 0.002 of 3 lr (WIDE[1]); predict 0.001 of its bound.  No seed had to be
replaced (fuzz_path_cases.REPLACED is empty)."""
import numpy as np
import pytest

import bf16_cases as C
import fuzz_cases as F
import fuzz_path_cases as P

STEP_CASES = P.all_step_cases()


def test_the_lists_hold_what_the_gpu_test_is_meant_to_run():
    assert len(P.REGULAR) == 24 and len(P.TINY) == 12 and len(P.R6) == 14 and len(P.WIDE) == 16
    assert len(set(P.REGULAR)) == 24 and len(set(P.TINY)) == 12 and len(set(P.R6)) == 14
    # regular: consecutive seeds clear of the other fuzz lists, the six forced paths four times each, and the first seed is the
    # smallest from 700 on that keeps the properties below
    seeds = [s for s, p in P.REGULAR]
    assert seeds == list(range(P.REGULAR_FIRST, P.REGULAR_FIRST + 24)) and P.REGULAR_FIRST >= 700
    taken = set(range(0, 28)) | set(range(443, 471)) | set(range(500, 528)) | set(range(600, 628))
    assert not taken & set(seeds) and not taken & {s for s, n, p in P.R6}
    assert P.PATH_CYCLE == ["kslices", "chain16", "no_chain", "x16", "split_any", "blocked_any"]
    assert all(sum(p == path for s, p in P.REGULAR) == 4 for path in P.PATH_CYCLE)
    assert P.regular_ok(P.REGULAR)
    assert not any(P.regular_ok(P.regular_at(first)) for first in range(700, P.REGULAR_FIRST))
    cfgs = {path: [F.config(s)[0] for s, p in P.REGULAR if p == path] for path in P.PATH_CYCLE}
    for path in P.PATH_CYCLE:       # (regular_ok, spelled out)
        assert any(c["drop"] for c in cfgs[path]), ("no dropout case on", path)
        assert any(c["opt"] == "sgd" for c in cfgs[path]), ("no SGD case on", path)
    assert any(c["window"] for c in cfgs["split_any"]) and any(c["long_rows"] for c in cfgs["split_any"])
    assert sum(c["B"] <= 109 for c in cfgs["split_any"]) >= 3
    assert sum(c["B"] > 112 for c in cfgs["blocked_any"]) >= 2
    # tiny: degenerate sizes over the three paths
    assert {p for s, p in P.TINY} == {"split_any", "no_chain", "x16"}
    assert all(c["h"] <= 8 and c["c"] <= 6 and c["B"] <= 5 and c["N"] < 40 for c in (F.config(s, tiny=True)[0] for s, p in P.TINY))
    # r6: each further class once, the four paths cycling; no cut form where the decoder input is wider than a slot
    assert [n for s, n, p in P.R6] == F.ACTS_R6
    assert [p for s, n, p in P.R6] == [["no_chain", "x16", "chain16", "split_any"][k % 4] for k in range(14)]
    assert not any(cfg["cut"] and cfg["c"] + cfg["inc"] + 1 > 208 for cfg in (P.r6_config(s, n)[0] for s, n, p in P.R6))
    # wide: both step forms of all eight shapes, on SPLIT_ANY
    assert set(P.WIDE) == {(k, cut) for k in range(8) for cut in (False, True)}
    assert all(path == "split_any" for g, cid, mk, seed, path in STEP_CASES if g == "wide")
    # decoder-only: four seeds on SPLIT_ANY and layer by layer; VAE: four seeds layer by layer (refused) and on X16_ROWS
    assert len(P.DECODER) == 8 and {p for s, p in P.DECODER} == {"split_any", "no_chain"} and len({s for s, p in P.DECODER}) == 4
    assert len(P.VAE) == 8 and {p for s, p in P.VAE} == {"no_chain", "x16"} and len({s for s, p in P.VAE}) == 4
    assert all(s % 2 for s, p in P.VAE)        # (the fp32 fuzz runs its VAE branch on odd seeds)
    # refusals the GPU test asserts instead of skipping do occur: the cut form layer by layer
    assert any(c["cut"] and F.cut_fits(c) and F.cut_refused(c, p) for c, p in ((mk()[0], path) for g, cid, mk, seed, path in STEP_CASES))
    assert 10 * len(P.REPLACED) <= len(STEP_CASES)


def test_output_form_restates_the_library_rule():
    """output_form (csrc/abi_chains.h) for an fp32 handle of the fuzz's sizes, at the row counts where the form changes."""
    for rows, split_any, blocked_any in ((1, "split", "single"), (109, "split", "single"), (110, "three", "three"), (112, "three", "three"),
                                         (113, "three", "split"), (208, "three", "split"), (209, "three", "split"), (1664, "three", "split"),
                                         (1665, "three", "three")):
        assert F.output_form("split_any", rows) == split_any and F.output_form("blocked_any", rows) == blocked_any, rows


def test_the_fallback_table_names_exactly_the_cases_that_fall_back():
    """Every SPLIT_ANY case of at most 109 rows and every BLOCKED_ANY case above 112 runs the split form on each of its steps;
    the others are in FALLBACK with the reason."""
    falls = set()
    for g, cid, mk, seed, path in STEP_CASES:
        if path not in ("split_any", "blocked_any"):
            continue
        cfg, r = mk()
        forms = [F.output_form(path, b) for b in P.step_rows(cfg, r)]
        if path == "split_any" and cfg["B"] <= 109 or path == "blocked_any" and cfg["B"] > 112:
            assert forms == ["split"] * 3, (g, cid, forms)
        else:
            assert "split" != forms[0], (g, cid, forms)
            falls.add((g, cid))
    for seed, path in P.DECODER:
        if path == "split_any" and F.output_form(path, F.decoder_config(seed)[3]) != "split":
            falls.add(("decoder", f"{seed}-{path}"))
    assert falls == set(P.FALLBACK), (falls ^ set(P.FALLBACK))
    split_decoders = [s for s, p in P.DECODER if p == "split_any" and F.decoder_config(s)[3] <= 109]
    assert len(split_decoders) >= 2


def pair_figures(cfg, la, lb, ora, twin, pred):
    """(losses, share of the allowed, maximum, predict) as fractions of the fp32 fuzz's caps"""
    kw, p, lr = F.model_kwargs(cfg)
    loss = float(np.max(np.abs(la - lb) / (5e-5 * np.abs(la) + 2e-6)))
    share = mx = 0.0
    for k, w in ora.p.items():
        d = np.abs(twin.p[k] - w)
        allowed = max(8, 0.01 * d.size, 2 * (d.shape[-1] if d.ndim > 1 else 1))
        share, mx = max(share, float((d > 5e-5).sum() / allowed)), max(mx, float(d.max() / (3 * max(lr))))
    pr = float(np.abs(pred[0] - pred[1]).max() / 1e-4) if pred is not None else 0.0
    return loss, share, mx, pr


@pytest.mark.parametrize("group,cid,mk,seed,path", [pytest.param(*c, id=f"{c[0]}-{c[1]}") for c in STEP_CASES if not (c[0] == "wide" and c[1].endswith("cut"))])
def test_oracle_and_twin_stay_within_a_quarter_of_every_cap(group, cid, mk, seed, path):
    """(a wide case's two step forms are one computation to the oracle: once)"""
    cfg, r = mk()
    loss, share, mx, pr = pair_figures(cfg, *C.run_pair(cfg, r, seed, bf16=False))
    print(f"FUZZPAIR {group} {cid} {cfg['opt']}: losses {loss:.3f} of the bound; share beyond 5e-5 {share:.3f} of the allowed; maximum {mx:.4f} of 3 lr; predict {pr:.3f} of 1e-4")
    assert loss <= 0.25 and share <= 0.25 and mx <= 0.25 and pr <= 0.25, (cfg, loss, share, mx, pr)
