"""The cases of the fp32 fuzz on the forced execution paths (tests/test_fuzz_paths_cpu.py, tests/test_fuzz_paths_gpu.py): the
fp32 sibling of tests/bf16_cases.py.

A case is a configuration of tests/fuzz_cases.py (the fp32 fuzz's generator and step loop, the same implementation) run as an
fp32 HipAAE created under one of the library's path switches (fuzz_cases.PATHS) against OracleAAE: three steps, the last one
shorter, the cut at the output layer and predict where the configuration draws them, at the fp32 fuzz's own tolerances.
SPLIT_ANY and BLOCKED_ANY are what bring random shapes to the three-term fp32 instantiations of dec_crit_x3_kernel,
dec_opt_x3_kernel and dec_opt_blocks_x3_kernel; the profile's launch counters say that they ran (fuzz_cases.output_form).

tests/test_fuzz_paths_cpu.py runs every step case through the oracle and through its twin with rounding off
(bf16_cases._Twin, bf16=False: float64 accumulation of every dense product, hidden activations moved by 4 units in the last
place) and asserts that the two differ by at most a QUARTER of each cap: three quarters are the device's."""
import fuzz_cases as F

# ---- the groups ----------------------------------------------------------------------------------------------------------------
PATH_CYCLE = [p for p in F.PATHS if p != "default"]       # kslices, chain16, no_chain, x16, split_any, blocked_any


def regular_at(first):
    return [(first + i, PATH_CYCLE[i % len(PATH_CYCLE)]) for i in range(24)]


def regular_ok(cases):
    """What the regular list has to hold (the issue's conditions; test_fuzz_paths_cpu.py asserts them of REGULAR)."""
    cfgs = [(path, F.config(seed)[0]) for seed, path in cases]
    on = lambda path: [c for p, c in cfgs if p == path]       # noqa: E731
    return (all(any(c["drop"] for c in on(p)) and any(c["opt"] == "sgd" for c in on(p)) for p in PATH_CYCLE) and
            any(c["window"] for c in on("split_any")) and any(c["long_rows"] for c in on("split_any")) and
            sum(c["B"] <= F.FUSED_ROWS for c in on("split_any")) >= 3 and sum(c["B"] > F.LAUNCH_ROWS for c in on("blocked_any")) >= 2)


# regular: 24 consecutive seeds of F.config, the path cycling over the six forced paths (four seeds each).  The first seed is the
# smallest from 700 on (clear of the fp32 fuzz's 0 .. 27 and 500 .. 527 and of the bf16 fuzz's 443 .. 470 and 600 .. 627) for which
# regular_ok holds (it is 851): every path with a dropout case and an SGD case, SPLIT_ANY with a window case, a long_rows case and at least
# three batches of one fused launch, BLOCKED_ANY with at least two batches above 112 rows.
REGULAR_FIRST = 851
REGULAR = regular_at(REGULAR_FIRST)
# tiny: F.config(seed, tiny=True) - one hidden unit, two items, one document - through the split form, layer by layer and on
# chain16x3_kernel's row threshold
TINY = [(200 + i, ["split_any", "no_chain", "x16"][i % 3]) for i in range(12)]
# r6: each of the fourteen further activation classes once, the path cycling
R6 = [(1200 + k, name, ["no_chain", "x16", "chain16", "split_any"][k % 4]) for k, name in enumerate(F.ACTS_R6)]
# wide conditions: F.WIDE on SPLIT_ANY, whole step and cut form, predict
WIDE = [(case, cut) for case in range(len(F.WIDE)) for cut in (False, True)]
# decoder-only (aae_decoder_step, seeds of F.decoder_config) and VAE (aae_vae_step; F.check_vae draws behind the same opening)
DECODER = [(200 + i, path) for i in range(4) for path in ("split_any", "no_chain")]
VAE = [(211 + 2 * i, path) for i in range(4) for path in ("no_chain", "x16")]

# Seeds replaced because oracle and twin alone disagree by more than a quarter of a cap: (group, case) -> (seed generated, its
# replacement, the measured figures).
REPLACED = {}


def r6_config(seed, name):
    cfg, r = F.config(seed)
    cfg["act"] = name
    # (as tests/test_fuzz_gpu.py: with one of these classes a decoder input wider than a slot runs layer by layer, where the
    #  library refuses the cut form - the whole step there)
    if cfg["c"] + cfg["inc"] + 1 > 208:
        cfg["cut"] = False
    return cfg, r


def all_step_cases():
    """(group, id, cfg factory, seed for init_params, path) of every case that runs whole steps"""
    out = []
    for seed, path in REGULAR:
        out.append(("regular", f"{seed}-{path}", lambda seed=seed: F.config(seed), seed, path))
    for seed, path in TINY:
        out.append(("tiny", f"{seed}-{path}", lambda seed=seed: F.config(seed, tiny=True), seed, path))
    for seed, name, path in R6:
        out.append(("r6", f"{name}-{path}", lambda seed=seed, name=name: r6_config(seed, name), seed, path))
    for case, cut in WIDE:
        out.append(("wide", f"{case}-{'cut' if cut else 'step'}", lambda case=case, cut=cut: F.wide_config(case, cut), 7000 + case, "split_any"))
    return out


def step_rows(cfg, r):
    """The rows of a case's three steps (the last one is shorter by a draw of the batches' generator)."""
    return [st["Bs"] for st in F.steps(cfg, r)]


# Cases on SPLIT_ANY / BLOCKED_ANY with a step that does NOT run the split form, and why: (group, id) -> reason.  The GPU test
# asserts of every step of every such case the form F.output_form names - that it fell back, and to what;
# test_fuzz_paths_cpu.py asserts that this table names exactly the cases F.output_form says fall back.
FALLBACK = {
    ("regular", "856-blocked_any"): "12 rows: one row block, and BLOCKED_ANY lifts the row-blocked form's size cap alone - the single launch",
    ("regular", "874-blocked_any"): "42 rows: one row block, and BLOCKED_ANY lifts the row-blocked form's size cap alone - the single launch",
    ("r6", "Softshrink-split_any"): "111 rows: one row block whose LDS image of dh2 does not fit (109 rows do) - the three GEMMs; the 97-row last batch splits",
    ("r6", "SiLU-split_any"): "249 rows on a handle without blocked_output: beyond one fused launch - the three GEMMs",
    ("wide", "4-step"): "150 rows on a handle without blocked_output: beyond one fused launch - the three GEMMs",
    ("wide", "4-cut"): "150 rows on a handle without blocked_output: beyond one fused launch - the three GEMMs",
    ("decoder", "201-split_any"): "114 rows on a handle without blocked_output: beyond one fused launch - the three GEMMs",
}
