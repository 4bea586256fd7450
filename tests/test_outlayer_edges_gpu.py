"""The decoder's output layer ALONE at the shape edges of its kernels, every form against float64 (tests/outlayer_cases.py has
the cases, the inputs, the restatement and the tolerances): HipAAE.output_layer_step on a handle with a code of 10, two
consecutive calls on a different batch each with non-zero Adam moments loaded at step count 5.

Forms: the single launch (dec_fused_kernel); the split form at its default width and at aae_set_split(1), where one workgroup of
the deferred launch walks every tile (dec_crit_x3_kernel + dec_opt_x3_kernel, three-term fp32); the three-kernel path; beyond
112 rows the row-blocked form (dec_crit_x3_kernel over row blocks + dec_opt_blocks_x3_kernel); SGD on four cases, where the
moments must come back bitwise as they were loaded.  The profile's launch counters say which form ran.

Compared with the float64 restatement, each relative to the quantity's largest magnitude: the loss and dL/d(dh2) of both calls,
dec.lin3.weight and bias and both moments of both after the second call.  The tolerances are four times what the fp32
restatement alone differs from float64 by (outlayer_cases.TOL; tests/test_outlayer_edges_cpu.py).  Every run prints observed /
allowed per quantity (OUTEDGE lines; DESIGN.md holds the worst per form)."""
import numpy as np
import pytest
import torch

import fuzz_cases as F
import outlayer_cases as C

pytestmark = pytest.mark.gpu


def run_form(cid, form):
    """The case's two calls on a handle of `form` -> (results by C.QUANTITIES, launches by kernel id)"""
    from aaerec import _hip
    from aaerec._hip import HipAAE, DeviceCSR
    import scipy.sparse as sp
    c, x = C.BY_ID[cid], C.inputs(cid)
    N, h, B = c["N"], c["h"], c["B"]
    kw, option, width, ran, not_ran = C.FORMS[form]
    if option:
        _hip.set_option(option, 1)
    try:        # (a handle reads its switches once, at creation)
        m = HipAAE(N, h, 10, max_batch=B, max_nnz=B * N, rng_mode="inject", gen_lr=C.LR, **kw)
    finally:
        if option:
            _hip.set_option(option, None)
    mom = x["mom"]
    m.load_params({"dec.lin3.weight": x["w"], "dec.lin3.bias": x["b"]})
    m.load_adam(_hip.O_DEC, 3, mom["m_w"], mom["v_w"], mom["m_b"], mom["v_b"], step=C.ADAM_STEP)
    m.set_grad_scale(C.GRAD_SCALE)
    if width is not None:
        m.set_split(width)
    m.profile_enable(True, kernels=F.OUT_KERNELS)
    indptr, indices, values = x["corpus"]
    csr = DeviceCSR(sp.csr_matrix((values, indices, indptr), shape=(x["n_docs"], N)), m.device)
    losses, da2s = [], []
    for call in range(2):
        rows = torch.as_tensor(x["pick"][call], device=m.device) if x["pick"] is not None else None
        m.dh2_rows(B)[:, :h + 1].copy_(torch.from_numpy(x["dh2"][call]))
        m.output_layer_step(csr, call * B, B, rows=rows)
        losses.append(m.losses()[0])
        da2s.append(m.da2_rows(B)[:, :h].cpu().numpy())
    torch.cuda.synchronize()
    counts = {k: m.profile_read(k)[1] for k in F.OUT_KERNELS}
    sd, st = m.state_dict(), m.adam_state("dec")
    got = dict(loss=np.asarray(losses), da2=np.stack(da2s), w=sd["dec.lin3.weight"], b=sd["dec.lin3.bias"],
               m_w=st["lin3.weight"][0], v_w=st["lin3.weight"][1], m_b=st["lin3.bias"][0], v_b=st["lin3.bias"][1])
    got = {k: np.array(v, copy=True) for k, v in got.items()}
    got["adam_step"] = st["step"]
    m.close()
    return got, counts


@pytest.mark.parametrize("cid,form", C.RUNS, ids=[f"{cid}-{form}" for cid, form in C.RUNS])
def test_output_layer_at_a_shape_edge_matches_float64(cid, form):
    optimizer = "sgd" if form.endswith("sgd") else "adam"
    ref, x = C.reference(cid, optimizer), C.inputs(cid)
    assert ref["max_logit"] < 12.0
    got, counts = run_form(cid, form)
    kw, option, width, ran, not_ran = C.FORMS[form]
    d = C.distance(got, ref, optimizer)
    print(f"OUTEDGE {cid} {form}: " + "  ".join(f"{q} {v:.2e} / {C.TOL[q]:.1e}" for q, v in d.items()) + f"  launches {counts}")
    # (every check of the run is evaluated before the first one fails the test: the message names all that miss)
    checks = {f"{q} within {C.TOL[q]:.1e} of its largest magnitude ({v:.3e})": v <= C.TOL[q] for q, v in d.items()}
    checks[f"launches {counts}: ran {ran}, not {not_ran}"] = all(counts[k] == 2 for k in ran) and all(counts[k] == 0 for k in not_ran)
    checks["the calls changed the parameters"] = not np.array_equal(got["w"], x["w"]) and not np.array_equal(got["b"], x["b"])
    if optimizer == "sgd":
        for q in ("m_w", "v_w", "m_b", "v_b"):
            checks[f"SGD: {q} bitwise as loaded"] = np.array_equal(got[q], x["mom"][q])
    else:
        checks["Adam: both moments moved"] = not np.array_equal(got["m_w"], x["mom"]["m_w"]) and not np.array_equal(got["v_w"], x["mom"]["v_w"])
        checks[f"Adam's step count {got['adam_step']} is {C.ADAM_STEP + 2}"] = got["adam_step"] == C.ADAM_STEP + 2
    assert all(checks.values()), (cid, form, [k for k, ok in checks.items() if not ok])
