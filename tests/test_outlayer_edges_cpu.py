"""The output-layer edge sweep without a GPU: what tests/outlayer_cases.py holds, that its float64 restatement is the reference's
computation (torch autograd and torch.optim.Adam on the same inputs), and how far the fp32 restatement
(test_bce_saturation_gpu.Restatement, the reference's arithmetic) lies from the float64 one - the figure every tolerance of
tests/test_outlayer_edges_gpu.py is four times of.  Asserted for every case: no quantity beyond PAIR_MAX, a QUARTER of its
tolerance; and that the maxima recorded in outlayer_cases.py are the measured ones (none is more than 10 % above what the list
gives, so a tolerance cannot outlive the case that set it)."""
import numpy as np
import pytest

import outlayer_cases as C

_seen = {}


def test_the_list_holds_the_edges():
    ids = [c["id"] for c in C.CASES]
    assert len(set(ids)) == len(ids) and 40 <= len(ids) <= 70
    shapes = {(c["N"], c["h"], c["B"]) for c in C.CASES}
    N0, h0, B0 = C.BASE
    assert C.BASE == (167, 100, 37)
    assert {h for N, h, B in shapes if (N, B) == (N0, B0)} >= {1, 2, 15, 16, 47, 62, 63, 64, 95, 96, 110, 111, 112, 175, 191, 192, 206, 207}
    assert {B for N, h, B in shapes if (N, h) == (N0, 207)} >= {1, 15, 16, 17, 48, 49, 63, 64, 65, 96, 97, 104, 108, 109}
    assert len({B for N, h, B in shapes if (N, h) == (N0, 100) and B <= 109}) >= 4 and len({B for N, h, B in shapes if (N, h) == (N0, 40)}) >= 4
    assert {N for N, h, B in shapes if (h, B) == (h0, B0)} >= {2, 31, 32, 33, 63, 64, 65, 167, 8500}
    for h in (100, 207):
        assert {B for N, hh, B in shapes if (N, hh) == (N0, h) and B > 112} == {113, 208, 209, 230, 313}
        assert {B for N, hh, B in shapes if (N, hh) == (33, h)} >= {113, 313}
    # the column-block counts of the h edges: 4, 7 and 13 blocks with the last one full, holding one column, and the count's change
    nb = lambda h: 4 if h + 1 <= 64 else 7 if h + 1 <= 112 else 13       # noqa: E731
    assert [nb(h) for h in (62, 63, 64, 110, 111, 112, 206, 207)] == [4, 4, 7, 7, 7, 13, 13, 13]
    # forms: every batch of one launch on all four forms, the others row-blocked; SGD on four cases
    for c in C.CASES:
        assert set(c["forms"]) >= (set(C.ONE_LAUNCH) if c["B"] <= 109 else {"blocked"}), c["id"]
        assert c["B"] <= 109 or c["B"] > 112
    assert sum(any(f.endswith("sgd") for f in c["forms"]) for c in C.CASES) == 4
    assert sum(c["window"] for c in C.CASES) >= len(C.CASES) // 2 - 1 and not all(c["window"] for c in C.CASES)
    assert all(C.TOL[q] == 4.0 * C.PAIR_MAX[q] for q in C.QUANTITIES)


@pytest.mark.parametrize("cid", [c["id"] for c in C.CASES])
def test_inputs_are_what_the_sweep_is_meant_to_feed(cid):
    c, x = C.BY_ID[cid], C.inputs(cid)
    N, h, B = c["N"], c["h"], c["B"]
    assert C.reference(cid)["max_logit"] < 12.0
    indptr, indices, values = x["corpus"]
    assert set(np.unique(values)) <= {0.25, 0.5, 0.75, 1.0} and len(indptr) == x["n_docs"] + 1
    assert x["n_docs"] == (6 * B if c["window"] else 2 * B) and (x["pick"] is not None) == c["window"]
    for call in range(2):
        d, T = x["dh2"][call], x["T"][call]
        assert d.shape == (B, h + 1) and np.all(d[:, h] == 1.0) and d[:, :h].min() >= 0.0 and d[:, :h].max() < 1.0
        assert B * h < 200 or 0.2 < (d[:, :h] == 0).mean() < 0.4
        per_row = (T != 0).sum(1)
        assert per_row[0] == N and T[:, N - 1].any()              # one row holds every item; the ragged tile's last item is hit
        assert B < 3 or c["dense"] or (per_row == 0).any()         # empty rows
        if c["dense"]:
            assert (T[:, :32] != 0).all() and B * 32 > 1024        # tile 0's entry list: more than 1024 entries
        if c["window"]:
            assert len(set(x["pick"][call].tolist())) == B and x["pick"][call].max() < x["n_docs"]
    assert x["mom"]["v_w"].min() >= 1e-8 and x["mom"]["v_b"].min() >= 1e-8


def test_float64_restatement_is_torch_autograd_and_adam():
    """logits -> F.binary_cross_entropy(sigmoid + 1e-12, T + 1e-12).mean() * grad_scale -> backward -> torch.optim.Adam with the
    loaded state, in float64 on the CPU: the same loss, dL/d(dh2), parameters and moments as Restatement64, to rounding."""
    import torch
    import torch.nn.functional as F
    cid = "N33"
    x, ref = C.inputs(cid), C.reference(cid)
    w, b = (torch.tensor(x[k], dtype=torch.float64, requires_grad=True) for k in ("w", "b"))
    opt = torch.optim.Adam([w, b], lr=C.LR)
    for p, k in ((w, "w"), (b, "b")):
        opt.state[p] = dict(step=torch.tensor(float(C.ADAM_STEP)), exp_avg=torch.tensor(x["mom"]["m_" + k], dtype=torch.float64),
                            exp_avg_sq=torch.tensor(x["mom"]["v_" + k], dtype=torch.float64))
    for call in range(2):
        d = torch.tensor(x["dh2"][call], dtype=torch.float64, requires_grad=True)
        # (in float64 a target of 1 + 1e-12 is above 1, which torch refuses and fp32 never sees: clamped, 1e-12 of a cell's term)
        target = torch.clamp(torch.tensor(x["T"][call], dtype=torch.float64) + 1e-12, max=1.0)
        loss = F.binary_cross_entropy(torch.sigmoid(d[:, :-1] @ w.T + b) + 1e-12, target)
        opt.zero_grad()
        (loss * C.GRAD_SCALE).backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), ref["loss"][call], rtol=1e-10)
        np.testing.assert_allclose(d.grad.numpy()[:, :-1], ref["da2"][call], rtol=1e-8, atol=1e-10 * np.abs(ref["da2"][call]).max())
    for got, q in ((w.detach(), "w"), (b.detach(), "b"), (opt.state[w]["exp_avg"], "m_w"), (opt.state[w]["exp_avg_sq"], "v_w"),
                   (opt.state[b]["exp_avg"], "m_b"), (opt.state[b]["exp_avg_sq"], "v_b")):
        assert np.abs(got.numpy() - ref[q]).max() <= 1e-10 * np.abs(ref[q]).max(), q
    # SGD: the moments stay as loaded
    sgd = C.reference(cid, "sgd")
    assert np.array_equal(sgd["m_w"], x["mom"]["m_w"].astype(np.float64)) and not np.array_equal(sgd["w"], x["w"].astype(np.float64))


def _pairs():
    return [(c["id"], opt) for c in C.CASES for opt in ["adam"] + (["sgd"] if any(f.endswith("sgd") for f in c["forms"]) else [])]


@pytest.mark.parametrize("cid,optimizer", _pairs())
def test_fp32_restatement_stays_within_a_quarter_of_every_tolerance(cid, optimizer):
    d = C.distance(C.restated_fp32(cid, optimizer), C.reference(cid, optimizer), optimizer)
    _seen[(cid, optimizer)] = d
    print(f"OUTPAIR {cid} {optimizer}: " + "  ".join(f"{q} {v:.2e} ({v / C.TOL[q]:.2f} of the tolerance)" for q, v in d.items()))
    assert all(v <= C.PAIR_MAX[q] for q, v in d.items()), {q: (v, C.PAIR_MAX[q]) for q, v in d.items() if v > C.PAIR_MAX[q]}
    if optimizer == "sgd":      # (the restatement never touched the moments)
        x, emu = C.inputs(cid), C.restated_fp32(cid, optimizer)
        assert all(np.array_equal(emu[q], x["mom"][q]) for q in ("m_w", "v_w", "m_b", "v_b"))


def test_the_recorded_maxima_are_the_measured_ones():
    """(runs behind the parametrised test above; on its own it measures the list itself)"""
    for cid, optimizer in _pairs():
        if (cid, optimizer) not in _seen:
            _seen[(cid, optimizer)] = C.distance(C.restated_fp32(cid, optimizer), C.reference(cid, optimizer), optimizer)
    for q in C.QUANTITIES:
        worst = max(d[q] for d in _seen.values() if q in d)
        assert 0.9 * C.PAIR_MAX[q] <= worst <= C.PAIR_MAX[q], (q, worst, C.PAIR_MAX[q])
