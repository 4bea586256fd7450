"""Bags from a resident CSR (csrc/cond_csr.h, aae_bag_csr_*), what can be checked without a GPU: the NumPy restatement of the
ragged reductions (ragged_cases.py) against bag_cases.bag_step on the padded form of the same lists (bit for bit) and against
torch's nn.EmbeddingBag(input, offsets, per_sample_weights) (test_cond_bag_gpu.py::test_kernels_equal_torch's tolerances);
the scratch arithmetic and every refusal of the C ABI through the loaded library; DeviceBags' host-side construction."""
import ctypes as C

import numpy as np
import pytest

import bag_cases as BC
import ragged_cases as RC

f32 = np.float32


def _random_case(seed, rows, dim, vocab, pad):
    """Values OFF the grid: sums round, so the order of the additions shows in the bits."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((vocab, dim)).astype(f32)
    if pad >= 0:
        table[pad] = 0
    return table, RC.make_lists(rng, rows, vocab, pad, long_row=70), rng.standard_normal((rows, dim)).astype(f32)


@pytest.mark.parametrize("sparse", [False, True], ids=["adam", "sparse_adam"])
@pytest.mark.parametrize("reduce", list(BC.NAMES), ids=list(BC.NAMES.values()))
def test_restatement_equals_the_padded_restatement_bit_for_bit(reduce, sparse):
    """All five modes, with and without a padding row, both optimisers, three steps: encodes, table and moments equal
    bag_cases.bag_step on the lists padded to their longest, bit for bit - on rounding values and on the 1/8 grid (ties)."""
    for pad in (-1, 0, 1):
        for rows, dim, vocab in ((1, 3, 2), (3, 7, 40), (9, 5, 2), (17, 4, 40)):
            if pad >= vocab:
                continue
            for grid in (False, True):
                seed = 100 * reduce + 10 * rows + pad + 2
                if grid:
                    c = RC.make_case(seed, rows, dim, vocab, reduce, pad, long_row=70)
                    table, lists, dout = c["table"], c["lists"], c["dout"]
                else:
                    table, lists, dout = _random_case(seed, rows, dim, vocab, pad)
                idx = RC.padded(lists, pad)
                p1, m1, v1 = table.copy(), np.zeros_like(table), np.zeros_like(table)
                p2, m2, v2 = table.copy(), np.zeros_like(table), np.zeros_like(table)
                for t in (1, 2, 3):
                    got = RC.step(p1, m1, v1, lists, reduce, pad, dout, 1e-2, t, sparse)
                    want = BC.bag_step(p2, m2, v2, idx, reduce, pad, dout, 1e-2, t, sparse)
                    tag = f"{BC.NAMES[reduce]} pad {pad} rows {rows} dim {dim} vocab {vocab} grid {grid} step {t}"
                    assert np.array_equal(got, want), tag
                    assert np.array_equal(p1, p2) and np.array_equal(m1, m2) and np.array_equal(v1, v2), tag


TORCH_COMBOS = [(r, s, w) for r in (RC.SUM, RC.MEAN_COUNT, RC.MAX) for s in (False, True) for w in (False, True)
                if BC.torch_exists(r, s) and (r == RC.SUM or not w)]


@pytest.mark.parametrize("reduce,sparse,weighted", TORCH_COMBOS,
                         ids=[f"{BC.NAMES[r]}-{'sparse_adam' if s else 'adam'}-{'weights' if w else 'plain'}" for r, s, w in TORCH_COMBOS])
def test_restatement_equals_torch_embedding_bag_with_offsets(reduce, sparse, weighted):
    """nn.EmbeddingBag(input, offsets, per_sample_weights) under torch.optim.Adam / SparseAdam, three steps on the CPU.  Step 0
    runs on the 1/8 grid (tie-free across rows, exact sums): encodes of sum and max bit for bit, mean within 2 ulp.  From step
    1 on the tables hold what Adam made of them and sums round: two summations of the L terms x_i of a bag (torch fuses the
    weight's product into the addition, and may reorder) differ by at most L * 2^-23 * sum |x_i|, the standard bound for
    recursive summation taken twice - that is the tolerance of those steps, per element.  exp_avg at 2e-8 / 2e-4,
    exp_avg_sq at 1e-12 / 2e-4, the table at 1e-5.  (torch takes per_sample_weights with mode='sum' only, and its mode='max'
    has no sparse gradient: those combinations have no definition to be held to.)"""
    lr = 1e-2
    for pad in (-1, 0):
        for rows, dim, vocab in ((3, 7, 40), (9, 5, 2), (17, 4, 40)):
            rng = np.random.default_rng(5 + reduce + rows)
            cases = [RC.make_case(31 * reduce + 7 * rows + s + pad + 1, rows, dim, vocab, reduce, pad, long_row=70, outside=False)
                     for s in range(3)]
            lists_steps, dout_steps = [c["lists"] for c in cases], [c["dout"] for c in cases]
            wts = [RC.make_weights(rng, lists) for lists in lists_steps] if weighted else None
            table = cases[0]["table"]
            want_outs, want_p, want_m, want_v = RC.torch_steps(table, lists_steps, reduce, pad, dout_steps, lr, sparse, wts)
            p, m, v = table.copy(), np.zeros_like(table), np.zeros_like(table)
            for t in range(3):
                absw = None if wts is None else [[abs(x) for x in row] for row in wts[t]]
                longest = max(len(row) for row in lists_steps[t])
                bound = longest * 2.0 ** -23 * RC.encode(np.abs(p), lists_steps[t], RC.SUM, pad, absw)[0].astype(np.float64)
                out = RC.step(p, m, v, lists_steps[t], reduce, pad, dout_steps[t], lr, t + 1, sparse,
                              None if wts is None else wts[t])
                tag = f"{BC.NAMES[reduce]} pad {pad} rows {rows} dim {dim} vocab {vocab} step {t}"
                if t == 0 and reduce in (RC.SUM, RC.MAX):
                    assert np.array_equal(out, want_outs[t]), tag
                elif t == 0:
                    ulp = np.spacing(np.abs(want_outs[t]).astype(f32))
                    assert (np.abs(out - want_outs[t]) <= 2 * ulp).all(), tag
                else:
                    assert (np.abs(out - want_outs[t]) <= bound).all(), tag
            np.testing.assert_allclose(m, want_m, atol=2e-8, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(v, want_v, atol=1e-12, rtol=2e-4, err_msg=tag)
            np.testing.assert_allclose(p, want_p, atol=1e-5, rtol=0, err_msg=tag)
            if pad >= 0:
                assert np.array_equal(p[pad], table[pad]), tag + ": the padding row moved"


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------
def test_scratch_bytes_is_monotone_and_refuses_negative_sizes():
    from aaerec import _hip
    lib = _hip.load_library()
    sizes = (0, 1, 2, 63, 64, 65, 1000, 4096, 4097, 1 << 20, 1 << 22)
    grid = np.array([[_hip.bag_csr_scratch_bytes(r, e) for e in sizes] for r in sizes])
    assert (grid > 0).all() and (grid % 256 == 0).all()
    assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()            # (sizes round up to 256 bytes)
    assert (np.diff(grid[:, ::3], axis=1) > 0).all() and (np.diff(grid[::3], axis=0) > 0).all()
    assert grid[6, 7] >= 16 * 4096 + 4 * (1000 * 256 + 4096)        # two key buffers, the winners, the entries' rows
    n = C.c_int64(-7)
    for r, e in ((-1, 10), (10, -1), (-5, -5)):
        assert lib.aae_bag_csr_scratch_bytes(r, e, C.byref(n)) == -1 and n.value == -7          # AAE_EINVAL, nothing written
        assert "max_rows and max_entries must be >= 0" in lib.aae_last_error().decode()
        with pytest.raises(_hip.AaeHipError, match="must be >= 0"):
            _hip.bag_csr_scratch_bytes(r, e)
    assert lib.aae_bag_csr_scratch_bytes(1, 1, None) == -1 and "bytes_out is NULL" in lib.aae_last_error().decode()


def _scratch_bytes(rows, entries):
    from aaerec import _hip
    return _hip.bag_csr_scratch_bytes(rows, entries)


def _call(lib, which, **over):
    """aae_bag_csr_encode / _update with plausible arguments (non-NULL made-up addresses: every refusal sits in front of the
    first HIP call, so nothing is dereferenced) and the ones of `over`."""
    P = lambda: C.c_void_p(4096)                                                  # noqa: E731
    a = dict(table=P(), m=P(), v=P(), g=P(), vocab=40, dim=8, indptr=P(), indices=P(), weights=None, n_docs=100, nnz=500,
             row_ids=P(), row0=0, rows=4, max_entries=64, reduce=BC.SUM, pad=-1, block=P(), ld=8, optimizer=0, lr=1e-3, step=1,
             scratch=P(), scratch_bytes=None)
    a.update(over)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = _scratch_bytes(max(a["rows"], 0), min(max(a["max_entries"], 0), 1 << 22))
    if which == "encode":
        rc = lib.aae_bag_csr_encode(a["table"], a["vocab"], a["dim"], a["indptr"], a["indices"], a["weights"], a["n_docs"], a["nnz"],
                                    a["row_ids"], a["row0"], a["rows"], a["reduce"], a["pad"], a["block"], a["ld"], a["scratch"],
                                    a["scratch_bytes"], None)
    else:
        rc = lib.aae_bag_csr_update(a["table"], a["m"], a["v"], a["g"], a["vocab"], a["dim"], a["indptr"], a["indices"],
                                    a["weights"], a["n_docs"], a["nnz"], a["row_ids"], a["row0"], a["rows"], a["max_entries"],
                                    a["reduce"], a["pad"], a["block"], a["ld"], a["optimizer"], a["lr"], a["step"], a["scratch"],
                                    a["scratch_bytes"], None)
    return rc, lib.aae_last_error().decode()


REFUSALS = [
    (dict(dim=0), "dim must be within [1, 256]"),
    (dict(dim=257, ld=300), "dim must be within [1, 256]"),
    (dict(rows=0), "rows must be >= 1"),
    (dict(rows=-2), "rows must be >= 1"),
    (dict(weights=C.c_void_p(4096), reduce=BC.MEAN_COUNT), "weights_dev goes with reduce AAE_BAG_SUM only"),
    (dict(weights=C.c_void_p(4096), reduce=BC.MAX), "weights_dev goes with reduce AAE_BAG_SUM only"),
    (dict(scratch_bytes=64), "scratch_bytes is smaller than aae_bag_csr_scratch_bytes"),
    (dict(scratch=None), "scratch_dev is NULL"),
    (dict(row_ids=None, row0=98), "row0 .. row0 + rows"),
    (dict(pad=40), "padding_idx"),
    (dict(reduce=5), "unknown reduce"),
]


@pytest.mark.parametrize("which", ["encode", "update"])
def test_every_refusal_is_reached_in_front_of_the_first_hip_call(which):
    from aaerec import _hip
    lib = _hip.load_library()
    EINVAL = -1                                 # include/aaerec_hip.h: AAE_EINVAL
    for over, text in REFUSALS:
        rc, msg = _call(lib, which, **over)
        assert rc != 0 and text in msg and msg.startswith("aae_bag_csr_" + which), (over, rc, msg)
        assert rc == EINVAL, (over, rc)
    if which == "update":
        for over, text in ((dict(max_entries=(1 << 22) + 1), "a step takes at most 2^22 entries"),
                           (dict(max_entries=0), "max_entries must be >= 1"),
                           (dict(step=0), "step counts from 1"),
                           (dict(optimizer=1, g=None), "grad_scratch_dev"),
                           (dict(reduce=BC.MAX, g=None), "grad_scratch_dev")):
            rc, msg = _call(lib, which, **over)
            assert rc == EINVAL and text in msg, (over, rc, msg)
        # the scratch is one byte short of what the bound asks for
        need = _scratch_bytes(4, 5000)
        rc, msg = _call(lib, which, max_entries=5000, scratch_bytes=need - 1)
        assert rc == EINVAL and "scratch_bytes" in msg


# ---- DeviceBags on the host ------------------------------------------------------------------------------------------------------
def test_device_bags_from_lists_and_from_offsets_agree():
    from aaerec import _hip
    rng = np.random.default_rng(3)
    lists = RC.make_lists(rng, 11, 40, -1, long_row=9)
    weights = RC.make_weights(rng, lists)
    idx, offsets, wts = RC.flat(lists, weights)
    a = _hip.DeviceBags(lists, "cpu", weights=wts)
    b = _hip.DeviceBags.from_offsets(idx, offsets, "cpu", weights=wts)
    c = _hip.DeviceBags.from_offsets(idx, np.concatenate([offsets, [len(idx)]]), "cpu", weights=wts, include_last_offset=True)
    for x in (b, c):
        assert x.n_docs == a.n_docs == 11 and x.nnz == a.nnz == len(idx)
        assert np.array_equal(x.indptr.numpy(), a.indptr.numpy()) and x.indptr.dtype.is_floating_point is False
        assert np.array_equal(x.indices.numpy(), a.indices.numpy())
        assert np.array_equal(x.weights.numpy(), a.weights.numpy())
        assert np.array_equal(x.lengths.numpy(), np.array([len(r) for r in lists], dtype=np.int32))
    # order and repeats are kept; a value beyond int32 names no row
    assert a.indices.numpy()[:9].tolist() == lists[0]
    assert _hip.bags_from_lists([[3, 2 ** 40, 3]])[1].tolist() == [3, -1, 3]
    # the entry bound of k rows: the k longest lists
    lens = sorted((len(r) for r in lists), reverse=True)
    assert [a.entry_bound(k) for k in (1, 2, 11, 50)] == [max(1, sum(lens[:k])) for k in (1, 2, 11, 11)]
    assert _hip.DeviceBags([[], []], "cpu").entry_bound(2) == 1
    # without include_last_offset the last bag runs to the end; with it the offsets must already say so
    assert _hip.bags_from_offsets([1, 2, 3], [0, 1])[0].tolist() == [0, 1, 3]
    assert _hip.bags_from_offsets([1, 2, 3], [0, 1, 3], include_last_offset=True)[0].tolist() == [0, 1, 3]
    with pytest.raises(ValueError):
        _hip.bags_from_offsets([1, 2, 3], [1, 2])
    with pytest.raises(ValueError):
        _hip.bags_from_offsets([1, 2, 3], [0, 1], weights=[1.0])
