"""GPU parity of the long-list ranking path (csrc/rank_long.h, abi_rank.h): aae_predict_topk / aae_decode_topk with
32 < k <= 1024 - the reference's MPD driver ranks 500 items per row with the same predict -> remove_non_missing -> argtopk
(aae.py:840-870, evaluation.py:183-199, 20-58).  Checked as tests/test_rank_gpu.py checks the short lists: against the
reference's host pipeline run on predict()'s dense matrix, and against the oracle's predict directly.  Tolerances are that
file's: 2e-6 on scaled scores for fp32 handles, 2e-3 for bf16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _host_topk(full, known_rows, k, exclude_known):
    """remove_non_missing + argtopk of the reference on a dense score matrix: min-max scale every row over ALL its scores,
    drop the row's input items, the k best (ties: smaller item id first)."""
    n = full.shape[0]
    ids = np.zeros((n, k), dtype=np.int64)
    vals = np.zeros((n, k), dtype=np.float32)
    for b in range(n):
        row = full[b].astype(np.float32)
        lo, hi = row.min(), row.max()
        sc = (row - lo) * (np.float32(1.0) / (hi - lo) if hi > lo else np.float32(1.0))
        rk = row.copy()
        if exclude_known:
            rk[known_rows[b]] = -np.inf
        order = np.lexsort((np.arange(rk.size), -rk))[:k]
        ids[b], vals[b] = order, sc[order]
    return ids, vals


def _corpus(r, N, n_docs, max_len):
    rows = [np.sort(r.choice(N, size=int(r.integers(1, max_len)), replace=False)) for _ in range(n_docs)]
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), np.ones(int(ip[-1]), dtype=np.float32), rows


def _dense(dev, csr, rows, R, cdev=None):
    return np.concatenate([dev.predict(csr, s, min(R, rows - s), cond=None if cdev is None else cdev[s:s + R]).cpu().numpy()
                           for s in range(0, rows, R)])


def _assert_lists(ids, vals, full, docs, k, excl, tol, tag=""):
    """ids / vals [rows][k] against the host pipeline over `full`: scores within tol, ids different only where the two
    items' scaled scores differ by at most tol, k distinct ids per row, none of them a known item."""
    want_ids, want_vals = _host_topk(full, docs, k, excl)
    print(tag, "max |scaled score - host pipeline| =", float(np.abs(vals - want_vals).max()), "tolerance", tol)
    np.testing.assert_allclose(vals, want_vals, atol=tol, err_msg=str(tag))
    b, j = np.nonzero(ids != want_ids)
    lo, hi = full.min(1), full.max(1)
    scaled = (full - lo[:, None]) / np.where(hi > lo, hi - lo, 1.0)[:, None]
    assert np.all(np.abs(scaled[b, ids[b, j]] - scaled[b, want_ids[b, j]]) <= tol), (tag, len(b))
    for row in range(ids.shape[0]):
        assert len(set(ids[row].tolist())) == k, (tag, row)
        if excl:
            assert not (set(ids[row].tolist()) & set(docs[row].tolist())), (tag, row)


def _model(case, N, h, c, inc, R, rows, dtype="f32", activation="ReLU", scale=8.0, steps=3, max_len=30):
    """A handle as tests/test_rank_gpu.py::_rank_case builds it: dec.lin3 scaled so the scores spread, a few training
    steps first (enc.lin1 rows with deferred Adam steps pending, a deferred optimiser launch in flight)."""
    from aaerec._hip import HipAAE, DeviceCSR
    from tools.synth import init_params
    r = np.random.default_rng(100 + case)
    kw = dict(dropout=(0.2, 0.2), gen_lr=1e-3, reg_lr=1e-3, activation=activation, **({"dtype": "bf16"} if dtype == "bf16" else {}))
    dev = HipAAE(N, h, c, cond_inc=inc, max_batch=R, rng_mode="device", seed=3, **kw)
    params = init_params(N, h, c, cond_inc=inc, seed=case)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * scale
    dev.load_params(params)
    ip, idx, val, docs = _corpus(r, N, rows, max_len)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
    cond = (r.standard_normal((rows, inc)) * 0.4).astype(np.float32) if inc else None
    cdev = torch.as_tensor(cond, device=dev.device) if inc else None
    n = min(R, max(1, rows // 3))
    for s in range(steps):
        dev.step(csr, s * n, n, cond=None if cdev is None else cdev[s * n:(s + 1) * n])
    return dev, csr, docs, cdev


def _long_case(case, N, h, c, inc, R, rows, k, excl, dtype, fused=True, activation="ReLU"):
    dev, csr, docs, cdev = _model(case, N, h, c, inc, R, rows, dtype, activation)
    cap = dev.rank_max_rows(k)
    assert cap >= R, (cap, R)
    rows = min(rows, cap)
    docs = docs[:rows]
    cdev = None if cdev is None else cdev[:rows].contiguous()
    dev.rank_long_stats()
    ids, vals = dev.predict_topk(csr, 0, rows, k, cond=cdev, exclude_known=excl)
    st = dev.rank_long_stats()
    print(f"case {case}: N={N} rows={rows} k={k} rank_max_rows={cap} fused calls={st['calls']} overflow rows={st['overflow_rows']} "
          f"entries per row: mean {st['entries'] / max(1, st['rows']):.1f} max {st['max_entries']} (k={k}, cap 4096)")
    if fused:
        assert st["calls"] == 1 and st["rows"] == rows, st           # the fused form ranked this call ...
        assert st["overflow_rows"] == 0, st                          # ... and the floor kept every list within its capacity
    else:
        assert st["calls"] == 0 and cap == R, (st, cap)
    ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    full = _dense(dev, csr, rows, R, cdev)
    tol = 2e-6 if dtype == "f32" else 2e-3
    _assert_lists(ids, vals, full, docs, k, excl, tol, f"case {case} predict_topk")
    # the same through aae_decode_topk (a caller-built decoder input)
    z = torch.cat([dev.encode(csr, s, min(R, rows - s)) for s in range(0, rows, R)])
    zc = z if cdev is None else torch.cat([z, cdev], 1)
    ids2, vals2 = dev.decode_topk(zc, csr, 0, k, exclude_known=excl)
    _assert_lists(ids2.cpu().numpy(), vals2.cpu().numpy(), full, docs, k, excl, tol, f"case {case} decode_topk")
    # determinism: the same call again, bit for bit
    ids3, vals3 = dev.predict_topk(csr, 0, rows, k, cond=cdev, exclude_known=excl)
    assert np.array_equal(ids3.cpu().numpy(), ids)
    assert np.array_equal(vals3.cpu().numpy().view(np.uint32), vals.view(np.uint32))
    return dev


def test_predict_topk_of_500_items_equals_the_host_pipeline():
    """The lists the reference's MPD driver asks for (argtopk(predictions, 500)): k = 500 on a small fp32 handle equals the
    host pipeline over predict()'s matrix.  (k beyond 32 was refused with AAE_EINVAL before the long-list path.)"""
    dev, csr, docs, _ = _model(1, 3001, 100, 30, 0, 50, 50, steps=0)
    ids, vals = dev.predict_topk(csr, 0, 50, 500)
    assert ids.shape == (50, 500) and vals.shape == (50, 500)
    full = _dense(dev, csr, 50, 50)
    _assert_lists(ids.cpu().numpy(), vals.cpu().numpy(), full, docs, 500, True, 2e-6, "k=500")


FUSED_CASES = [  # N, h, c, inc, max_batch, rows, k, exclude_known, dtype
    (5000, 200, 50, 0, 512, 64, 33, True, "f32"),
    (5000, 200, 50, 0, 512, 64, 100, True, "f32"),
    (5000, 200, 50, 0, 512, 64, 500, True, "f32"),
    (5000, 200, 50, 0, 512, 64, 1024, True, "f32"),
    (4587, 200, 50, 300, 512, 60, 100, True, "f32"),        # C4's shape: a 300-wide condition
    (47000, 100, 50, 0, 100, 300, 500, True, "bf16"),       # C2's shape in bf16 mode
    (100000, 200, 50, 0, 100, 512, 500, True, "f32"),       # C3 x 512 rows
    (2900000, 200, 50, 0, 32, 40, 500, True, "f32"),        # dec.lin3 beyond 2^31 bytes: the window instantiations
    (2000, 61, 20, 7, 512, 100, 100, False, "f32"),         # nothing excluded
]


@pytest.mark.parametrize("case", range(len(FUSED_CASES)))
def test_fused_long_lists_equal_host_pipeline(case):
    N, h, c, inc, R, rows, k, excl, dtype = FUSED_CASES[case]
    dev = _long_case(case, N, h, c, inc, R, rows, k, excl, dtype)
    if N == 100000:
        assert dev.rank_max_rows(500) >= 512       # (the workspace arithmetic of DESIGN.md's long-list section)
        print("C3 handle: rank_max_rows(500) =", dev.rank_max_rows(500), "rank_max_rows(1024) =", dev.rank_max_rows(1024))


@pytest.mark.parametrize("k", [100, 500])
def test_dense_long_lists_of_a_model_without_the_fused_launch(k):
    """A GELU model has no fused ranking launch: max_batch rows per call through the score matrix and the long-list kernel
    on it (radix select + LDS sort) - same contract, same checks."""
    _long_case(40 + k, 3001, 100, 30, 0, 50, 113, k, True, "f32", fused=False, activation="GELU")


def test_first_32_of_a_long_list_are_the_short_list():
    """The new path agrees with the untouched one: the first 32 scores of a k = 100 call are the k = 32 call's scores."""
    dev, csr, docs, _ = _model(7, 5000, 200, 50, 0, 512, 64)
    i32, v32 = (t.cpu().numpy() for t in dev.predict_topk(csr, 0, 64, 32))
    i100, v100 = (t.cpu().numpy() for t in dev.predict_topk(csr, 0, 64, 100))
    assert dev.rank_long_stats()["calls"] == 1
    np.testing.assert_allclose(v100[:, :32], v32, atol=2e-6)
    d = i100[:, :32] != i32
    assert np.all(np.abs(v100[:, :32][d] - v32[d]) <= 2e-6)


def test_long_lists_match_oracle_predict_and_chunked_calls_agree():
    from aaerec._hip import HipAAE, DeviceCSR
    from oracle import aae_oracle as O
    from oracle.dense_torch_port import init_params
    N, h, c, R, rows, k = 6000, 64, 24, 512, 90, 500
    r = np.random.default_rng(5)
    params = init_params(N, h, c, seed=2)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * 6.0
    kw = dict(dropout=(0.0, 0.0), gen_lr=1e-3, reg_lr=1e-3)
    dev = HipAAE(N, h, c, max_batch=R, rng_mode="inject", **kw)
    dev.load_params(params)
    ora = O.OracleAAE(params, **kw)
    ip, idx, val, docs = _corpus(r, N, rows, 12)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
    want = ora.predict(ip, idx, val)
    ids, vals = (t.cpu().numpy() for t in dev.predict_topk(csr, 0, rows, k))
    assert dev.rank_long_stats()["calls"] == 1
    _assert_lists(ids, vals, want, docs, k, True, 1e-5, "oracle")      # (test_rank_gpu.py's bound against the oracle)
    parts = [dev.predict_topk(csr, s, 30, k) for s in range(0, rows, 30)]
    assert np.array_equal(torch.cat([p[0] for p in parts]).cpu().numpy(), ids)
    np.testing.assert_array_equal(torch.cat([p[1] for p in parts]).cpu().numpy(), vals)


def test_saturated_scores_give_a_valid_long_list():
    """dec.lin3 scaled until hundreds of sigmoids per row are 1.0f: the k scaled scores equal the host pipeline's, every
    named item holds the score of its rank, no known item is named (fused form: ordered by logit; ids may differ at ties)."""
    from aaerec._hip import HipAAE, DeviceCSR
    from tools.synth import init_params
    N, h, c, R, rows, k = 6000, 200, 50, 512, 64, 500
    r = np.random.default_rng(77)
    dev = HipAAE(N, h, c, max_batch=R, rng_mode="device", seed=5, dropout=(0.0, 0.0))
    params = init_params(N, h, c, seed=9)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * 600.0
    params["dec.lin2.weight"] = params["dec.lin2.weight"] * 4.0
    dev.load_params(params)
    ip, idx, val, docs = _corpus(r, N, rows, 30)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
    ids, vals = (t.cpu().numpy() for t in dev.predict_topk(csr, 0, rows, k))
    assert dev.rank_long_stats()["calls"] == 1
    full = _dense(dev, csr, rows, R)
    assert np.median((full == 1.0).sum(1)) >= 10
    want_ids, want_vals = _host_topk(full, docs, k, True)
    np.testing.assert_allclose(vals, want_vals, atol=2e-6)
    lo, hi = full.min(1), full.max(1)
    scaled = (full - lo[:, None]) / np.where(hi > lo, hi - lo, 1.0)[:, None]
    np.testing.assert_allclose(np.take_along_axis(scaled, ids.astype(np.int64), axis=1), want_vals, atol=2e-6)
    for row in range(rows):
        assert len(set(ids[row].tolist())) == k and not (set(ids[row].tolist()) & set(docs[row].tolist()))


@pytest.mark.parametrize("inc", [0, 7])
def test_overflowing_collect_lists_take_the_exact_fallback(inc):
    """RANK_COLLECT_CAP set to a handful of entries: every row's list overflows and is ranked through the score matrix -
    the same scores, a valid list; unset, no row of the same call overflows.  With a condition (inc = 7) the spans that start
    at rows 64 and 128 read their own condition rows: a wrong offset would show."""
    from aaerec import _hip
    k, rows, R = 100, 150, 64
    _hip.set_option("RANK_COLLECT_CAP", 8)
    try:
        small, csr, docs, cdev = _model(3, 20000, 100, 30, inc, R, rows, steps=0)     # (no training: both handles hold the same weights)
    finally:
        _hip.set_option("RANK_COLLECT_CAP", None)
    dev, csr2, docs2, cdev2 = _model(3, 20000, 100, 30, inc, R, rows, steps=0)
    assert min(small.rank_max_rows(k), dev.rank_max_rows(k)) >= rows
    ids, vals = (t.cpu().numpy() for t in dev.predict_topk(csr2, 0, rows, k, cond=cdev2))
    st = dev.rank_long_stats()
    assert st["calls"] == 1 and st["overflow_rows"] == 0, st
    ids_s, vals_s = (t.cpu().numpy() for t in small.predict_topk(csr, 0, rows, k, cond=cdev))
    st = small.rank_long_stats()
    assert st["calls"] == 1 and st["overflow_rows"] == rows, st
    full = _dense(small, csr, rows, R, cdev)
    _assert_lists(ids_s, vals_s, full, docs, k, True, 2e-6, "overflow")
    np.testing.assert_allclose(vals_s, vals, atol=2e-6)
    z = torch.cat([small.encode(csr, s, min(R, rows - s)) for s in range(0, rows, R)])
    zc = z if cdev is None else torch.cat([z, cdev], 1)
    ids_d, vals_d = (t.cpu().numpy() for t in small.decode_topk(zc, csr, 0, k))
    _assert_lists(ids_d, vals_d, full, docs, k, True, 2e-6, "overflow decode_topk")


@pytest.mark.parametrize("N,h,c,R,rows,k,act", [(64, 8, 3, 16, 12, 50, "ReLU"), (300, 200, 50, 8, 20, 290, "ReLU"),
                                                 (1100, 32, 8, 16, 40, 1024, "ReLU"), (64, 8, 3, 16, 12, 50, "GELU")])
def test_short_rows_end_in_minus_one(N, h, c, R, rows, k, act):
    """Rows whose known items leave fewer than k to rank: their items, then id -1 / score 0.0 - the rule of the k <= 32 paths
    (tests/test_rank_gpu.py::test_fused_rank_degenerate_shapes), in the fused and in the dense form."""
    from aaerec._hip import HipAAE, DeviceCSR
    from tools.synth import init_params
    r = np.random.default_rng(N + rows)
    dev = HipAAE(N, h, c, max_batch=R, rng_mode="device", seed=1, activation=act)
    params = init_params(N, h, c, seed=3)
    params["dec.lin3.weight"] = params["dec.lin3.weight"] * 6.0
    dev.load_params(params)
    rows = min(rows, dev.rank_max_rows(k))
    ip, idx, val, docs = _corpus(r, N, rows, N - 2 if N <= 64 else 2 * (N - k))     # (rows that name more than N - k items among them)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
    ids, vals = (t.cpu().numpy() for t in dev.predict_topk(csr, 0, rows, k))
    full = _dense(dev, csr, rows, R)
    short = 0
    for b in range(rows):
        row = full[b]
        lo, hi = row.min(), row.max()
        sc = (row - lo) / (hi - lo) if hi > lo else np.zeros_like(row)
        free = np.setdiff1d(np.arange(N), docs[b])
        n_ok = min(k, len(free))
        short += n_ok < k
        assert np.all(ids[b, n_ok:] == -1) and np.all(vals[b, n_ok:] == 0.0), (b, ids[b], len(free))
        got = ids[b, :n_ok]
        assert len(set(got.tolist())) == n_ok and not (set(got.tolist()) & set(docs[b].tolist()))
        np.testing.assert_allclose(vals[b, :n_ok], sc[got], atol=2e-6)
        assert np.all(np.diff(vals[b, :n_ok]) <= 1e-6)
        kth = np.sort(sc[free])[-n_ok]
        assert np.all(sc[got] >= kth - 2e-6)
    assert short > 0, "the case is meant to have rows with fewer than k rankable items"


def test_model_level_predict_topk_and_the_custom_op_take_long_lists():
    """AdversarialAutoEncoder.predict_topk (chunks of rank_max_rows(k) rows) and torch.ops.aaerec.predict_topk at k = 100."""
    import scipy.sparse as sp
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec import ops
    from aaerec._hip import DeviceCSR
    r = np.random.default_rng(11)
    N, n = 3000, 230
    X = sp.random(n, N, density=0.004, format="csr", random_state=3, dtype=np.float32)
    X.data[:] = 1.0
    X = X[np.diff(X.indptr) > 0]
    n = X.shape[0]
    m = AdversarialAutoEncoder(n_hidden=100, n_code=30, batch_size=50, n_epochs=1, verbose=False, seed=1)
    m.fit(X)
    ids, vals = m.predict_topk(X, k=100)
    assert ids.shape == (n, 100)
    full = m.predict(X)
    full = full.toarray() if sp.issparse(full) else np.asarray(full)
    docs = [X.indices[X.indptr[b]:X.indptr[b + 1]] for b in range(n)]
    _assert_lists(ids, vals, full.astype(np.float32), docs, 100, True, 2e-6, "model")
    csr = DeviceCSR(X, m.hip.device)
    mid = ops.register_model(m.hip)
    oi, ov = torch.ops.aaerec.predict_topk(mid, csr.indptr, csr.indices, csr.values, 0, 40, int(csr.nnz_per_row_max), None, 100, True)
    np.testing.assert_allclose(ov.cpu().numpy(), vals[:40], atol=2e-6)
