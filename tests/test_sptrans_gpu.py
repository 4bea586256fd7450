"""The device CSR transpose (csrc/sptrans.h; _hip.csr_transpose / _hip.cooc_transpose) bit for bit against scipy's
A.T.tocsr() + sort_indices(), and aae_spmm_f32 (_hip.spmm_f32) against the float64 product within csrc/lowrank.h's bound."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS = 4096          # _hip.SPTRANS_LDS: the longest segment sorted in LDS in one go


def _hip():
    from aaerec import _hip
    return _hip


def _canon(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def _want(A):
    T = A.T.tocsr()
    T.sort_indices()
    return T


def _got(t, bits=np.uint32):
    nnz = int(t.indptr[-1])
    return t.indptr.cpu().numpy(), t.indices[:nnz].cpu().numpy(), t.values[:nnz].cpu().numpy().view(bits)


def _check(A, values="f32"):
    """Transpose canonical A (float32 or int32 values) on the device: the bits of scipy's transpose.  Returns the device result."""
    hip = _hip()
    if values == "f32":
        A = A.astype(np.float32)
        t = hip.csr_transpose(hip.DeviceCSR.from_arrays(A.indptr, A.indices, A.data, A.shape[1], DEV))
    else:
        A = A.astype(np.int32)
        t = hip.cooc_transpose(hip.DeviceCooc(A, DEV))
    W = _want(A)
    ip, idx, val = _got(t)
    assert tuple(t.shape) == W.shape
    assert ip.dtype == np.int64 and np.array_equal(ip, W.indptr.astype(np.int64))
    assert np.array_equal(idx, W.indices.astype(np.int32))
    assert np.array_equal(val, W.data.view(np.uint32))
    return t


def _one_column(rows, n_cols=3, col=1):
    """Every row holds column `col`: T's row `col` is a segment of `rows` entries; values distinct so a misplaced pair shows."""
    return sp.csr_matrix((np.arange(1, rows + 1, dtype=np.float64), np.full(rows, col), np.arange(rows + 1)), shape=(rows, n_cols))


def _random(rows, cols, density, seed):
    r = np.random.default_rng(seed)
    A = sp.random(rows, cols, density=density, random_state=np.random.RandomState(seed), format="csr")
    A.data[:] = r.integers(1, 1000, size=A.nnz)
    return _canon(A)


@pytest.mark.parametrize("values", ["f32", "i32"])
def test_empty_shapes(values):
    _check(sp.csr_matrix((0, 7)), values)                   # no rows
    _check(sp.csr_matrix((5, 9)), values)                   # rows, no entries
    A = _random(40, 50, 0.05, 1).tolil()
    A[[0, 7, 39], :] = 0
    A[:, [0, 13, 49]] = 0
    _check(_canon(A.tocsr()), values)                       # empty rows and empty columns mixed in


@pytest.mark.parametrize("rows", [1, LDS, LDS + 1, 10007, 3 * LDS + 5])
@pytest.mark.parametrize("values", ["f32", "i32"])
def test_one_column_holds_every_row(rows, values):
    _check(_one_column(rows), values)


def test_single_column_matrix():
    _check(_one_column(300, n_cols=1, col=0))
    _check(_one_column(LDS + 9, n_cols=1, col=0), "i32")


def test_mixed_segments_over_several_workgroups():
    """Short, LDS-sized and merged segments side by side; Zipf-like columns as the workload's."""
    r = np.random.default_rng(3)
    rows, cols = 30011, 37
    p = 1.0 / (1.0 + np.arange(cols))
    ids = [np.sort(r.choice(cols, size=int(r.integers(0, 6)), replace=False, p=p / p.sum())) for _ in range(rows)]
    ip = np.concatenate([[0], np.cumsum([i.size for i in ids])])
    idx = np.concatenate(ids)
    A = sp.csr_matrix((r.integers(1, 1 << 20, size=idx.size).astype(np.float64), idx, ip), shape=(rows, cols))
    assert np.diff(_want(A).indptr).max() > 2 * LDS
    _check(A)
    _check(A, "i32")


def test_float_bits_are_moved_not_rounded():
    """-0.0 and a NaN payload keep their bits."""
    A = _random(60, 45, 0.1, 5).astype(np.float32)
    bits = A.data.view(np.uint32)
    bits[0], bits[1], bits[2] = 0x80000000, 0x7FC12345, 0xFFC00001
    hip = _hip()
    t = hip.csr_transpose(hip.DeviceCSR.from_arrays(A.indptr, A.indices, A.data, A.shape[1], DEV))
    W = _want(A)
    ip, idx, val = _got(t)
    assert np.array_equal(ip, W.indptr) and np.array_equal(idx, W.indices) and np.array_equal(val, W.data.view(np.uint32))
    assert {0x80000000, 0x7FC12345, 0xFFC00001} <= set(val.tolist())


def test_column_id_out_of_range_is_skipped():
    hip = _hip()
    A = _random(50, 20, 0.2, 7).astype(np.float32)
    idx = A.indices.copy()
    drop = np.zeros(A.nnz, dtype=bool)
    drop[[3, 10]] = True
    idx[3], idx[10] = 20, -1                                # one past the last column, and a negative id
    t = hip.csr_transpose(hip.DeviceCSR.from_arrays(A.indptr, idx, A.data, A.shape[1], DEV))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    K = sp.csr_matrix((A.data[~drop], (rows[~drop], A.indices[~drop])), shape=A.shape)
    W = _want(_canon(K))
    ip, idx_t, val = _got(t)
    assert np.array_equal(ip, W.indptr) and np.array_equal(idx_t, W.indices) and np.array_equal(val, W.data.view(np.uint32))


def test_same_bits_twice_and_round_trip():
    hip = _hip()
    A = sp.vstack([_random(9000, 30, 0.3, 9), _one_column(5000, n_cols=30, col=4)]).tocsr().astype(np.float32)
    A = _canon(A)
    d = hip.DeviceCSR.from_arrays(A.indptr, A.indices, A.data, A.shape[1], DEV)
    a, b = _got(hip.csr_transpose(d)), _got(hip.csr_transpose(d))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    back = hip.csr_transpose(hip.csr_transpose(d))
    ip, idx, val = _got(back)
    assert tuple(back.shape) == A.shape
    assert np.array_equal(ip, A.indptr) and np.array_equal(idx, A.indices) and np.array_equal(val, A.data.view(np.uint32))


def test_a_result_beyond_the_lds_limit_needs_its_scratch():
    """The raw call refuses, before anything is launched, a result of more than 4096 entries without a scratch of nnz pairs."""
    import torch
    hip = _hip()
    lib = hip.load_library()
    n = LDS + 1
    ip = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    idx = torch.zeros(n, dtype=torch.int32, device=DEV)
    val = torch.zeros(n, dtype=torch.float32, device=DEV)
    tip = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    cur = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.aae_csr_transpose_fill(p(ip), p(idx), p(val), n, 1, p(tip), p(idx.clone()), p(val.clone()), p(cur), None, 0, n, None)
    assert rc == -1 and b"scratch" in lib.aae_last_error()


# ---- aae_spmm_f32 ----------------------------------------------------------------------------------------------------
def _spmm_case(width, seed=21, rows=37, cols=700):
    """Feature rows with float values: row 1 empty, row 2 holding 613 entries (more than the 256 staged in LDS at a time)."""
    r = np.random.default_rng(seed)
    ids = [np.sort(r.choice(cols, size=int(r.integers(1, 30)), replace=False)) for _ in range(rows)]
    ids[1] = np.zeros(0, dtype=np.int64)
    ids[2] = np.sort(r.choice(cols, size=613, replace=False))
    ip = np.concatenate([[0], np.cumsum([i.size for i in ids])])
    idx = np.concatenate(ids)
    x = r.random(idx.size).astype(np.float32) + 0.25
    D = r.standard_normal((cols, width)).astype(np.float32)
    return sp.csr_matrix((x, idx, ip), shape=(rows, cols)), D


@pytest.mark.parametrize("width", [1, 4, 26, 4096])
def test_spmm_f32_within_the_fp32_chain_bound(width):
    """|out - exact| <= 2^-23 (nnz_r + 8) sum_e |x_e| |D_e,j|: csrc/lowrank.h's projection chain (Higham (3.5), gamma_n at
    twice the unit roundoff), the operands being fp32 already."""
    import torch
    hip = _hip()
    A, D = _spmm_case(width)
    ld = (width + 3) & ~3
    dense = torch.full((A.shape[1], ld), float("nan"), dtype=torch.float32, device=DEV)      # (padding: read, never stored)
    dense[:, :width] = torch.from_numpy(D).to(DEV)
    csr = hip.DeviceCSR.from_arrays(A.indptr, A.indices, A.data, A.shape[1], DEV)
    out = torch.full((A.shape[0], ld + 4), -7.0, dtype=torch.float32, device=DEV)
    got = hip.spmm_f32(csr, dense, width=width, out=out).cpu().numpy().astype(np.float64)
    A64, D64 = A.astype(np.float64), D.astype(np.float64)
    want = np.asarray(A64 @ D64)
    tol = 2.0 ** -23 * (np.diff(A.indptr) + 8)[:, None] * np.asarray(abs(A64) @ np.abs(D64))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) - tol).max())
    assert (got[1] == 0).all()                                                              # the empty row
    assert (out[:, width:].cpu().numpy() == -7.0).all()                                     # nothing beyond `width` is written
    again = hip.spmm_f32(csr, dense, width=width).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.astype(np.float32).view(np.uint32))    # the same bits every run


def test_spmm_f32_refuses_more_than_4096_columns():
    import torch
    hip = _hip()
    A, _ = _spmm_case(4)
    csr = hip.DeviceCSR.from_arrays(A.indptr, A.indices, A.data, A.shape[1], DEV)
    for width in (4097, 5000):
        dense = torch.zeros(A.shape[1], (width + 3) & ~3, dtype=torch.float32, device=DEV)
        with pytest.raises(hip.AaeHipError, match="error -1"):
            hip.spmm_f32(csr, dense, width=width)
