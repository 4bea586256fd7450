"""aae_cond_gather (csrc/cond_gather.h) and the resident route of the constant condition blocks, what can be checked without
a GPU: the entry point in the header, the ctypes table and the built library; every refusal of its argument check (it runs in
front of the first HIP call); the NumPy restatement _hip.cond_gather_host against plain indexing on the GPU test's cases
(gather_cases.py); and resident_condition_data's decision, with stand-in conditions."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import gather_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                 # include/aaerec_hip.h: AAE_EINVAL


def test_header_ctypes_table_and_library_carry_the_entry_point():
    from aaerec import _hip
    with open(os.path.join(ROOT, "include", "aaerec_hip.h")) as f:
        text = f.read()
    assert "int aae_cond_gather(const aae_cond_src* srcs, int32_t n_srcs, const int32_t* row_ids_dev, int64_t row0," in text
    assert "#define AAE_COND_SRC_MAX 8" in text and "#define AAE_ABI_VERSION 4" in text
    assert "typedef struct { const float* base_dev; int64_t ld; int64_t n_docs; int32_t width; int32_t col0; } aae_cond_src;" in text
    assert "aae_cond_gather" in _hip._PROTOS and _hip.COND_SRC_MAX == 8
    # the struct as the header lays it out: a pointer, two int64, two int32
    assert C.sizeof(_hip.AaeCondSrc) == 32
    assert [f[0] for f in _hip.AaeCondSrc._fields_] == ["base_dev", "ld", "n_docs", "width", "col0"]
    lib = _hip.load_library()
    assert hasattr(lib, "aae_cond_gather") and lib.aae_abi_version() == 4


def _call(lib, n_srcs=2, srcs="default", row_ids=4096, row0=0, rows=4, out=4096, out_ld=64, **over):
    """aae_cond_gather with plausible arguments (made-up non-NULL addresses: every refusal sits in front of the first HIP
    call, so nothing is dereferenced); `over` changes fields of the LAST source."""
    from aaerec import _hip
    arr = (_hip.AaeCondSrc * 9)()
    for i in range(9):
        arr[i] = _hip.AaeCondSrc(4096, 8, 100, 5, 6 * i)
    last = arr[max(0, min(n_srcs, 9) - 1)]
    for k, v in over.items():
        setattr(last, k, v)
    rc = lib.aae_cond_gather(None if srcs is None else arr, n_srcs, row_ids, row0, rows, out, out_ld, None)
    return rc, lib.aae_last_error().decode()


REFUSALS = [
    dict(n_srcs=0), dict(n_srcs=-1), dict(n_srcs=9),
    dict(srcs=None), dict(out=None), dict(base_dev=None),
    dict(width=0), dict(width=-3),
    dict(ld=4),                              # ld < width (5)
    dict(col0=-1),
    dict(col0=60),                           # col0 + width = 65 > out_ld = 64
    dict(out_ld=10),                         # the last source's columns end at 11
    dict(rows=-1),
    dict(n_docs=-1),
]


@pytest.mark.parametrize("over", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in REFUSALS])
def test_every_refusal_is_reached_in_front_of_the_first_hip_call(over):
    from aaerec import _hip
    lib = _hip.load_library()
    rc, msg = _call(lib, **over)
    assert rc == EINVAL and msg.startswith("aae_cond_gather: "), (over, rc, msg)
    # ... for every position of the bad source, and with rows == 0 as well: the check comes first
    if not ({"n_srcs", "srcs", "out", "rows", "out_ld"} & set(over)):
        for n in (1, 8):
            rc, msg = _call(lib, n_srcs=n, rows=0, **over)
            assert rc == EINVAL and msg.startswith("aae_cond_gather: "), (over, n, rc, msg)


def test_zero_rows_return_ok_without_a_launch():
    """rows == 0 with good arguments: 0, on a machine without a GPU too (nothing is launched); row_ids_dev may be NULL."""
    from aaerec import _hip
    lib = _hip.load_library()
    for n in (1, 2, 8):
        for ids in (4096, None):
            rc, msg = _call(lib, n_srcs=n, rows=0, row_ids=ids)
            assert rc == 0, (n, rc, msg)
    assert _call(lib, rows=0, n_docs=0)[0] == 0               # (an empty table is a table: every id is an empty row)
    assert _call(lib, rows=0, ld=5, col0=59)[0] == 0          # ld == width, col0 + width == out_ld: the edges are inside


@pytest.mark.parametrize("width", GC.WIDTHS)
def test_host_restatement_equals_plain_indexing(width):
    from aaerec import _hip
    for ld, shift, col0, out_ld, rows, kind, seed in GC.cases(width):
        _, view = GC.table_buffer(seed, GC.N_DOCS, width, ld, shift)
        ids, row0 = GC.row_ids(kind, rows, GC.N_DOCS, seed)
        got = _hip.cond_gather_host([view], ids, row0, rows, out=GC.sentinel(rows, out_ld).copy(), col0s=[col0])
        want = GC.plain_indexing([view], ids, row0, rows, GC.sentinel(rows, out_ld).copy(), [col0])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (width, ld, shift, col0, out_ld, rows, kind)
        # what the case is there for: the block's columns changed, every other column kept the prefill
        keep = np.ones(out_ld, dtype=bool)
        keep[col0:col0 + width] = False
        assert np.array_equal(got.view(np.uint32)[:, keep], GC.sentinel(rows, out_ld).view(np.uint32)[:, keep])
        assert not np.array_equal(got.view(np.uint32)[:, ~keep], GC.sentinel(rows, out_ld).view(np.uint32)[:, ~keep])


def test_host_restatement_eight_sources_and_defaults():
    from aaerec import _hip
    views = [GC.table_buffer(50 + i, n, w, ld, shift)[1] for i, (n, w, ld, shift, _) in enumerate(GC.EIGHT)]
    col0s, total = GC.eight_col0s()
    ids, _ = GC.row_ids("perm", 257, GC.N_DOCS, 9)
    got = _hip.cond_gather_host(views, ids, out=GC.sentinel(257, total + 4).copy(), col0s=col0s)
    want = GC.plain_indexing(views, ids, 0, 257, GC.sentinel(257, total + 4).copy(), col0s)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # defaults: one block behind the other from column 0 into a new block of zeros; the NULL form of the row ids
    got = _hip.cond_gather_host(views[:2], None, 296, 5)
    want = GC.plain_indexing(views[:2], None, 296, 5, np.zeros((5, 9), dtype=np.float32), [0, 4])
    assert got.shape == (5, 9) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[4].any()                                    # row 300: behind the table


# ---- resident_condition_data's decision ----------------------------------------------------------------------------------
class _Resident:
    def __init__(self, constant):
        self.constant_concat = constant
        self.asked = 0

    def resident(self, inputs, device):
        self.asked += 1
        return ("resident", inputs, device)

    def device_native(self, device):
        return True


class _NoResident:
    constant_concat = True


def _model(conds, flag, dp=None, native=True):
    return types.SimpleNamespace(conditions=dict(enumerate(conds)), resident_conditions=flag, _dp=dp,
                                 _is_device_native=lambda: native, hip=types.SimpleNamespace(device="cuda:0"))


def test_a_constant_block_becomes_resident_only_under_the_flag():
    from aaerec.aae import resident_condition_data
    data = ["const", "train", "own"]
    conds = [_Resident(True), _Resident(False), _NoResident()]
    assert resident_condition_data(_model(conds, False), data) == data and conds[0].asked == conds[1].asked == 0
    out = resident_condition_data(_model(conds, True), data)
    assert out[0] == ("resident", "const", "cuda:0") and out[1] == ("resident", "train", "cuda:0")
    assert out[2] == "own"                                   # a condition without resident() is left alone
    assert conds[0].asked == conds[1].asked == 1


def test_nothing_becomes_resident_under_data_parallelism_or_off_the_native_route():
    from aaerec.aae import resident_condition_data
    data = ["const", "train"]
    conds = [_Resident(True), _Resident(False)]
    assert resident_condition_data(_model(conds, True, dp=object()), data) == data
    assert resident_condition_data(_model(conds, True, native=False), data) == data
    assert conds[0].asked == conds[1].asked == 0
    # a resident() that declines (None) leaves the data as it is
    conds[0].resident = lambda inputs, device: None
    assert resident_condition_data(_model(conds, True), data)[0] == "const"


def test_a_subclass_with_its_own_encode_does_not_inherit_resident():
    """The gather stands for PretrainedWordEmbeddingCondition.encode, a cast: a subclass whose encode() does more keeps the
    per-step route (resident() answers None) instead of silently losing its encode."""
    from aaerec import _hip, condition as C

    class Vect:
        embedding = np.zeros((1, 3), dtype=np.float32)

        def fit(self, raw):
            return self

        def transform(self, raw):
            return np.asarray(raw)

    class Normalised(C.PretrainedWordEmbeddingCondition):
        def encode(self, inputs):
            x = super().encode(inputs)
            return x / x.norm(dim=1, keepdim=True)

    data = np.arange(12, dtype=np.float64).reshape(4, 3)
    plain = C.PretrainedWordEmbeddingCondition(Vect(), use_cuda=False)
    block = plain.resident(data, "cpu")
    assert isinstance(block, _hip.DeviceBlock) and np.array_equal(block.data.numpy(), plain.encode(data).numpy())
    assert Normalised(Vect(), use_cuda=False).resident(data, "cpu") is None
    assert plain.resident(np.zeros(5), "cpu") is None        # (not a matrix: the per-step route)


def test_device_block_and_take_on_the_host():
    """DeviceBlock's surface and _take's three row forms, on CPU tensors (no kernel is called)."""
    import torch
    from aaerec import _hip
    from aaerec.aae import _take
    host = np.arange(12, dtype=np.float64).reshape(4, 3)
    b = _hip.DeviceBlock(host, "cpu")
    assert len(b) == 4 and b.width == 3 and b.device == torch.device("cpu") and b.data.dtype == torch.float32
    w = _take(b, slice(1, 9))
    assert isinstance(w, _hip.BlockWindow) and (w.row_ids, w.row0, w.rows, len(w)) == (None, 1, 3, 3)
    ids = torch.tensor([3, 0], dtype=torch.int32)
    w = _take(b, np.array([3, 0]), ids)
    assert w.row_ids is ids and w.rows == 2 and w.block is b
    w = _take(b, np.array([2, 2, 1]))
    assert w.row_ids.dtype == torch.int32 and w.row_ids.tolist() == [2, 2, 1] and w.rows == 3
    with pytest.raises(TypeError):
        b.window(torch.tensor([1, 2]))                       # int64 row ids
    with pytest.raises(TypeError):
        _hip.DeviceBlock(np.zeros(5), "cpu")
