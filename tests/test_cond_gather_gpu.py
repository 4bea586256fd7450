"""aae_cond_gather (csrc/cond_gather.h) on the device against its NumPy restatement _hip.cond_gather_host, compared as uint32
words: a gather is a copy, so NaN payloads and -0.0 arrive as they are.  The cases (gather_cases.py) reach every branch of the
alignment choice, the tail behind the last quad, a partial last workgroup, every way of naming rows and rows outside the table;
one case holds the 64-bit offsets with a table whose last row starts 2^31 floats in."""
import numpy as np
import pytest
import torch

import gather_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_view(buf, n_docs, width, ld, shift):
    """The table on the device at the host view's offset from a fresh allocation (the caching allocator hands out 512-byte
    aligned blocks: shift 1 moves the base off 16 bytes)."""
    t = torch.from_numpy(buf).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t.as_strided((n_docs, width), (ld, 1), shift)


def _ids_dev(ids):
    return None if ids is None else torch.from_numpy(ids).to(DEV)


@pytest.mark.parametrize("width", GC.WIDTHS)
def test_kernel_equals_the_host_restatement_bit_for_bit(width):
    from aaerec import _hip
    tables, vec = {}, 0
    for ld, shift, col0, out_ld, rows, kind, seed in GC.cases(width):
        key = (ld, shift)
        if key not in tables:
            buf, view = GC.table_buffer(1000 + 7 * width + 2 * ld + shift, GC.N_DOCS, width, ld, shift)
            tables[key] = (view, _hip.DeviceBlock(_device_view(buf, GC.N_DOCS, width, ld, shift)))
        view, block = tables[key]
        ids, row0 = GC.row_ids(kind, rows, GC.N_DOCS, seed)
        want = _hip.cond_gather_host([view], ids, row0, rows, out=GC.sentinel(rows, out_ld).copy(), col0s=[col0])
        out = torch.from_numpy(GC.sentinel(rows, out_ld).copy()).to(DEV)
        assert out.data_ptr() % 16 == 0
        got = _hip.cond_gather([block.window(_ids_dev(ids), row0, rows)], out=out, col0s=[col0])
        assert got is out
        tag = f"width {width} ld {ld} shift {shift} col0 {col0} out_ld {out_ld} rows {rows} ids {kind}"
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), tag
        vec += width >= 4 and ld % 4 == 0 and shift == 0 and col0 % 4 == 0 and out_ld % 4 == 0
    # A check of the CASE LIST, not of the kernel: by the entry point's alignment rule, restated above from the case's own
    # parameters, 2 of the 32 cases of a width of a quad or more qualify for the 16-byte path.  Which path the kernel took
    # cannot be seen from its output (both copy the same bits); the next test runs that alignment over every row count.
    assert vec == (2 if width >= 4 else 0)


@pytest.mark.parametrize("width,ld", [(4, 4), (5, 8), (300, 300), (301, 304)])
def test_the_16_byte_path_over_every_row_count_and_id_form(width, ld):
    """The alignment that takes 16-byte loads and stores (base and out on 16 bytes, ld, col0 and out_ld multiples of 4) with
    every row count and every way of naming rows; widths 5 and 301 leave one column behind the last quad."""
    from aaerec import _hip
    buf, view = GC.table_buffer(2000 + width, GC.N_DOCS, width, ld, 0)
    block = _hip.DeviceBlock(_device_view(buf, GC.N_DOCS, width, ld, 0))
    col0, out_ld = 4, (width + 4 + 3) // 4 * 4 + 4
    for rows in GC.ROWS:
        for k, kind in enumerate(GC.IDS):
            ids, row0 = GC.row_ids(kind, rows, GC.N_DOCS, rows + k)
            want = _hip.cond_gather_host([view], ids, row0, rows, out=GC.sentinel(rows, out_ld).copy(), col0s=[col0])
            out = torch.from_numpy(GC.sentinel(rows, out_ld).copy()).to(DEV)
            assert out.data_ptr() % 16 == 0 and block.data.data_ptr() % 16 == 0
            _hip.cond_gather([block.window(_ids_dev(ids), row0, rows)], out=out, col0s=[col0])
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (width, rows, kind)


@pytest.mark.parametrize("odd", [0, 1], ids=["out_ld%4==0", "out_ld%4==1"])
def test_eight_sources_in_one_call(odd):
    """Eight blocks of different widths, strides and lengths in one launch, two pairs of them in adjacent columns, gaps
    between the others: the gaps and the columns behind the last block keep the prefill."""
    from aaerec import _hip
    views, blocks = [], []
    for i, (n, w, ld, shift, _) in enumerate(GC.EIGHT):
        buf, view = GC.table_buffer(50 + i, n, w, ld, shift)
        views.append(view)
        blocks.append(_hip.DeviceBlock(_device_view(buf, n, w, ld, shift)))
    col0s, total = GC.eight_col0s()
    out_ld = (total + 3) // 4 * 4 + 4 + odd
    for kind, rows in (("perm", 257), ("range", 5)):
        ids, row0 = GC.row_ids(kind, rows, GC.N_DOCS, 9)
        want = _hip.cond_gather_host(views, ids, row0, rows, out=GC.sentinel(rows, out_ld).copy(), col0s=col0s)
        out = torch.from_numpy(GC.sentinel(rows, out_ld).copy()).to(DEV)
        ids_dev = _ids_dev(ids)
        _hip.cond_gather([b.window(ids_dev, row0, rows) for b in blocks], out=out, col0s=col0s)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want.view(np.uint32)), (kind, rows)
        named = np.zeros(out_ld, dtype=bool)
        for c, v in zip(col0s, views):
            named[c:c + v.shape[1]] = True
        assert (~named).sum() >= 11 and np.array_equal(got[:, ~named], GC.sentinel(rows, out_ld).view(np.uint32)[:, ~named])
    # a ninth window, or windows that name different rows, are refused by the wrapper
    with pytest.raises(ValueError):
        _hip.cond_gather([blocks[0].window(row0=0, rows=2)] * 9)
    with pytest.raises(ValueError):
        _hip.cond_gather([blocks[0].window(row0=0, rows=2), blocks[1].window(row0=1, rows=2)])


def test_defaults_allocate_the_block_and_place_the_windows_one_behind_the_other():
    from aaerec import _hip
    a = torch.arange(12, dtype=torch.float32, device=DEV).reshape(4, 3)
    b = -torch.arange(20, dtype=torch.float32, device=DEV).reshape(4, 5)
    ids = torch.tensor([3, 1, 3], dtype=torch.int32, device=DEV)
    out = _hip.cond_gather([_hip.DeviceBlock(a).window(ids), _hip.DeviceBlock(b).window(ids)])
    assert out.shape == (3, 8) and torch.equal(out, torch.cat([a[ids.long()], b[ids.long()]], 1))
    # a column slice of a wider block as `out`: the row stride is the block's
    wide = torch.full((3, 16), 7.0, device=DEV)
    _hip.cond_gather([_hip.DeviceBlock(b).window(ids)], out=wide[:, 4:9])
    assert torch.equal(wide[:, 4:9], b[ids.long()]) and (wide[:, :4] == 7).all() and (wide[:, 9:] == 7).all()


def test_offsets_are_64_bit():
    """A table of 2^23 + 1 rows at ld 256: its last row starts 2^31 floats in.  Only the first and the last row are written
    (torch.empty: 8.6 GB, untouched in between) and exactly those two are gathered."""
    from aaerec import _hip
    n_docs, ld = (1 << 23) + 1, 256
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 12 * (1 << 30):
        pytest.skip("less than 12 GB of device memory free")
    table = torch.empty(n_docs, ld, dtype=torch.float32, device=DEV)
    rows = torch.from_numpy(GC.table_buffer(77, 2, ld, ld, 0)[1].copy()).to(DEV)
    table[0].copy_(rows[0])
    table[n_docs - 1].copy_(rows[1])
    ids = torch.tensor([n_docs - 1, 0, n_docs, n_docs - 1], dtype=torch.int32, device=DEV)
    out = _hip.cond_gather([_hip.DeviceBlock(table).window(ids)])
    want = torch.stack([rows[1], rows[0], torch.zeros_like(rows[0]), rows[1]])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    # the NULL form: row0 + r in 64 bits
    out = _hip.cond_gather([_hip.DeviceBlock(table).window(row0=n_docs - 1, rows=2)])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), torch.stack([rows[1], torch.zeros_like(rows[1])]).cpu().numpy().view(np.uint32))
    del table
