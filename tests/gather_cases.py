"""The cases of aae_cond_gather (csrc/cond_gather.h) that test_cond_gather_cpu.py holds the NumPy restatement to and
test_cond_gather_gpu.py the kernel: tables seeded with NaN payloads, -0.0, infinities and denormals, laid out so that every
branch of the kernel's alignment choice is reached (ld a multiple of 4 or not, the base on 16 bytes or one float off, col0 and
out_ld multiples of 4 or not), widths around the quad (the tail behind the last full quad), row counts around the workgroup's
four rows, and every way of naming rows."""
import numpy as np

N_DOCS = 300
WIDTHS = (1, 3, 4, 5, 300, 301)
ROWS = (1, 3, 4, 5, 64, 257)
COL0S = (0, 1, 4, 50)
IDS = ("perm", "repeat", "reversed", "range")
SPECIALS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF],
                    dtype=np.uint32)        # quiet / negative / signalling NaN payloads, -0.0, +-inf, denormals


def table_buffer(seed, n_docs, width, ld, shift):
    """(flat float32 buffer, its [n_docs, width] view of row stride ld that starts `shift` floats in).  The buffer ends with the
    last row's last column: with ld == width and no shift the table fills it exactly."""
    rng = np.random.default_rng(seed)
    buf = rng.standard_normal(shift + (n_docs - 1) * ld + width).astype(np.float32)
    bits = buf.view(np.uint32)
    where = rng.random(len(buf)) < 0.08
    bits[where] = rng.choice(SPECIALS, int(where.sum()))
    view = np.lib.stride_tricks.as_strided(buf[shift:], shape=(n_docs, width), strides=(4 * ld, 4), writeable=False)
    return buf, view


def sentinel(rows, out_ld):
    """The prefill of an output block: a different word in every element, none of them a word of a table by accident."""
    return (np.uint32(0xDEAD0000) + np.arange(rows * out_ld, dtype=np.uint32) % np.uint32(0xFFFF)).reshape(rows, out_ld).view(np.float32)


def row_ids(kind, rows, n_docs, seed):
    """(row_ids or None, row0) of a call.  The id lists of three rows or more name one row in front of the table (-1) and one
    behind it (n_docs); the NULL form with row0 > 0 runs one row past the table's end in every second case."""
    rng = np.random.default_rng(seed)
    if kind == "range":
        return None, (n_docs - rows + 1 if seed % 2 else 7)
    if kind == "perm":
        ids = rng.permutation(n_docs)[:rows]
    elif kind == "repeat":
        ids = rng.integers(0, max(1, rows // 3), rows)
    else:
        ids = np.arange(n_docs - 1, n_docs - 1 - rows, -1)
    ids = ids.astype(np.int32)
    if rows >= 3:
        ids[1], ids[-1] = -1, n_docs
    return ids, 0


def cases(width):
    """The 32 alignment combinations of one width: (ld, shift, col0, out_ld, rows, kind, seed).  Row counts and id kinds cycle
    over all 192 cases, so every (rows, kind) pair meets eight alignment combinations."""
    out, g = [], WIDTHS.index(width) * 32
    for ld_extra in (0, 3):
        for shift in (0, 1):
            for col0 in COL0S:
                for odd in (0, 1):
                    out_ld = (col0 + width + 2 + 3) // 4 * 4 + odd
                    out.append((width + ld_extra, shift, col0, out_ld, ROWS[g % 6], IDS[(g // 6) % 4], g))
                    g += 1
    return out


def plain_indexing(views, ids, row0, rows, out, col0s):
    """The definition, with plain NumPy indexing a row at a time, on uint32 words."""
    bits = out.view(np.uint32)
    for view, c in zip(views, col0s):
        words = np.ascontiguousarray(view).view(np.uint32)
        for r in range(rows):
            i = int(ids[r]) if ids is not None else row0 + r
            bits[r, c:c + view.shape[1]] = words[i] if 0 <= i < view.shape[0] else 0
    return out


# eight sources in one call: (n_docs, width, ld, shift, gap in front of the block).  Blocks 0 and 1 are adjacent (gap 0), so
# are 4 and 5; the shorter tables make one id a row of one block and an empty row of another
EIGHT = ((300, 4, 4, 0, 0), (300, 5, 8, 0, 0), (200, 300, 300, 0, 3), (300, 1, 1, 1, 2), (120, 8, 12, 0, 1), (300, 3, 3, 0, 0),
         (300, 301, 304, 1, 4), (300, 12, 12, 0, 1))


def eight_col0s():
    col0s, off = [], 0
    for _, width, _, _, gap in EIGHT:
        col0s.append(off + gap)
        off += gap + width
    return col0s, off
