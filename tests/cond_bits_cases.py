"""Shared by test_cond_bits_gpu.py: two consecutive steps (encode + update) of the trainable-condition kernels through each of
the three call families of aaerec._hip - cat_* (aae_cat_*), bag_* (aae_bag_*) and bag_csr_* (aae_bag_csr_*) - on off-grid
inputs, so that every sum rounds and a different order of the additions or a fused multiply-add shows in the bits.

tests/golden/cond_bits.json records one SHA-256 per (case, array) over the little-endian float32 bytes of the encoded blocks,
the table, exp_avg and exp_avg_sq after the second step.  The file pins the ORDER of the arithmetic and its CONTRACTION (which
products stay separate from the additions behind them) under one toolchain: the three families are held to each other bit for
bit elsewhere, which cannot see all of them drifting together - a change in a helper they share moves every route at once and
only the recorded digests notice.  When a toolchain change legitimately moves bits (a compiler that rounds a division or a
square root differently), regenerate the file on an MI355X with the library under test and say so in the commit:

    python tests/cond_bits_cases.py <commit the library was built from> [output file]
"""
import hashlib
import json
import os
import sys

import numpy as np

import bag_cases as BC
import ragged_cases as RC

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_bits.json")
ARRAYS = ("encode", "table", "exp_avg", "exp_avg_sq")
SHAPES = ((65, 65, 40), (3, 7, 2))          # (rows, dim, vocab) of the recorded cases
LR, STEPS = 1e-2, 2


def make_inputs(seed, rows, dim, vocab, pad, weighted=False):
    """Table, dout of every step (and weights) from standard_normal; the lists of ragged_cases.make_lists: a list of 130, the
    empty list, the all-out-of-vocabulary list, a table row named three times in one list and again in two others, the indices
    -3, vocab and 2^30."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((vocab, dim)).astype(f32)
    lists = RC.make_lists(rng, rows, vocab, pad)
    douts = [rng.standard_normal((rows, dim)).astype(f32) for _ in range(STEPS)]
    weights = [[f32(x) for x in rng.standard_normal(len(row))] for row in lists] if weighted else None
    return table, lists, douts, weights


def run(route, table, lists, douts, reduce, pad, sparse, weights=None):
    """STEPS steps through one call family.  route 'cat': cat_encode / cat_update (reduce SUM or MEAN_WIDTH, padding row 0);
    'bag': bag_encode / bag_update on ragged_cases.padded(lists, pad); 'csr': bag_csr_encode / bag_csr_update on the lists as
    resident DeviceBags.  The encode and gradient blocks are column slices of NaN-filled wider ones.  Returns (encode [STEPS,
    rows, dim], table, exp_avg, exp_avg_sq) as float32 arrays; asserts that no encode wrote outside its columns and that the
    gradient scratch is left zero."""
    import torch
    from aaerec import _hip
    dev = torch.device("cuda")
    rows, dim = douts[0].shape
    table = torch.from_numpy(np.array(table, dtype=f32)).to(dev)
    m, v, scratch = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    if route == "csr":
        src = _hip.DeviceBags(lists, dev, weights=None if weights is None else RC.flat(lists, weights)[2]).window(row0=0, rows=rows)
    else:
        assert weights is None, "per-sample weights exist on the CSR route only"
        src = torch.from_numpy(RC.padded(lists, pad).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(dev)
    if route == "cat":
        assert pad == 0 and reduce in (BC.SUM, BC.MEAN_WIDTH)
    outs = []
    for t, dout in enumerate(douts, start=1):
        block = torch.full((rows, dim + 5), float("nan"), device=dev)
        dblock = torch.full((rows, dim + 3), float("nan"), device=dev)
        dblock[:, 2:2 + dim] = torch.from_numpy(dout).to(dev)
        out, d = block[:, 3:3 + dim], dblock[:, 2:2 + dim]
        if route == "cat":
            _hip.cat_encode(table, src, out, mean=reduce == BC.MEAN_WIDTH)
            _hip.cat_update(table, m, v, src, d, LR, t, mean=reduce == BC.MEAN_WIDTH, grad_scratch=None if sparse else scratch)
        else:
            encode, update = (_hip.bag_csr_encode, _hip.bag_csr_update) if route == "csr" else (_hip.bag_encode, _hip.bag_update)
            encode(table, src, out, reduce=reduce, padding_idx=pad)
            update(table, m, v, src, d, LR, t, reduce=reduce, padding_idx=pad, grad_scratch=scratch, sparse=sparse)
        block = block.cpu().numpy()
        assert np.isnan(block[:, :3]).all() and np.isnan(block[:, 3 + dim:]).all(), "the encode wrote outside its columns"
        assert not scratch.any(), "the gradient scratch is left zero"
        outs.append(block[:, 3:3 + dim])
    return np.stack(outs), table.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f4").tobytes()).hexdigest()


def digests():
    """{case: {array: SHA-256}} of the recorded cases: the five reductions x {Adam, SparseAdam} x padding_idx {-1, 0} at both
    SHAPES - one digest where the padded and the CSR route both exist, asserted here -, BAG_SUM with per-sample weights through
    bag_csr_* under both optimisers, and cat_* in sum and mean mode."""
    found = {}

    def record(case, got):
        found[case] = {name: sha(a) for name, a in zip(ARRAYS, got)}
        return found[case]

    for rows, dim, vocab in SHAPES:
        shape = f"rows {rows} dim {dim} vocab {vocab}"
        for sparse in (False, True):
            opt = "sparse_adam" if sparse else "adam"
            for reduce, name in BC.NAMES.items():
                for pad in (-1, 0):
                    table, lists, douts, _ = make_inputs(100 * reduce + rows + pad, rows, dim, vocab, pad)
                    case = f"bag {name} {opt} pad {pad} {shape}"
                    padded = record(case, run("bag", table, lists, douts, reduce, pad, sparse))
                    csr = {name: sha(a) for name, a in zip(ARRAYS, run("csr", table, lists, douts, reduce, pad, sparse))}
                    for array in ARRAYS:
                        assert csr[array] == padded[array], f"{case}: {array} of the CSR route differs from the padded route's"
            for reduce in (BC.SUM, BC.MEAN_WIDTH):
                table, lists, douts, _ = make_inputs(900 + reduce + rows, rows, dim, vocab, 0)
                record(f"cat {BC.NAMES[reduce]} {opt} {shape}", run("cat", table, lists, douts, reduce, 0, sparse))
    rows, dim, vocab = SHAPES[0]
    for sparse in (False, True):
        table, lists, douts, weights = make_inputs(77, rows, dim, vocab, -1, weighted=True)
        record(f"csr weighted sum {'sparse_adam' if sparse else 'adam'} pad -1 rows {rows} dim {dim} vocab {vocab}",
               run("csr", table, lists, douts, BC.SUM, -1, sparse, weights))
    return found


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "aae-recommender_amd"))
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    import torch
    record = {"library_built_from": sys.argv[1], "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
              "digests": digests()}
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(record["digests"]), "cases")
