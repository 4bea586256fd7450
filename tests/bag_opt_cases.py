"""Shared by test_cond_bag_opts_cpu.py and test_cond_bag_opts_gpu.py: a NumPy restatement of nn.Embedding's max_norm (the
renorm in front of the lookup: csrc/cond_bag.h bag_row_norm / bag_row_renorm) and scale_grad_by_freq (bag_freq_scale) in
the kernels' operation order, on top of bag_cases' reductions, gradients and optimisers; the same steps in torch; and the
error bound of a renormalised element."""
import numpy as np

import bag_cases as BC
import ragged_cases as RC

f32 = np.float32
INF = float("inf")
NORM_TYPES = (1.0, 2.0, INF)


# ---- max_norm -------------------------------------------------------------------------------------------------------------
def row_norm(row, norm_type, dtype=f32):
    """The p-norm of a table row.  float32: the kernel's order - lane l sums |x|^p over its columns l, l + 64, l + 128, ..
    ascending, the 64 partial results fold by the xor butterfly 32, 16, .. 1, then (p = 2) the square root.  float64: the
    definition."""
    row = np.asarray(row)
    if dtype is not f32:
        return np.linalg.norm(row.astype(np.float64), ord=norm_type)
    lanes = np.zeros(64, dtype=f32)
    for k in range(0, len(row), 64):
        x = np.zeros(64, dtype=f32)
        x[:len(row[k:k + 64])] = row[k:k + 64]
        lanes = lanes + x * x if norm_type == 2.0 else lanes + np.abs(x) if norm_type == 1.0 else np.maximum(lanes, np.abs(x))
    for d in (32, 16, 8, 4, 2, 1):
        other = lanes[np.arange(64) ^ d]
        lanes = np.maximum(lanes, other) if norm_type == INF else lanes + other
    return np.sqrt(lanes[0]) if norm_type == 2.0 else lanes[0]


def named_rows(idx, vocab):
    """The distinct table rows an input names: every index inside the table, a padding row included."""
    flat = np.asarray([j for row in idx for j in row], dtype=np.int64) if not isinstance(idx, np.ndarray) else idx.reshape(-1)
    return np.unique(flat[(flat >= 0) & (flat < vocab)])


def renorm(table, idx, max_norm, norm_type, dtype=f32):
    """torch's embedding_renorm_ in place on `table` (of dtype `dtype`): every distinct named row whose norm is strictly above
    max_norm times max_norm / (norm + 1e-7), once.  Returns the rows it scaled."""
    assert table.dtype == dtype
    mx, eps = dtype(f32(max_norm)), dtype(1e-7)                 # (max_norm reaches the kernels as a float32)
    scaled = []
    for j in named_rows(idx, table.shape[0]):
        n = row_norm(table[j], norm_type, dtype)
        if n > mx:
            table[j] = table[j] * (mx / (n + eps))
            scaled.append(int(j))
    return scaled


def renorm_bound(old_row, dim, max_norm):
    """|element after the renorm - the float64 restatement's| for any float32 evaluation: the norm is a sum of
    `dim` non-negative terms - relative error at most (dim + 2) u in any order, the square root included -, the add of 1e-7,
    the division and the product add 4 u, and a row whose decision flips against the restatement has norm within that of
    max_norm, so its scale is within it plus 1e-7 / max_norm of 1.  |new| <= |old|, so the bound is taken on |old|."""
    u = 2.0 ** -24
    return np.abs(np.asarray(old_row, dtype=np.float64)) * ((dim + 6) * u + 1e-7 / max_norm)


def torch_renorm(table, idx, max_norm, norm_type, bag, device="cpu"):
    """The table after one forward of nn.EmbeddingBag(mode='sum') (bag) or nn.Embedding on the 2-D input idx."""
    import torch
    import torch.nn as nn
    vocab, dim = table.shape
    mod = (nn.EmbeddingBag(vocab, dim, mode="sum", max_norm=max_norm, norm_type=norm_type) if bag else
           nn.Embedding(vocab, dim, max_norm=max_norm, norm_type=norm_type)).to(device)
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(np.asarray(table, dtype=f32)))
    mod.eval()                                                  # (the renorm runs in eval too)
    mod(torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(device))
    return mod.weight.detach().cpu().numpy().copy()


def renorm_case(seed, rows, width, dim, vocab, pad, norm_type, on_grid=True):
    """A table, an input and a max_norm with rows above it and below it; on the grid (multiples of 1/8: with norm_type 1 and
    inf the norm is exact) one row lies EXACTLY at max_norm, and - vocab 40 - one row is all zero.  The input is
    bag_cases.make_idx's (a bag repeating one row, one row named by many bags, the padding row named) plus, where there is
    room, an index behind the table and a negative one.  Returns table, idx, max_norm, at (the row at max_norm or -1)."""
    rng = np.random.default_rng(seed)
    table = BC.make_table(rng, vocab, dim, -1) if on_grid else rng.standard_normal((vocab, dim)).astype(f32)
    if on_grid:                                                 # rows of different size under every norm (inf: 0.5, 1, .. 4)
        caps = (np.arange(vocab) % 8 + 1) / 2.0
        table = np.clip(table, -caps[:, None], caps[:, None]).astype(f32)
    idx = BC.make_idx(rng, rows, width, vocab, pad)
    if rows >= 5 and width >= 2:
        idx[3, 0], idx[3, width - 1] = vocab, -3
    named = named_rows(idx, vocab)
    if vocab >= 40 and on_grid:
        table[named[len(named) // 2]] = 0
    norms = np.array([row_norm(r, norm_type, np.float64) for r in table])
    order = named[np.argsort(norms[named], kind="stable")]
    at = int(order[len(order) // 2])                            # the median named row: named rows above and below it
    max_norm = float(f32(norms[at])) if norms[at] > 0 else 1.0
    if not on_grid or norm_type == 2.0:
        at = -1                                                 # (a rounded norm: the row may fall on either side)
    return table, idx, max_norm, at


# ---- scale_grad_by_freq ----------------------------------------------------------------------------------------------------
def counts(idx, vocab):
    """How often every table row occurs among all indices of the mini-batch (every bag, whatever wins or weighs)."""
    flat = np.asarray([j for row in idx for j in row], dtype=np.int64) if not isinstance(idx, np.ndarray) else idx.reshape(-1)
    return np.bincount(flat[(flat >= 0) & (flat < vocab)], minlength=vocab)


def settle_gradients(table, idx, dout, reduce, pad):
    """bag_cases.settle_mean_gradients for every reduction: behind a division by a count of 3 or 5 contributions that cancel
    in exact arithmetic leave a residue that depends on whether one divides the sum (the kernels) or every contribution
    (torch), and Adam turns such a residue into a step of up to lr.  Where a gradient element some bag contributes to is
    below 1/64, the dout entry of the first contributing bag moves by a grid step, until none is left."""
    table, idx, dout = np.asarray(table, dtype=f32), np.asarray(idx), np.asarray(dout, dtype=f32).copy()
    ok = BC.live(idx, table.shape[0], pad)
    _, win = BC.bag_encode(table, idx, reduce, pad)
    for _ in range(400):
        g, rows = BC.bag_grad(table, idx, reduce, pad, dout)
        bad = [(j, d) for j in rows for d in np.nonzero(np.abs(g[j]) < 1 / 64)[0]]
        moved = False
        for j, d in bad:
            for r in range(idx.shape[0]):
                slots = np.nonzero(ok[r] & (idx[r] == j))[0]
                if len(slots) and (reduce < BC.MAX_PAD0 or win[r, d] in slots):
                    dout[r, d] = dout[r, d] + f32(0.125) if dout[r, d] < 4 else f32(-4)
                    moved = True
                    break
        if not moved:
            return dout
    raise AssertionError("the gradients did not settle")


def freq_grad(table, idx, reduce, pad, dout, weights=None):
    """bag_cases.bag_grad (lists with weights: ragged_cases.grad) with every row's sum divided by its count: one float32
    division per element, behind the sum."""
    if isinstance(idx, np.ndarray):
        g, rows = BC.bag_grad(table, idx, reduce, pad, dout)
    else:
        g, rows = RC.grad(table, idx, reduce, pad, dout, weights)
    n = counts(idx, table.shape[0])
    for j in rows:
        g[j] = g[j] / f32(n[j])
    return g, rows


def step(table, m, v, idx, reduce, pad, dout, lr, t, sparse=False, max_norm=None, norm_type=2.0, by_freq=False, weights=None):
    """renorm + encode + backward + optimiser step t in place; returns the encoded block.  idx: a [rows, width] array or
    value lists (weights: per-sample weights, SUM only).  Without options: bag_cases.bag_step / ragged_cases.step."""
    if max_norm is not None:
        renorm(table, idx, max_norm, norm_type)
    if not by_freq:
        if isinstance(idx, np.ndarray):
            return BC.bag_step(table, m, v, idx, reduce, pad, dout, lr, t, sparse)
        return RC.step(table, m, v, idx, reduce, pad, dout, lr, t, sparse, weights)
    assert not sparse, "torch has no sparse gradient scaled by frequency"
    out = BC.bag_encode(table, idx, reduce, pad)[0] if isinstance(idx, np.ndarray) else RC.encode(table, idx, reduce, pad, weights)[0]
    g, _ = freq_grad(table, idx, reduce, pad, dout, weights)
    BC.adam_dense(table, m, v, g, lr, t)
    return out


def torch_embedding_steps(table, idx_steps, reduce, pad, dout_steps, lr, max_norm=None, norm_type=2.0, by_freq=False):
    """The steps through nn.Embedding(sparse=False) followed by the explicit .sum(1) / .mean(1) / .max(1)[0] under
    torch.optim.Adam on the CPU - the form whose dense backward scales by frequency correctly (CPU nn.EmbeddingBag's does
    not: DESIGN 3.7b).  reduce: SUM, MEAN_WIDTH or MAX_PAD0 (a padding row must hold zeros: nn.Embedding reads it).
    Returns (encoded blocks, table, exp_avg, exp_avg_sq)."""
    import torch
    import torch.nn as nn
    vocab, dim = table.shape
    assert pad < 0 or not np.asarray(table)[pad].any()
    mod = nn.Embedding(vocab, dim, padding_idx=None if pad < 0 else pad, sparse=False, max_norm=max_norm, norm_type=norm_type,
                       scale_grad_by_freq=by_freq)
    fwd = {BC.SUM: lambda i: mod(i).sum(1), BC.MEAN_WIDTH: lambda i: mod(i).mean(1), BC.MAX_PAD0: lambda i: mod(i).max(1)[0]}[reduce]
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(np.asarray(table, dtype=f32)))
    opt = torch.optim.Adam(mod.parameters(), lr=lr)
    outs = []
    for idx, dout in zip(idx_steps, dout_steps):
        opt.zero_grad()
        out = fwd(torch.from_numpy(np.asarray(idx, dtype=np.int64)))
        out.backward(torch.from_numpy(np.asarray(dout, dtype=f32)))
        opt.step()
        outs.append(out.detach().numpy().copy())
    st = opt.state[mod.weight]
    return outs, mod.weight.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
