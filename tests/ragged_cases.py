"""Shared by test_cond_ragged_cpu.py and test_cond_ragged_gpu.py: a NumPy restatement of the bag reductions over RAGGED value
lists (csrc/cond_csr.h: aae_bag_csr_encode / aae_bag_csr_update) - no padded rectangle, entries walked in list order -, their
backward and the two optimisers, the same steps in torch's (input, offsets, per_sample_weights) call form, and the list
generators.  Held to bag_cases.bag_step on the padded form and to torch in test_cond_ragged_cpu.py."""
import numpy as np

import bag_cases as BC

f32 = np.float32
SUM, MEAN_WIDTH, MEAN_COUNT, MAX_PAD0, MAX = BC.SUM, BC.MEAN_WIDTH, BC.MEAN_COUNT, BC.MAX_PAD0, BC.MAX


def width_of(lists):
    """What _pad_batch pads a batch to: its longest list, at least 1."""
    return max(1, max((len(row) for row in lists), default=0))


def padded(lists, pad):
    """The [rows, width] block of the padded route: the lists followed by padding slots (the padding row, or -1 - a dead
    index - where the table has none)."""
    fill = pad if pad >= 0 else -1
    idx = np.full((len(lists), width_of(lists)), fill, dtype=np.int64)
    for r, row in enumerate(lists):
        idx[r, :len(row)] = row
    return idx


def _live(j, vocab, pad):
    return 0 <= j < vocab and j != pad


def encode(table, lists, reduce, pad, weights=None):
    """out [rows, dim] float32 and win [rows, dim] (max modes: the position in the list of the first entry attaining the
    maximum; -1: none or MAX_PAD0's zero candidate).  weights: one list of float32 per row (SUM only)."""
    table = np.asarray(table, dtype=f32)
    vocab, dim = table.shape
    width = width_of(lists)
    out, win = np.zeros((len(lists), dim), dtype=f32), np.full((len(lists), dim), -1, dtype=np.int64)
    for r, row in enumerate(lists):
        acc, n, have = np.zeros(dim, dtype=f32), 0, False
        for w, j in enumerate(row):
            ok = _live(j, vocab, pad)
            n += ok
            if reduce < MAX_PAD0:
                if ok:
                    acc = acc + (table[j] if weights is None else f32(weights[r][w]) * table[j])
                continue
            if not ok and reduce == MAX:
                continue
            t = table[j] if ok else np.zeros(dim, dtype=f32)
            better = np.ones(dim, dtype=bool) if not have else t > acc
            acc, win[r], have = np.where(better, t, acc), np.where(better, w if ok else -1, win[r]), True
        if reduce == MAX_PAD0 and len(row) < width:         # the padding slots behind the list: one candidate of value 0
            better = np.ones(dim, dtype=bool) if not have else f32(0) > acc
            acc, win[r] = np.where(better, f32(0), acc), np.where(better, -1, win[r])
        if reduce == MEAN_WIDTH:
            acc = acc / f32(width)
        elif reduce == MEAN_COUNT:
            acc = acc / f32(n) if n else np.zeros(dim, dtype=f32)
        out[r] = acc
    return out, win


def grad(table, lists, reduce, pad, dout, weights=None):
    """g [vocab, dim] float32 - the entries naming a table row summed in (row of the batch, position in the list) order - and
    the sorted table rows the batch names."""
    table, dout = np.asarray(table, dtype=f32), np.asarray(dout, dtype=f32)
    vocab, dim = table.shape
    width = width_of(lists)
    _, win = encode(table, lists, reduce, pad)
    g, named = np.zeros((vocab, dim), dtype=f32), set()
    for r, row in enumerate(lists):
        n = sum(_live(j, vocab, pad) for j in row)
        for w, j in enumerate(row):
            if not _live(j, vocab, pad):
                continue
            named.add(int(j))
            if reduce == SUM:
                c = dout[r] if weights is None else f32(weights[r][w]) * dout[r]
            elif reduce == MEAN_WIDTH:
                c = dout[r] / f32(width)
            elif reduce == MEAN_COUNT:
                c = dout[r] / f32(n)
            else:
                c = np.where(win[r] == w, dout[r], f32(0))
            g[j] = g[j] + c
    return g, np.array(sorted(named), dtype=np.int64)


def step(table, m, v, lists, reduce, pad, dout, lr, t, sparse, weights=None):
    """encode + backward + optimiser step t (1-based) in place (bag_cases' optimisers); returns the encoded block."""
    out, _ = encode(table, lists, reduce, pad, weights)
    g, rows = grad(table, lists, reduce, pad, dout, weights)
    if sparse:
        BC.adam_sparse(table, m, v, rows, g, lr, t)
    else:
        BC.adam_dense(table, m, v, g, lr, t)
    return out


def flat(lists, weights=None):
    """(indices int64, offsets int64 [rows], weights float32 or None): nn.EmbeddingBag's 1-D call form."""
    lens = np.array([len(row) for row in lists], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lists) else np.zeros(0, dtype=np.int64)
    idx = np.array([j for row in lists for j in row], dtype=np.int64)
    wts = None if weights is None else np.array([x for row in weights for x in row], dtype=f32)
    return idx, offsets, wts


def torch_steps(table, lists_steps, reduce, pad, dout_steps, lr, sparse, weights_steps=None):
    """The same steps in torch on the CPU: nn.EmbeddingBag(input, offsets, per_sample_weights) for SUM / MEAN_COUNT / MAX
    under torch.optim.Adam / SparseAdam.  Returns (encoded blocks, table, exp_avg, exp_avg_sq)."""
    import torch
    import torch.nn as nn
    vocab, dim = table.shape
    mod = nn.EmbeddingBag(vocab, dim, mode={SUM: "sum", MEAN_COUNT: "mean", MAX: "max"}[reduce],
                          padding_idx=None if pad < 0 else pad, sparse=sparse)
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(np.asarray(table, dtype=f32)))
    opt = (torch.optim.SparseAdam if sparse else torch.optim.Adam)(mod.parameters(), lr=lr)
    outs = []
    for s, (lists, dout) in enumerate(zip(lists_steps, dout_steps)):
        idx, offsets, wts = flat(lists, None if weights_steps is None else weights_steps[s])
        opt.zero_grad()
        out = mod(torch.from_numpy(idx), torch.from_numpy(offsets), None if wts is None else torch.from_numpy(wts))
        out.backward(torch.from_numpy(np.asarray(dout, dtype=f32)))
        opt.step()
        outs.append(out.detach().numpy().copy())
    st = opt.state[mod.weight]
    zeros = np.zeros((vocab, dim), dtype=f32)
    return (outs, mod.weight.detach().numpy().copy(), st["exp_avg"].numpy().copy() if "exp_avg" in st else zeros,
            st["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in st else zeros)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def make_lists(rng, rows, vocab, pad, long_row=130, outside=True):
    """`rows` value lists with lengths drawn from 0-5 and then, where the shape has room: one list of `long_row` entries (a
    row that crosses a wavefront's 64 lanes twice), an empty list, a list of out-of-vocabulary values only, and one table row
    named three times within one list and again in two others.  outside: the indices -3, vocab and 2^30 appear."""
    lists = [[int(j) for j in rng.integers(0, vocab, size=int(rng.integers(0, 6)))] for _ in range(rows)]
    hot = int(rng.integers(0, vocab))
    if pad >= 0 and hot == pad:
        hot = (hot + 1) % vocab
    lists[0] = [int(j) for j in rng.integers(0, vocab, size=long_row)]
    if rows >= 3:
        lists[1] = []
        lists[2] = [vocab, -3, 2 ** 30] if outside else [hot]
    if rows >= 8:
        lists[3] = [hot, int(rng.integers(0, vocab)), hot, hot]
        lists[5] = lists[5] + [hot]
        lists[7] = [hot] + lists[7]
        if outside:
            lists[4] = lists[4] + [-3]
            lists[6] = [2 ** 30] + lists[6] + [vocab]
    return lists


def make_weights(rng, lists):
    """per_sample_weights on the 1/8 grid, never 0."""
    values = np.concatenate([np.arange(-16, 0), np.arange(1, 17)]) / 8.0
    return [[f32(x) for x in rng.choice(values, size=len(row))] for row in lists]


def ties_free(table, lists, reduce, pad):
    return BC.no_cross_ties(table, padded(lists, pad), reduce, pad)


def make_case(seed, rows, dim, vocab, reduce, pad, long_row=130, outside=True):
    """Table, lists and dout on the 1/8 grid (sums exact in any order; no two different table rows tie in a bag; no mean
    gradient of a named row near Adam's eps), as bag_cases.make_case draws them."""
    rng = np.random.default_rng(seed)
    for _ in range(200):
        table, lists = BC.make_table(rng, vocab, dim, pad), make_lists(rng, rows, vocab, pad, long_row, outside)
        if reduce < MAX_PAD0 or ties_free(table, lists, reduce, pad):
            dout = BC.grid(rng, (rows, dim))
            if reduce in (MEAN_WIDTH, MEAN_COUNT):
                # behind a division by up to `width` no gradient of a named row may end near Adam's eps (bag_cases.
                # settle_mean_gradients: below 1/64): one sign, so nothing cancels, and at least width / 64 in size
                lo = int(np.ceil(width_of(lists) / 8.0)) + 1
                assert lo <= 32, "the longest list is too long for a settled mean gradient on the grid"
                dout = (rng.integers(lo, 33, size=(rows, dim)) / 8.0).astype(f32)
            dout = BC.settle_mean_gradients(padded(lists, pad), dout, vocab, pad, reduce)
            return dict(table=table, lists=lists, dout=dout, reduce=reduce, pad=pad)
    raise AssertionError("no tie-free inputs in 200 draws")
