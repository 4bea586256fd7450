"""Shared by test_cond_bag_cpu.py and test_cond_bag_gpu.py: a NumPy restatement of the five bag reductions of
csrc/cond_bag.h (aae_bag_encode / aae_bag_update), their backward and the two optimisers, the same thing in torch (the
definition: it is what the reference calls), the input generators, and the condition stand-ins that replay the reference's
recorded runs on the oracle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32 = np.float32
SUM, MEAN_WIDTH, MEAN_COUNT, MAX_PAD0, MAX = range(5)           # include/aaerec_hip.h: AAE_BAG_*
NAMES = {SUM: "sum", MEAN_WIDTH: "mean_width", MEAN_COUNT: "mean_count", MAX_PAD0: "max_pad0", MAX: "max"}

# the reference's recorded runs (tools/gen_golden.py bagcond): fixture -> (model, condition kind)
BAG_FIXTURES = {"step_cat_max": ("aae", "cat"), "step_cat_max_dense": ("aae", "cat"), "step_bag_mean": ("aae", "bag"),
                "step_bag_max": ("aae", "bag"), "step_vae_bag": ("vae", "bag")}
BAG_MODES = {"sum": SUM, "mean": MEAN_COUNT, "max": MAX}         # nn.EmbeddingBag's mode -> reduction


# ---- the restatement ---------------------------------------------------------------------------------------------------
def live(idx, vocab, pad):
    idx = np.asarray(idx)
    return (idx >= 0) & (idx < vocab) & (idx != pad)


def bag_encode(table, idx, reduce, pad):
    """out [rows, dim] float32 and win [rows, dim]: the first slot attaining the maximum (max modes; -1: none, or a padding
    slot in MAX_PAD0).  Sums run in slot order in float32."""
    table, idx = np.asarray(table, dtype=f32), np.asarray(idx)
    rows, width = idx.shape
    vocab, dim = table.shape
    ok = live(idx, vocab, pad)
    out, win = np.zeros((rows, dim), dtype=f32), np.full((rows, dim), -1, dtype=np.int64)
    for r in range(rows):
        if reduce in (SUM, MEAN_WIDTH, MEAN_COUNT):
            acc = np.zeros(dim, dtype=f32)
            for w in range(width):
                if ok[r, w]:
                    acc = acc + table[idx[r, w]]
            n = int(ok[r].sum())
            out[r] = acc / f32(width) if reduce == MEAN_WIDTH else (acc / f32(n) if n else 0) if reduce == MEAN_COUNT else acc
            continue
        have = False
        for w in range(width):
            if not ok[r, w] and reduce == MAX:
                continue
            t = table[idx[r, w]] if ok[r, w] else np.zeros(dim, dtype=f32)
            better = np.ones(dim, dtype=bool) if not have else t > out[r]
            out[r] = np.where(better, t, out[r])
            win[r] = np.where(better, w if ok[r, w] else -1, win[r])
            have = True
    return out, win


def bag_grad(table, idx, reduce, pad, dout):
    """g [vocab, dim] float32 (contributions summed in slot order) and the sorted table rows the batch names (the rows of the
    coalesced sparse gradient: every live index, whether or not it won anything)."""
    table, idx, dout = np.asarray(table, dtype=f32), np.asarray(idx), np.asarray(dout, dtype=f32)
    rows, width = idx.shape
    vocab, dim = table.shape
    ok = live(idx, vocab, pad)
    _, win = bag_encode(table, idx, reduce, pad)
    g = np.zeros((vocab, dim), dtype=f32)
    for r in range(rows):
        n = int(ok[r].sum())
        for w in range(width):
            if not ok[r, w]:
                continue
            if reduce == SUM:
                c = dout[r]
            elif reduce == MEAN_WIDTH:
                c = dout[r] / f32(width)
            elif reduce == MEAN_COUNT:
                c = dout[r] / f32(n)
            else:
                c = np.where(win[r] == w, dout[r], f32(0))
            g[idx[r, w]] = g[idx[r, w]] + c
    return g, np.unique(idx[ok])


def adam_dense(p, m, v, g, lr, t):
    """torch.optim.Adam defaults over the whole table, in place (oracle.aae_oracle.Adam's operation order)."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    m += f32(1 - b1) * (g - m)
    v *= f32(b2)
    v += (f32(1 - b2) * g) * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p += (f32(-(lr / bc1)) * m) / (np.sqrt(v) / f32(bc2 ** 0.5) + f32(eps))


def adam_sparse(p, m, v, rows, g, lr, t):
    """torch.optim.SparseAdam defaults on the rows `rows` with gradients g[rows], in place (oracle.aae_oracle.SparseAdam)."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    if len(rows) == 0:
        return
    gr, m_old, v_old = g[rows], m[rows], v[rows]
    mu = ((gr - m_old) * f32(1 - b1)).astype(f32)
    vu = ((gr * gr - v_old) * f32(1 - b2)).astype(f32)
    m[rows], v[rows] = m_old + mu, v_old + vu
    step_size = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    p[rows] += f32(-step_size) * ((mu + m_old) / (np.sqrt(vu + v_old) + f32(eps)))


def bag_step(table, m, v, idx, reduce, pad, dout, lr, t, sparse):
    """encode + backward + optimiser step t (1-based) in place; returns the encoded block."""
    out, _ = bag_encode(table, idx, reduce, pad)
    g, rows = bag_grad(table, idx, reduce, pad, dout)
    if sparse:
        adam_sparse(table, m, v, rows, g, lr, t)
    else:
        adam_dense(table, m, v, g, lr, t)
    return out


# ---- torch: the definition ------------------------------------------------------------------------------------------------
def torch_exists(reduce, sparse):
    """nn.EmbeddingBag(mode='max') has no sparse gradient: that one combination exists in the kernels only."""
    return not (reduce == MAX and sparse)


def torch_steps(table, idx_steps, reduce, pad, dout_steps, lr, sparse):
    """The same steps in torch on the CPU: nn.Embedding(padding_idx=pad) + .mean(1) / .max(1)[0] for MEAN_WIDTH / MAX_PAD0
    (CategoricalCondition's forms), nn.EmbeddingBag(mode=..., padding_idx=pad or None) for the others, under torch.optim.Adam /
    SparseAdam.  Returns (encoded blocks, table, exp_avg, exp_avg_sq)."""
    import torch
    import torch.nn as nn
    vocab, dim = table.shape
    if reduce in (MEAN_WIDTH, MAX_PAD0):
        assert pad >= 0 and not np.asarray(table)[pad].any(), "nn.Embedding reads its padding row: it must hold zeros"
        mod = nn.Embedding(vocab, dim, padding_idx=pad, sparse=sparse)
        fwd = (lambda i: mod(i).mean(1)) if reduce == MEAN_WIDTH else (lambda i: mod(i).max(1)[0])
    else:
        mod = nn.EmbeddingBag(vocab, dim, mode={SUM: "sum", MEAN_COUNT: "mean", MAX: "max"}[reduce],
                              padding_idx=None if pad < 0 else pad, sparse=sparse)
        fwd = mod
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(np.asarray(table, dtype=f32)))
    opt = (torch.optim.SparseAdam if sparse else torch.optim.Adam)(mod.parameters(), lr=lr)
    outs = []
    for idx, dout in zip(idx_steps, dout_steps):
        opt.zero_grad()
        out = fwd(torch.from_numpy(np.asarray(idx, dtype=np.int64)))
        out.backward(torch.from_numpy(np.asarray(dout, dtype=f32)))
        opt.step()
        outs.append(out.detach().numpy().copy())
    st = opt.state[mod.weight]
    zeros = np.zeros((vocab, dim), dtype=f32)
    return (outs, mod.weight.detach().numpy().copy(), st["exp_avg"].numpy().copy() if "exp_avg" in st else zeros,
            st["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in st else zeros)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def grid(rng, shape):
    """Multiples of 1/8 within [-4, 4]: every sum of a few of them is exact in float32, so summation order cannot matter."""
    return (rng.integers(-32, 33, size=shape) / 8.0).astype(f32)


def no_cross_ties(table, idx, reduce, pad):
    """True when no two DIFFERENT table rows (a padding slot of MAX_PAD0 counting as a row of its own, of value 0) tie in any
    column of any bag.  Repeats of one row in a bag tie with themselves: harmless (the first slot wins, and every slot of
    the bag feeds the same table row), and kept."""
    table, idx = np.asarray(table), np.asarray(idx)
    ok = live(idx, table.shape[0], pad)
    for r in range(idx.shape[0]):
        cand = {int(j): table[j] for j in idx[r][ok[r]]}
        if reduce == MAX_PAD0 and not ok[r].all():
            cand[-1] = np.zeros(table.shape[1], dtype=f32)
        if len(cand) > 1 and (np.diff(np.sort(np.stack(list(cand.values())), axis=0), axis=0) == 0).any():
            return False
    return True


def make_table(rng, vocab, dim, pad):
    """[vocab, dim] on the 1/8 grid; within a column every row holds a different non-zero value (vocab <= 64), so bags never tie
    across rows - a padding row (MAX_PAD0's zero candidate) holds zeros."""
    assert vocab <= 64
    values = np.concatenate([np.arange(-32, 0), np.arange(1, 33)]) / 8.0
    table = np.stack([rng.permutation(values)[:vocab] for _ in range(dim)], axis=1).astype(f32)
    if pad >= 0:
        table[pad] = 0
    return table


def make_idx(rng, rows, width, vocab, pad):
    """[rows, width] indices: random, then - where the shape has room - a row repeating one index, an all-padding row, a row
    padded behind its first entry, and one table row named by every bag (the ownership path: many slots of different rows)."""
    idx = rng.integers(0, vocab, size=(rows, width)).astype(np.int64)
    hot = int(rng.integers(0, vocab))
    if pad >= 0 and hot == pad:
        hot = (hot + 1) % vocab
    idx[:, int(rng.integers(0, width))] = np.where(rng.random(rows) < 0.6, hot, idx[:, 0])
    if rows >= 3:
        idx[1, :] = idx[1, 0] if idx[1, 0] != pad else hot          # the same row in every slot of the bag
        if pad >= 0:
            idx[2, :] = pad                                            # an empty bag
    if rows >= 5 and pad >= 0:
        idx[4, 1:] = pad                                               # shorter than the padded width
    return idx


def settle_mean_gradients(idx, dout, vocab, pad, reduce):
    """dout with no gradient element of a named table row near Adam's eps.  Sums of grid values are exact, so a gradient that
    cancels is exactly 0 in any arithmetic - except behind a mean, whose division by 3 or 5 rounds: contributions that cancel
    in exact arithmetic then leave a residue of a few 1e-9 that depends on how the division is written (torch multiplies by a
    reciprocal), and Adam's m / (sqrt(v) + 1e-8) turns that residue into a step of up to lr.  Such an element pins a rounding,
    not the reduction: where the exact (float64) gradient of a named row is below 1/64, one contributing dout entry moves by
    a grid step, until none is left."""
    if reduce not in (MEAN_WIDTH, MEAN_COUNT):
        return dout
    idx, dout = np.asarray(idx), np.asarray(dout, dtype=f32).copy()
    ok = live(idx, vocab, pad)
    div = np.maximum(ok.sum(1), 1) if reduce == MEAN_COUNT else np.full(len(idx), idx.shape[1])
    slots = np.argwhere(ok)
    first_bag = {}
    for r, w in slots:
        first_bag.setdefault(int(idx[r, w]), int(r))
    for _ in range(400):
        g = np.zeros((vocab, dout.shape[1]))
        np.add.at(g, idx[ok], (dout.astype(np.float64) / div[:, None])[slots[:, 0]])
        named = np.zeros(vocab, dtype=bool)
        named[idx[ok]] = True
        bad = np.argwhere(named[:, None] & (np.abs(g) < 1 / 64))
        if not len(bad):
            return dout
        for j, d in bad:
            r = first_bag[int(j)]
            dout[r, d] = dout[r, d] + f32(0.125) if dout[r, d] < 4 else f32(-4)
    raise AssertionError("the mean gradients did not settle")


def make_case(seed, rows, width, dim, vocab, reduce, pad):
    rng = np.random.default_rng(seed)
    for _ in range(100):
        table, idx = make_table(rng, vocab, dim, pad), make_idx(rng, rows, width, vocab, pad)
        if reduce < MAX_PAD0 or no_cross_ties(table, idx, reduce, pad):
            dout = settle_mean_gradients(idx, grid(rng, (rows, dim)), vocab, pad, reduce)
            return dict(table=table, idx=idx, dout=dout, reduce=reduce, pad=pad)
    raise AssertionError("no tie-free inputs in 100 draws")


# rows x width x dim x vocab: every value of the issue's lists, odd sizes, more than one block of 4 slots, dim beyond one lane
# group (65) and at the limit (256), the bag of one entry (width 1)
SHAPES = [(1, 1, 1, 2), (1, 2, 7, 2), (3, 1, 64, 40), (3, 5, 65, 40), (65, 2, 7, 40), (65, 5, 256, 40), (3, 2, 256, 2),
          (65, 1, 65, 2), (65, 5, 64, 2), (1, 5, 1, 40)]
# reduction -> padding rows to run it with (-1: none); CategoricalCondition's two forms have their padding at 0 only
PADS = {SUM: (-1, 0, 1), MEAN_WIDTH: (0,), MEAN_COUNT: (-1, 0, 1), MAX_PAD0: (0,), MAX: (-1, 0, 1)}


# ---- the reference's recorded runs on the oracle --------------------------------------------------------------------------------
class BagEmbedding:
    """Stand-in of a trainable bag condition for oracle.aae_oracle's models (the protocol of its CategoricalEmbedding): the
    restatement above behind the code.  reduce / pad / sparse as in aae_bag_*."""

    def __init__(self, weight, lr, reduce, pad, sparse):
        self.params = {"w": np.asarray(weight, dtype=f32).copy()}
        self.m, self.v, self.t = np.zeros_like(self.params["w"]), np.zeros_like(self.params["w"]), 0
        self.lr, self.reduce, self.pad, self.sparse = float(lr), reduce, pad, sparse
        self.inc = self.params["w"].shape[1]

    def fwd(self, z, idx, train=True):
        self._c, self._idx = z.shape[1], np.asarray(idx)
        return np.concatenate([z, bag_encode(self.params["w"], self._idx, self.reduce, self.pad)[0]], axis=1)

    def bwd(self, dz):
        self._g, self._rows = bag_grad(self.params["w"], self._idx, self.reduce, self.pad, dz[:, self._c:self._c + self.inc])
        return dz[:, :self._c]

    def step(self):
        self.t += 1
        if self.sparse:
            adam_sparse(self.params["w"], self.m, self.v, self._rows, self._g, self.lr, self.t)
        else:
            adam_dense(self.params["w"], self.m, self.v, self._g, self.lr, self.t)


def fixture_kind(fx):
    """(reduce, pad, sparse, lr) of a recorded run's condition, from its config."""
    if "bag" in fx.cfg:
        b = fx.cfg["bag"]
        return BAG_MODES[b["mode"]], -1, False, b["lr"]
    k = fx.cfg["cat"]
    assert k["reduce"] == "max"
    return MAX_PAD0, 0, k["sparse"], k["lr"]


def build_oracle(fx):
    from oracle import aae_oracle as O
    reduce, pad, sparse, lr = fixture_kind(fx)
    cond = BagEmbedding(fx.z["init.cond.embedding"], lr, reduce, pad, sparse)
    if fx.cfg.get("vae"):
        params = {f"{n}.{t}": fx.z[f"init.{n}.{t}"] for n in ("fc1", "fc21", "fc22", "fc3", "fc4") for t in ("weight", "bias")}
        return O.OracleVAE(params, lr=fx.cfg["gen_lr"], conditions=[cond])
    return O.OracleAAE(fx.init_params(), conditions=[cond], **fx.model_kwargs())
