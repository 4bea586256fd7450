"""IRGAN on the device (the reference's irgan/cf_gan.py with gen_model.py and dis_model.py), and its restatement in NumPy.

Two matrix-factorisation nets, the generator G and the discriminator D, each `user_emb [users, d]`, `item_emb [items, d]`,
`item_bias [items]` under torch.optim.SGD(lr, momentum=0.9) whose gradients are DENSE: every element of all three tensors moves
on every step (buf = 0.9 buf + grad; p -= lr buf).  logit(u, j) = user_emb[u] . item_emb[j] + item_bias[j].

  generate_for_d  (every fifth D epoch) per user with positives, in dict order: |pos| negatives, with replacement, from
                  softmax(G logit / 0.2) over all items -> the lines (u, pos[i], neg[i]).
  D step          batch_size consecutive lines (the last batch of an epoch is shorter), each the triples (u, pos, 1), (u, neg, 0):
                  loss = mean BCE-with-logits + lambda_D (mean(user_emb^2) + mean(item_emb^2) + mean(item_bias^2)),
                  lambda_D = 0.1 / batch_size; one momentum step on D.
  G step          per user with positives: p = softmax(G logit); 2 |pos| samples s from pn = 0.8 p + 0.2 / |pos| on the positives;
                  reward_s = 2 (sigmoid(D logit(u, s)) - 1/2) p_s / pn_s; loss = -mean(log(max(p_s, 1e-8)) reward_s); one momentum
                  step on G.  d loss / d logit_j = p_j R - sum_{s = j} reward_s / n with R = sum_{s: p_s >= 1e-8} reward_s / n,
                  n = 2 |pos|; a sample under the clamp contributes nothing.
  fit             n_epochs x (d_epochs D epochs, then g_epochs G epochs).
  predict(X)      for every key u of the dict the G logits of user u with the TRAINING positives of u set to 0 (not -inf: the
                  reference writes the other items into a row of zeros); a user absent from the training dict has nothing zeroed.

Where this departs from the reference, on purpose: `conditions` raises NotImplementedError (the reference's conditioned variant
sends the code through an nn.Linear its optimiser never sees, hard-codes view(-1, 5) and never steps the conditions); predict
without conditions works (the reference dies on an unbound c_batch) and computes what all_rating followed by simple_test_one_user
compute; users without positives are skipped in both phases (the reference emits no lines for them and divides by zero in the G
phase); a repeated item of a user counts once; pn is not renormalised (its sum is 1 up to rounding) on either route; there is no
dis-train.txt - the lines live in a buffer, and every D epoch reads the lines generate_for_d last wrote (the reference reads
them through linecache, which keeps serving the FIRST file a process wrote; tools/gen_golden.py gen_irgan clears that cache).

Routes.  `route()` says "device" or None.  The device route (csrc/irgan.h through _hip.irgan_*) needs a device, emb_dim in
[1, 64], batch_size <= 1024 lines and at most 2048 positives per user; everything else, and device=None, runs the host route:
the same steps in NumPy, float32 by default or float64 (`host_dtype`).  Both take their draws from `draws`:
  "device"  the library's keyed generator (csrc/device_common.h rng_key / hash_cell; streams 16 and 17), restated here as
            `draw_negatives` / `draw_samples`: keyed by (seed, draw counter, user, sample index), so a seed gives the same lines
            however the users are chunked.  The sampler is a two-level inverse CDF in float64 over tiles of 128 items (csrc/irgan.h
            states it; `softmax_tables` / `pick` are the same arithmetic), the G mixture taken literally: one word decides
            "uniform positive" (0.2) or "from p".
  "numpy"   the reference's np.random.choice calls in the reference's order (probabilities come to the host: slow, for A/B runs).
`fit(X, draws=...)` takes recorded draws instead (tests/golden/irgan_*.npz), in the reference's order.
"""
import os

import numpy as np
import scipy.sparse as sp
import torch

from . import _hip, ranking
from .base import Recommender

KEYS = _hip.IRGAN_KEYS
TILE = _hip.IRGAN_TILE
TEMPERATURE = 0.2            # generate_for_d
SAMPLE_LAMBDA = 0.2          # the weight of the uniform part of pn
CLAMP = 1e-8
MOMENTUM = 0.9
SID_NEG, SID_G = 16, 17
MIX_THRESHOLD = 858993459    # floor(0.2 * 2^32)
_M64 = (1 << 64) - 1


# ---- the keyed generator and the sampler (csrc/irgan.h SAMPLER) -----------------------------------------------------------------
def _key(seed, draw, sid):
    return ((int(seed) & _M64) ^ ((int(draw) * 0xD1B54A32D192ED03) & _M64) ^ ((sid * 0xA0761D6478BD642F) & _M64)) & _M64


def _words(key, row, cols):
    """hash_cell(key, row, cols): uint32 per entry of cols."""
    lo, hi = np.uint32(key & 0xFFFFFFFF), np.uint32(key >> 32)
    r = np.uint32(int(row) & 0xFFFFFFFF)
    c = (np.asarray(cols, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = (lo + r * np.uint32(0x9E3779B1)) ^ (hi + c * np.uint32(0x85EBCA77))
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def logits_f32(user_row, item_emb, item_bias):
    """The device's logits of one user: acc = bias, then acc = fmaf(u[d], v[d], acc) for d ascending, in float32 (the product
    of two float32 is exact in float64, so one rounding per term - fmaf's)."""
    acc = np.asarray(item_bias, dtype=np.float32).copy()
    u, V = np.asarray(user_row, dtype=np.float32), np.asarray(item_emb, dtype=np.float32)
    for d in range(V.shape[1]):
        acc = (acc.astype(np.float64) + np.float64(u[d]) * V[:, d].astype(np.float64)).astype(np.float32)
    return acc


def softmax_tables(x, e=None, m=None):
    """The softmax tables of one user over tiles of TILE items from x = logit * inv_temp (float32): per tile m_t = max, e_j =
    exp(x_j - m_t) in float32, s_t = sum of e in float64; M = max m_t, W_t = s_t exp(m_t - M), cum = the prefix sums of W,
    Z = cum[-1].  e, m: tables to rebuild from instead (perturbed weights)."""
    n = tiles = None
    if e is None:
        x = np.asarray(x, dtype=np.float32)
        n = x.size
        tiles = (n + TILE - 1) // TILE
        xp = np.full(tiles * TILE, -np.inf, dtype=np.float32)
        xp[:n] = x
        xp = xp.reshape(tiles, TILE)
        m = xp.max(axis=1)
        with np.errstate(invalid="ignore"):
            e = np.exp(xp - m[:, None]).astype(np.float32)
    M = np.float64(m.max())
    scale = np.exp(m.astype(np.float64) - M)
    W = e.astype(np.float64).sum(axis=1) * scale
    cum = np.cumsum(W)
    return dict(n=n, tiles=tiles, m=m, e=e, M=M, scale=scale, cum=cum, Z=cum[-1])


def pick(tab, x):
    """Items of the uniforms x in [0, 1): the two-level inverse CDF."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    target = x * tab["Z"]
    t = np.minimum(np.searchsorted(tab["cum"], target, side="right"), tab["tiles"] - 1)
    prev = np.where(t > 0, tab["cum"][np.maximum(t - 1, 0)], 0.0)
    w = tab["e"][t].astype(np.float64) * tab["scale"][t][:, None]
    acc = np.cumsum(np.concatenate([prev[:, None], w], axis=1), axis=1)[:, 1:]
    over = acc > target[:, None]
    last = np.minimum(TILE, tab["n"] - t * TILE) - 1
    idx = np.where(over.any(axis=1), over.argmax(axis=1), last)
    return (t * TILE + np.minimum(idx, last)).astype(np.int64)


def _pick_flagged(tab, x):
    """(items, boundary): a draw is boundary when moving its uniform by 2^-20 or the item weights by 4 units in the last place
    (alternating signs, both ways) changes the item."""
    items = pick(tab, x)
    flag = np.zeros(items.shape, dtype=bool)
    for dx in (-2.0 ** -20, 2.0 ** -20):
        flag |= pick(tab, np.clip(x + dx, 0.0, np.nextafter(1.0, 0.0))) != items
    sign = np.where(np.arange(TILE) % 2 == 0, 1.0, -1.0)
    for s in (1.0, -1.0):
        e = (tab["e"].astype(np.float64) * (1.0 + s * sign * 4 * 2.0 ** -23)).astype(np.float32)
        flag |= pick(softmax_tables(None, e=e, m=tab["m"]) | dict(n=tab["n"], tiles=tab["tiles"]), x) != items
    return items, flag


def _uniform(words):
    return (words.astype(np.float64) + 0.5) * 2.0 ** -32


def draw_negatives(seed, draw, user, n, logits, temperature=TEMPERATURE, flags=False):
    """The n negatives generate_for_d draws for `user` from softmax(logits / temperature): stream 16, word 2 i + 1 of row `user`
    for sample i.  logits: float32 (logits_f32).  flags: (items, boundary) instead."""
    inv = np.float32(1.0) / np.float32(temperature)
    tab = softmax_tables(np.asarray(logits, dtype=np.float32) * inv)
    x = _uniform(_words(_key(seed, draw, SID_NEG), user, 2 * np.arange(n, dtype=np.int64) + 1))
    return _pick_flagged(tab, x) if flags else pick(tab, x)


def draw_samples(seed, draw, user, pos, logits, flags=False):
    """The 2 |pos| samples of a G step of `user` (pos: the ascending positives) from 0.8 softmax(logits) + 0.2 uniform(pos):
    stream 17; word 2 i decides - below MIX_THRESHOLD the positive pos[(w1 |pos|) >> 32] - and word 2 i + 1 = w1 picks."""
    pos = np.asarray(pos, dtype=np.int64)
    n = 2 * pos.size
    key = _key(seed, draw, SID_G)
    i = np.arange(n, dtype=np.int64)
    w0, w1 = _words(key, user, 2 * i), _words(key, user, 2 * i + 1)
    tab = softmax_tables(np.asarray(logits, dtype=np.float32))
    x = _uniform(w1)
    from_p, flag = _pick_flagged(tab, x) if flags else (pick(tab, x), None)
    mix = w0 < np.uint32(MIX_THRESHOLD)
    items = np.where(mix, pos[(w1.astype(np.uint64) * np.uint64(pos.size)) >> np.uint64(32)], from_p)
    return (items, flag & ~mix) if flags else items


# ---- the host route --------------------------------------------------------------------------------------------------------
def new_net(users, items, dim, init_delta=0.05, param=None, rng=None, dtype=np.float32):
    """A net as a dict of the six arrays KEYS: uniform(-init_delta, init_delta) embeddings and a zero bias, or the triple
    `param`; zero momentum."""
    if param is not None:
        u, v, b = (np.array(p, dtype=dtype) for p in param)
    else:
        rng = rng or np.random
        u = rng.uniform(-init_delta, init_delta, size=(users, dim)).astype(dtype)
        v = rng.uniform(-init_delta, init_delta, size=(items, dim)).astype(dtype)
        b = np.zeros(items, dtype=dtype)
    if u.shape != (users, dim) or v.shape != (items, dim) or b.shape != (items,):
        raise ValueError("gen_param does not have the shapes ({0}, {2}), ({1}, {2}), ({1},)".format(users, items, dim))
    return dict(user_emb=u, item_emb=v, item_bias=b, m_user_emb=np.zeros_like(u), m_item_emb=np.zeros_like(v),
                m_item_bias=np.zeros_like(b))


def cast_net(net, dtype):
    return {k: np.array(net[k], dtype=dtype) for k in KEYS}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _momentum_step(net, grads, lr, momentum):
    dt = net["user_emb"].dtype.type
    for k, g in zip(KEYS[:3], grads):
        buf = net["m_" + k]
        buf *= dt(momentum)
        buf += g.astype(buf.dtype, copy=False)
        net[k] -= dt(lr) * buf


def host_d_step(net, lines, lr, momentum, lam):
    """One D step over the int lines [L, 3] = (user, positive, negative), in the dtype of the net.  The loss."""
    U, V, b = net["user_emb"], net["item_emb"], net["item_bias"]
    dt = U.dtype.type
    lines = np.asarray(lines, dtype=np.int64).reshape(-1, 3)
    n = 2 * lines.shape[0]
    u, it = np.repeat(lines[:, 0], 2), lines[:, 1:3].reshape(-1)
    y = np.tile(np.asarray([1, 0], dtype=U.dtype), lines.shape[0])
    x = (U[u] * V[it]).sum(axis=1) + b[it]
    g = ((_sigmoid(x) - y) / dt(n)).astype(U.dtype)
    bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
    loss = bce.mean(dtype=np.float64) + lam * ((U.astype(np.float64) ** 2).mean() + (V.astype(np.float64) ** 2).mean() +
                                               (b.astype(np.float64) ** 2).mean())
    gU, gV, gb = np.zeros_like(U), np.zeros_like(V), np.zeros_like(b)
    np.add.at(gU, u, g[:, None] * V[it])
    np.add.at(gV, it, g[:, None] * U[u])
    np.add.at(gb, it, g)
    gU += dt(2.0 * lam / U.size) * U
    gV += dt(2.0 * lam / V.size) * V
    gb += dt(2.0 * lam / b.size) * b
    _momentum_step(net, (gU, gV, gb), lr, momentum)
    return float(loss)


def host_d_steps(net, lines, batch_size, lr, momentum, lam, n_steps=None):
    """The D steps of one epoch over `lines` (or its first n_steps batches).  The losses."""
    lines = np.asarray(lines).reshape(-1, 3)
    total = (lines.shape[0] + batch_size - 1) // batch_size
    return [host_d_step(net, lines[s * batch_size:(s + 1) * batch_size], lr, momentum, lam)
            for s in range(total if n_steps is None else n_steps)]


def host_g_step(G, D, user, pos, samples, lr, momentum):
    """One G step of `user` with the given samples, in the dtype of G.  The loss."""
    U, V, b = G["user_emb"], G["item_emb"], G["item_bias"]
    dt = U.dtype.type
    samples = np.asarray(samples, dtype=np.int64)
    n, npos = samples.size, len(pos)
    logits = V @ U[user] + b
    e = np.exp(logits - logits.max())
    p = e / e.sum()
    ps = p[samples]
    pn = dt(1.0 - SAMPLE_LAMBDA) * ps + np.where(np.isin(samples, pos), dt(SAMPLE_LAMBDA) / dt(npos), dt(0))
    dl = (D["user_emb"][user] * D["item_emb"][samples]).sum(axis=1) + D["item_bias"][samples]
    reward = (dt(2) * (_sigmoid(dl.astype(U.dtype)) - dt(0.5)) * ps / pn).astype(U.dtype)
    loss = -np.mean(np.log(np.maximum(ps, dt(CLAMP))) * reward, dtype=np.float64)
    c = np.where(ps >= dt(CLAMP), reward / dt(n), dt(0)).astype(U.dtype)
    gl = p * c.sum()
    np.subtract.at(gl, samples, c)
    gU = np.zeros_like(U)
    gU[user] = gl @ V
    _momentum_step(G, (gU, np.outer(gl, U[user]), gl), lr, momentum)
    return float(loss)


def host_scores(G, users, pos_of):
    """float [len(users), items]: the G logits of `users`, 0 at the training positives pos_of(u) of each."""
    out = G["user_emb"][np.asarray(users, dtype=np.int64)] @ G["item_emb"].T + G["item_bias"]
    for r, u in enumerate(users):
        out[r, pos_of(u)] = 0
    return out


def _scaled(s, best):
    span = s.max() - s.min()
    return (s[best] - s.min()) / (span if span > 0 else 1.0)


class _HostEngine:
    def __init__(self, G, D, dtype):
        self.G, self.D = cast_net(G, dtype), cast_net(D, dtype)

    def nets(self):
        return self.G, self.D

    def logits(self, user):
        return logits_f32(self.G["user_emb"][user], self.G["item_emb"], self.G["item_bias"])

    def plain_logits(self, user):
        return np.asarray(self.G["item_emb"] @ self.G["user_emb"][user] + self.G["item_bias"], dtype=np.float32)

    def sample_neg(self, m, seed, draw):
        for q, u in enumerate(m._order):
            lo, hi = m._line_off[q], m._line_off[q + 1]
            m._lines[lo:hi, 2] = draw_negatives(seed, draw, u, hi - lo, self.logits(u))

    def set_lines(self, lines):
        self.lines = np.array(lines, dtype=np.int64)

    def d_epoch(self, m, want_loss):
        return host_d_steps(self.D, self.lines, m.batch_size, m.lr, MOMENTUM, m.lam_d)[-1]

    def g_steps(self, m, users, samples, seed, draw, want_loss):
        loss = None
        for i, u in enumerate(users):
            s = samples[i] if samples is not None else draw_samples(seed, draw, u, m._pos[u], self.logits(u))
            loss = host_g_step(self.G, self.D, u, m._pos[u], s, m.lr, MOMENTUM)
        return loss

    def scores(self, m, users):
        return host_scores(self.G, users, m._pos_of)


class _DeviceEngine:
    def __init__(self, G, D, device, m):
        self.device = torch.device(device)
        self.G, self.D = _hip.DeviceIrganNet(G, device), _hip.DeviceIrganNet(D, device)
        tiles = (self.G.items + TILE - 1) // TILE
        slots = max(1, min(len(m._order), (64 << 20) // (tiles * (24 + 4 * TILE))))
        self.scratch = _hip.irgan_scratch(self.G, slots)
        up = lambda a, dt: _hip.upload(np.ascontiguousarray(a, dtype=dt), self.device)      # noqa: E731
        self.pos = (up(m._pos_indptr, np.int64), up(m._pos_sorted, np.int32))
        self.order = up(np.asarray(m._order), np.int32)
        self.line_off = up(m._line_off, np.int64)
        self.lines = up(m._lines, np.int32)
        self.max_pos = int(np.diff(m._pos_indptr).max()) if len(m._order) else 0

    def nets(self):
        return self.G.arrays(), self.D.arrays()

    def plain_logits(self, user):
        return _hip.irgan_scores(self.G, _hip.upload(np.asarray([user], dtype=np.int32), self.device))[0].cpu().numpy()

    def sample_neg(self, m, seed, draw):
        _hip.irgan_sample_neg(self.G, self.order, self.line_off, self.max_pos, TEMPERATURE, seed, draw, self.lines, self.scratch)

    def set_lines(self, lines):
        self.lines = _hip.upload(np.ascontiguousarray(lines, dtype=np.int32), self.device)

    def d_epoch(self, m, want_loss):
        n = int(self.lines.shape[0])
        out = _hip.irgan_d_steps(self.D, self.lines, m.batch_size, (n + m.batch_size - 1) // m.batch_size, m.lr, MOMENTUM, m.lam_d,
                                 self.scratch, losses=want_loss)
        return float(out[-1]) if want_loss and n else None

    def g_steps(self, m, users, samples, seed, draw, want_loss):
        if not len(users):
            return None
        ud = _hip.upload(np.asarray(users, dtype=np.int32), self.device)
        sd = od = None
        if samples is not None:
            sd = _hip.upload(np.concatenate([np.asarray(s, dtype=np.int32) for s in samples]), self.device)
            od = _hip.upload(np.concatenate(([0], np.cumsum([len(s) for s in samples]))).astype(np.int64), self.device)
        out = _hip.irgan_g_steps(self.G, self.D, ud, self.pos, self.max_pos, m.lr, MOMENTUM, self.scratch, samples=sd, sample_off=od,
                                 seed=seed or 0, draw=draw, losses=want_loss)
        return float(out[-1]) if want_loss else None


class IRGAN(ranking.ScratchRanker):
    """The reference's IRGAN (cf_gan.py:26-238) with its arguments, and: device ("cuda:0"; None: the host route), seed (the
    initial parameters and, with draws="device", every draw; None: one is drawn and stored when draws="device"), draws ("device" /
    "numpy": the module docstring), host_dtype (of the host route), scratch_bytes (the [rows, items] scratch of a ranking call)."""

    DRAWS = ("device", "numpy")

    def __init__(self, user_num, item_num, gen_param=None, batch_size=16, emb_dim=5, lr=0.001, init_delta=0.05, g_epochs=50,
                 d_epochs=100, n_epochs=15, conditions=None, verbose=True, device="cuda:0", seed=None, draws="device",
                 host_dtype=np.float32, scratch_bytes=256 << 20):
        if conditions is not None:
            raise NotImplementedError(
                "IRGAN with conditions is not built: the reference's conditioned variant sends the code through an nn.Linear its "
                "optimiser never sees, hard-codes view(-1, 5) and never steps the conditions")
        if draws not in self.DRAWS:
            raise ValueError("draws must be one of {}, not {!r}".format(self.DRAWS, draws))
        if emb_dim < 1 or batch_size < 1:
            raise ValueError("emb_dim and batch_size must be positive")
        self.user_num, self.item_num, self.gen_param = int(user_num), int(item_num), gen_param
        self.batch_size, self.emb_dim, self.lr, self.init_delta = int(batch_size), int(emb_dim), lr, init_delta
        self.g_epochs, self.d_epochs, self.n_epochs = g_epochs, d_epochs, n_epochs
        self.conditions, self.verbose, self.device, self.draws = None, verbose, device, draws
        self.host_dtype, self.scratch_bytes = host_dtype, int(scratch_bytes)
        if seed is None and draws == "device":
            seed = int.from_bytes(os.urandom(8), "little")
        self.seed = seed
        self.lam_d = 0.1 / batch_size
        self.draw = 0                      # the draw counter of the keyed generator: one per generate_for_d and per G epoch
        rng = np.random.RandomState(seed & 0xFFFFFFFF) if seed is not None else None
        self._init = (new_net(user_num, item_num, emb_dim, init_delta, gen_param, rng),
                      new_net(user_num, item_num, emb_dim, init_delta, gen_param, rng))
        self._set_positives({})
        self._engine = None
        self.last_losses = {}

    # ---- routes ------------------------------------------------------------------------------------------------------------
    def route(self):
        """"device" when the kernels run this model, None when the host does."""
        if self.device is None or not torch.cuda.is_available():
            return None
        if not 1 <= self.emb_dim <= _hip.IRGAN_DIM_MAX or self.batch_size > _hip.IRGAN_BATCH_MAX:
            return None
        if len(self._order) and int(np.diff(self._pos_indptr).max()) > _hip.IRGAN_POS_MAX:
            return None
        return "device"

    def _set_positives(self, X):
        self.user_pos_train = X
        self._pos, self._order = {}, []
        for u, items in X.items():
            seen = list(dict.fromkeys(int(i) for i in items))
            if not 0 <= int(u) < self.user_num or any(not 0 <= i < self.item_num for i in seen):
                raise ValueError("user {} or one of its items lies outside the model".format(u))
            if seen:
                self._pos[int(u)] = np.sort(np.asarray(seen, dtype=np.int64))
                self._order.append(int(u))
        counts = np.zeros(self.user_num, dtype=np.int64)
        for u, p in self._pos.items():
            counts[u] = p.size
        self._pos_indptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        self._pos_sorted = np.concatenate([self._pos[u] for u in sorted(self._pos)] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
        # the lines of generate_for_d: (u, pos[i], .) in dict and list order
        rows, off = [], [0]
        for u in self._order:
            seen = list(dict.fromkeys(int(i) for i in X[u]))
            rows += [(u, i, 0) for i in seen]
            off.append(len(rows))
        self._lines = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        self._line_off = np.asarray(off, dtype=np.int64)

    def _pos_of(self, u):
        return self._pos.get(int(u), np.zeros(0, dtype=np.int64))

    def _make_engine(self, G, D):
        if self.route() == "device":
            return _DeviceEngine(G, D, self.device, self)
        return _HostEngine(G, D, self.host_dtype)

    def _nets(self):
        return self._engine.nets() if self._engine is not None else self._init

    # ---- training ----------------------------------------------------------------------------------------------------------
    def fit(self, X, y=None, condition_data=None, draws=None, on_block=None):
        """X: the reference's dict user -> list of items.  draws: recorded draws to replay instead of drawing - an iterable of
        integer arrays in the reference's order (per generate_for_d the negatives of each user, per G epoch the samples of
        each).  on_block(kind, model): called behind every D-epoch block ("d") and G-epoch block ("g")."""
        if y is not None:
            raise NotImplementedError("(Semi-)supervised usage not supported")
        if condition_data is not None:
            raise NotImplementedError("IRGAN with conditions is not built")
        G, D = self._nets()
        self._set_positives(X)
        eng = self._engine = self._make_engine(G, D)
        replay = iter(draws) if draws is not None else None
        want = bool(self.verbose)
        for epoch in range(self.n_epochs):
            if self.verbose:
                print("Epoch", epoch + 1)
            for d_epoch in range(self.d_epochs):
                if d_epoch % 5 == 0:
                    self._generate_for_d(eng, replay)
                loss = eng.d_epoch(self, want or on_block is not None) if self._lines.shape[0] else None
                self.last_losses["d"] = loss
                if self.verbose and loss is not None:
                    print("\r[D Epoch %d/%d] [loss: %f]" % (d_epoch, self.d_epochs, loss))
            if on_block is not None:
                on_block("d", self)
            for g_epoch in range(self.g_epochs):
                loss = self._g_epoch(eng, replay, want or on_block is not None)
                self.last_losses["g"] = loss
                if self.verbose and loss is not None:
                    print("\r[G Epoch %d/%d] [loss: %f]" % (g_epoch, self.g_epochs, loss))
            if on_block is not None:
                on_block("g", self)
        return self

    def _generate_for_d(self, eng, replay):
        if replay is None and self.draws == "device":
            eng.sample_neg(self, self.seed, self.draw)
            self.draw += 1
            if isinstance(eng, _HostEngine):
                eng.set_lines(self._lines)
            return
        for q, u in enumerate(self._order):
            lo, hi = self._line_off[q], self._line_off[q + 1]
            if replay is not None:
                neg = np.asarray(next(replay), dtype=np.int64)
            else:                          # the reference's lines 98-102, on the logits as they stand
                rating = eng.plain_logits(u) / 0.2
                ex = np.exp(rating)
                neg = np.random.choice(np.arange(self.item_num), size=hi - lo, p=ex / np.sum(ex))
            if neg.size != hi - lo:
                raise ValueError("recorded draws do not fit the users' positives")
            self._lines[lo:hi, 2] = neg
        eng.set_lines(self._lines)

    def _g_epoch(self, eng, replay, want_loss):
        if replay is None and self.draws == "device":
            loss = eng.g_steps(self, self._order, None, self.seed, self.draw, want_loss)
            self.draw += 1
            return loss
        loss = None
        for u in self._order:
            pos = self._pos[u]
            if replay is not None:
                s = np.asarray(next(replay), dtype=np.int64)
            else:                          # the reference's lines 178-189
                ex = np.exp(eng.plain_logits(u))
                prob = ex / np.sum(ex)
                pn = (1 - SAMPLE_LAMBDA) * prob
                pn[pos] += SAMPLE_LAMBDA * 1.0 / pos.size
                pn /= pn.sum()
                s = np.random.choice(np.arange(self.item_num), 2 * pos.size, p=pn)
            loss = eng.g_steps(self, [u], [s], None, 0, want_loss)
        return loss

    # ---- state -------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The twelve tensors ("gen." / "dis." + KEYS, momentum included) as float arrays, the seed, the draw counter and the
        training dict."""
        G, D = self._nets()
        out = {"gen." + k: np.array(G[k]) for k in KEYS}
        out.update({"dis." + k: np.array(D[k]) for k in KEYS})
        out["seed"], out["draw"] = self.seed, self.draw
        # the training dict (predict zeroes its items): users in dict order, their items as one CSR
        lists = [list(v) for v in self.user_pos_train.values()]
        out["train_users"] = np.asarray(list(self.user_pos_train.keys()), dtype=np.int64)
        out["train_indptr"] = np.concatenate(([0], np.cumsum([len(v) for v in lists]))).astype(np.int64)
        out["train_items"] = np.asarray([i for v in lists for i in v], dtype=np.int64)
        return out

    def load_state_dict(self, state):
        G = {k: np.asarray(state["gen." + k], dtype=np.float32) for k in KEYS}
        D = {k: np.asarray(state["dis." + k], dtype=np.float32) for k in KEYS}
        for net in (G, D):
            if net["user_emb"].shape != (self.user_num, self.emb_dim) or net["item_emb"].shape != (self.item_num, self.emb_dim):
                raise ValueError("the state does not have this model's shapes")
        self.seed, self.draw = state.get("seed", self.seed), int(state.get("draw", self.draw))
        if "train_users" in state:
            ip, it = np.asarray(state["train_indptr"]), np.asarray(state["train_items"])
            self._set_positives({int(u): it[ip[q]:ip[q + 1]].tolist() for q, u in enumerate(np.asarray(state["train_users"]))})
        self._init = (G, D)
        self._engine = self._make_engine(G, D)
        return self

    # ---- prediction --------------------------------------------------------------------------------------------------------
    def _users_of(self, keys):
        users = np.asarray(list(keys), dtype=np.int64)
        if users.size and (users.min() < 0 or users.max() >= self.user_num):
            raise IndexError("a key of X lies outside [0, user_num)")
        return users

    def _host_scores(self, users):
        G = self._nets()[0]
        return host_scores(cast_net(G, self.host_dtype) if not isinstance(self._engine, _HostEngine) else G, users, self._pos_of)

    def predict(self, X, condition_data=None):
        """float64 [len(X), items]: row by row what the reference's all_rating + simple_test_one_user give for the keys of X."""
        users = self._users_of(X.keys() if hasattr(X, "keys") else X)
        if isinstance(self._engine, _DeviceEngine) and users.size:
            e = self._engine
            return _hip.irgan_scores(e.G, _hip.upload(users.astype(np.int32), e.device), e.pos).cpu().numpy().astype(np.float64)
        return np.asarray(self._host_scores(users), dtype=np.float64).reshape(users.size, self.item_num)

    def _rank_inputs(self, users, known):
        users = self._users_of(users)
        K = sp.csr_matrix(known, dtype=np.float64, copy=True)
        K.sum_duplicates()
        K.sort_indices()
        if K.shape != (users.size, self.item_num):
            raise ValueError("the known items have shape {}, not {}".format(K.shape, (users.size, self.item_num)))
        return users, K

    def _host_rows(self, users, K):
        return ranking.host_rows(K, lambda r0, r1: np.asarray(self._host_scores(users[r0:r1]), dtype=np.float64))

    def _on_device(self, k=None):
        if k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, self.item_num):
            return False
        if self._engine is None and self.route() == "device":
            self._engine = self._make_engine(*self._init)
        return isinstance(self._engine, _DeviceEngine)

    def _buffers(self):
        dev = self._engine.device
        return lambda rows: {"scratch": torch.empty(rows, (self.item_num + 3) & ~3, dtype=torch.float32, device=dev)}

    def predict_topk(self, users, known, k=10, y_true=None, metrics=None):
        """(ids int32 [n, k], scaled scores float32 [n, k]): the k best items of every row - row r scored as user users[r] with
        that user's training positives at 0, the items of row r of the CSR `known` left out; the better score first, the smaller
        id at equal scores, id -1 / score 0 behind a row's last rankable item.  metrics: [(mean, std)] per name instead."""
        users, K = self._rank_inputs(users, known)
        n = users.size
        if k < 1:
            raise ValueError("k must be positive")
        if not (self._on_device(k) and n):
            return ranking.host_finish_lists(ranking.host_topk(self._host_rows(users, K), n, k, _scaled), metrics, y_true, K.shape)
        e = self._engine
        ud, kd = _hip.upload(users.astype(np.int32), e.device), _hip.DeviceCSR(K, e.device)
        parts = self._device_chunks(n, self.item_num, self._buffers(),
                                    lambda s0, rows, **b: _hip.irgan_topk(e.G, ud[s0:s0 + rows], e.pos, kd, s0, rows, k, **b))
        return ranking.finish_lists(parts, k, metrics, y_true, K.shape)

    def predict_ranks(self, users, known, y_true, metrics=None):
        """CSR of int32 with y_true's canonical pattern: the 1-based rank of every held-out item in the full ranking of its row,
        in predict_topk's ordering.  metrics: [(mean, std)] per name instead."""
        users, K = self._rank_inputs(users, known)
        n = users.size
        Ys = ranking.canonical_truth(y_true, K.shape, "the known items")
        if not (self._on_device() and n):
            return ranking.host_finish_ranks(ranking.host_ranks(self._host_rows(users, K), Ys), metrics)
        e = self._engine
        ud, kd, td = _hip.upload(users.astype(np.int32), e.device), _hip.DeviceCSR(K, e.device), _hip.DeviceCSR(Ys, e.device)
        return ranking.finish_ranks(self._device_chunks(
            n, self.item_num, self._buffers(),
            lambda s0, rows, **b: _hip.irgan_ranks(e.G, ud[s0:s0 + rows], e.pos, kd, s0, rows, td,
                                                   int(Ys.indptr[s0 + rows] - Ys.indptr[s0]), **b)), Ys, metrics)


class IRGANRecommender(Recommender):
    """The reference's IRGANRecommender (cf_gan.py:241-315): train / predict / __str__, the keyword arguments handed to IRGAN;
    test row t is scored as user t, as the reference's driver has it.  predict_topk / predict_ranks rank on the device."""

    def __init__(self, user_num, item_num, gen_param=None, conditions=None, **kwargs):
        super().__init__()
        if conditions is not None:
            raise NotImplementedError("IRGAN with conditions is not built (aaerec/irgan.py says why)")
        self.verbose = kwargs.get("verbose", True)
        self.conditions = conditions
        self.model_params = kwargs
        self.gen_param = gen_param
        self.user_num = user_num
        self.item_num = item_num
        self.model = None

    def __str__(self):
        desc = "IRGAN"
        if self.conditions:
            desc += " conditioned on: " + ", ".join(self.conditions.keys())
        desc += "\nModel Params: " + str(self.model_params)
        return desc

    def route(self):
        return self.model.route() if self.model is not None else IRGAN(self.user_num, self.item_num, **self.model_params).route()

    def train(self, training_set):
        self.model = IRGAN(self.user_num, self.item_num, self.gen_param, conditions=self.conditions, **self.model_params)
        if self.verbose:
            print(self)
        self.model.fit(training_set.to_dict())

    def predict(self, test_set):
        return self.model.predict(test_set.to_dict())

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None):
        X = test_set.tocsr()
        return self.model.predict_topk(np.arange(X.shape[0]), X, k=k, y_true=y_true, metrics=metrics)

    def predict_ranks(self, test_set, y_true, metrics=None):
        X = test_set.tocsr()
        return self.model.predict_ranks(np.arange(X.shape[0]), X, y_true, metrics=metrics)
