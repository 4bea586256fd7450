"""Shared by tests/test_irgan_cpu.py and tests/test_irgan_gpu.py: the fixtures recorded from the real reference
(tests/golden/irgan_*.npz, tools/gen_golden.py gen_irgan), random nets, and the sampler cases.

TOLERANCES.  Parameters and momentum against the fixtures: 1e-5 absolute (the project's parameter tolerance), losses 2e-6
relative + 1e-7 (tests/test_oracle_golden.py).  Device steps against the float64 host route: 4 x the float32 host route's own
distance from the float64 one on the same case, floored at 1e-6.

SAMPLER CASES.  A draw of the restatement is "boundary" when moving its uniform by 2^-20 or the item weights by 4 units in the
last place changes the item (aaerec.irgan._pick_flagged).  Over N items there are N - 1 boundaries in [0, 1), so about 2 N 2^-20
of the draws from p are boundary - 0.07 % at the largest case here, 385 items; the cap of the CPU test is a quarter of 1 %, that
of the device comparison 1 %.  Every case draws some 4 600 times (24 users x 64 positives: 1 536 negatives, 3 072 samples), so
that the cap is tens of draws and not one."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["irgan_small", "irgan_dup"]
TOL_PARAM, TOL_LOSS_R, TOL_LOSS_A = 1e-5, 2e-6, 1e-7
TILE = 128           # csrc/irgan.h kIrTile: items of a workgroup's tile, in the update kernels and in the sampler


class Fixture:
    def __init__(self, name):
        self.z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.cfg = json.loads(str(self.z["cfg"]))
        ip, it = self.z["pos_indptr"], self.z["pos_items"]
        self.X = {u: it[ip[u]:ip[u + 1]].tolist() for u in range(self.cfg["users"])}
        dp = self.z["draw_indptr"]
        self.draws = [self.z["draws"][dp[i]:dp[i + 1]] for i in range(len(dp) - 1)]

    def state(self, prefix):
        """The twelve tensors recorded at `prefix` ("init", "block<b>") under the keys of IRGAN.state_dict()."""
        from aaerec.irgan import KEYS
        return {pre + k: self.z["%s.%s.%s" % (prefix, tag, k)] for tag, pre in (("g", "gen."), ("d", "dis.")) for k in KEYS}

    def model(self, **kw):
        from aaerec.irgan import IRGAN
        c = self.cfg
        m = IRGAN(c["users"], c["items"], batch_size=c["batch_size"], emb_dim=c["emb_dim"], lr=c["lr"], n_epochs=c["n_epochs"],
                  d_epochs=c["d_epochs"], g_epochs=c["g_epochs"], verbose=False, draws="numpy", **kw)
        return m.load_state_dict(self.state("init"))

    def replay(self, **kw):
        """(model, [state_dict after every block], [last loss of every block]) of a replay with the recorded draws."""
        m = self.model(**kw)
        states, losses = [], []

        def on_block(kind, model):
            states.append(model.state_dict())
            losses.append(model.last_losses[kind])

        m.fit(self.X, draws=self.draws, on_block=on_block)
        return m, states, losses

    def block_losses(self):
        """The reference's last logged loss of every block, in block order (D, G, D, G ...)."""
        c = self.cfg
        per_d = len(self.z["d_losses"]) // c["n_epochs"]
        per_g = len(self.z["g_losses"]) // c["n_epochs"]
        out = []
        for e in range(c["n_epochs"]):
            out += [self.z["d_losses"][(e + 1) * per_d - 1], self.z["g_losses"][(e + 1) * per_g - 1]]
        return out


def compare_states(fx, states, tol, what):
    worst = 0.0
    for b, got in enumerate(states):
        want = fx.state("block%d" % b)
        for k, w in want.items():
            d = float(np.abs(np.asarray(got[k], dtype=np.float64) - w).max())
            worst = max(worst, d)
            assert d <= tol, "{}: block {} {} differs by {:.3g} (tolerance {:.3g})".format(what, b, k, d, tol)
    return worst


def random_net(rng, users, items, dim, scale=None, bias=0.3, momentum=0.01):
    """A net in float32 with every tensor and every momentum buffer filled: embeddings uniform(-scale, scale) (default
    0.7 / sqrt(dim): logits of order 1/2), the bias uniform(-bias, bias)."""
    s = 0.7 / np.sqrt(dim) if scale is None else scale
    f = lambda lim, *shape: rng.uniform(-lim, lim, size=shape).astype(np.float32)      # noqa: E731
    return dict(user_emb=f(s, users, dim), item_emb=f(s, items, dim), item_bias=f(bias, items),
                m_user_emb=f(momentum, users, dim), m_item_emb=f(momentum, items, dim), m_item_bias=f(momentum, items))


ITEM_COUNTS = [TILE - 1, TILE, TILE + 1, 3 * TILE + 1]        # one below, at and one above the tile; four tiles
DIMS = [1, 5, 8, 64]

# name: (users, items, dim, positives per user, seed)
SAMPLER_CASES = {
    "below_tile_d5": (24, TILE - 1, 5, 64, 1),
    "tile_d1": (24, TILE, 1, 64, 2),
    "above_tile_d8": (24, TILE + 1, 8, 64, 3),
    "three_tiles_d64": (24, 3 * TILE + 1, 64, 64, 4),
}


def sampler_case(name):
    """(net, {user: ascending positives}) of a sampler case."""
    users, items, dim, npos, seed = SAMPLER_CASES[name]
    rng = np.random.RandomState(1000 + seed)
    net = random_net(rng, users, items, dim)
    pos = {u: np.sort(rng.choice(items, size=npos, replace=False)).astype(np.int64) for u in range(users)}
    return net, pos


def restated_draws(name, seed, draw):
    """The restatement's negatives and G samples of every user of a case: ({u: (items, boundary)}, {u: (items, boundary)})."""
    from aaerec import irgan as I
    net, pos = sampler_case(name)
    neg, smp = {}, {}
    for u, p in pos.items():
        lg = I.logits_f32(net["user_emb"][u], net["item_emb"], net["item_bias"])
        neg[u] = I.draw_negatives(seed, draw, u, p.size, lg, flags=True)
        smp[u] = I.draw_samples(seed, draw, u, p, lg, flags=True)
    return neg, smp
