"""What test_vae_wide_cpu.py and test_vae_wide_gpu.py share: the bound, the two reference fixtures with a decoder input wider
than one 208-column slot (tools/gen_golden.py gen_vae: a constant block + CategoricalCondition(32) in one ConditionList) and
their oracle, random parameters and batches of the boundary sweep."""
import numpy as np

from oracle import aae_oracle as O

W_MAX = 1040                         # n_code + cond_inc + 1 of a VAE handle: five k-parts of 208 columns (csrc/abi_model.h)
WIDE_FIXTURES = ["step_vae_wide", "step_vae_wide5"]
VAE_NAMES = ("fc1", "fc21", "fc22", "fc3", "fc4")


def build_wide_oracle(fx):
    """OracleVAE behind [ConcatConst(block), CategoricalEmbedding(32)] - the order of the fixture's ConditionList."""
    k = fx.cfg["cat"]
    conds = [O.ConcatConst(fx.cfg["concat"]),
             O.CategoricalEmbedding(fx.z["init.cond.embedding"], lr=k["lr"], reduce=k["reduce"], sparse=k["sparse"])]
    assert fx.cfg["concat"] + conds[1].inc == fx.cfg["cond_inc"]
    params = {f"{n}.{t}": fx.z[f"init.{n}.{t}"] for n in VAE_NAMES for t in ("weight", "bias")}
    return O.OracleVAE(params, lr=fx.cfg["gen_lr"], conditions=conds)


def vae_params(N, h, c, inc, seed, spread=1.0):
    """nn.Linear's uniform initialisation of the five Linears under the oracle's names (fc4 times `spread`)."""
    r = np.random.default_rng(seed)

    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return r.uniform(-b, b, (o, i)).astype(np.float32), r.uniform(-b, b, o).astype(np.float32)
    p = {}
    for name, (o, i) in (("fc1", (h, N)), ("fc21", (c, h)), ("fc22", (c, h)), ("fc3", (h, c + inc)), ("fc4", (N, h))):
        p[name + ".weight"], p[name + ".bias"] = lin(o, i)
    p["fc4.weight"] *= np.float32(spread)
    return p


def to_hip(p):
    return {"enc.lin1.weight": p["fc1.weight"], "enc.lin1.bias": p["fc1.bias"],
            "enc.lin3.weight": np.vstack([p["fc21.weight"], p["fc22.weight"]]),
            "enc.lin3.bias": np.concatenate([p["fc21.bias"], p["fc22.bias"]]),
            "dec.lin1.weight": p["fc3.weight"], "dec.lin1.bias": p["fc3.bias"],
            "dec.lin3.weight": p["fc4.weight"], "dec.lin3.bias": p["fc4.bias"]}


def from_oracle(p):
    """The oracle's parameters under the handle's names."""
    return to_hip(p)


def corpus(r, N, n_docs, max_len):
    rows = [np.sort(r.choice(N, size=int(r.integers(1, max_len)), replace=False)) for _ in range(n_docs)]
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), np.ones(int(ip[-1]), dtype=np.float32), rows
