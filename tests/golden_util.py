"""Helpers shared by the oracle tests and the GPU parity tests: load a fixture
written by tools/gen_golden.py and replay it on any implementation."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

STEP_CASES = [
    "step_nodrop_gauss", "step_masks", "step_masks_uneven", "step_cond_concat",
    "step_cond_categorical", "step_cond_concat_bias", "step_selu", "step_categorical_prior",
    "step_bernoulli_prior", "step_prior_scale", "step_sgd", "step_nonorm", "step_ragged",
    "step_tanh", "step_lrs", "step_wide", "step_headline", "step_c4", "step_saturated",
]

# trainable CategoricalCondition variants (SparseAdam / mean / single index / behind a constant block)
CAT_CASES = ["step_cat_sparse_sum", "step_cat_sparse_mean", "step_cat_single", "step_concat_cat"]

# r6: one reference run per further class name getattr(nn, activation)() accepts (aae.py:110) that the kernels cover
# (tools/gen_golden.py acts); the last four are not monotone: their derivative goes through the stored output's branch bit
ACT_CASES = ["step_act_" + a for a in (
    "softplus", "hardtanh", "relu6", "celu", "softsign", "hardsigmoid", "logsigmoid", "softshrink", "hardshrink", "identity",
    "elu", "leakyrelu", "sigmoid", "gelu", "silu", "mish", "hardswish")]

NET_KEYS = ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"]


class Fixture:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.cfg = json.loads(str(self.z["config_json"]))
        self.steps = self.cfg["steps"]

    def init_params(self):
        out = {k[len("init."):]: self.z[k] for k in self.z.files
               if k.startswith("init.") and not k.startswith("init.cond")}
        if "init_from" in self.cfg:
            # a fixture that starts from another one's initial parameters, some of them rescaled in fp32 (the generator
            # asserts that this restatement gives the reference's own arrays bit for bit): the arrays are stored once
            base = Fixture(self.cfg["init_from"]).init_params()
            for k, f in self.cfg.get("init_scale", {}).items():
                base[k] = (base[k] * np.float32(f)).astype(np.float32)
            out = dict(base, **out)
        return out

    def model_kwargs(self):
        c = self.cfg
        kw = dict(gen_lr=c.get("gen_lr", 1e-3), reg_lr=c.get("reg_lr", 1e-3),
                  prior=c.get("prior", "gauss"), prior_scale=c.get("prior_scale"),
                  optimizer=c.get("optimizer", "adam"),
                  normalize_inputs=c.get("normalize_inputs", True),
                  activation=c.get("activation", "ReLU"),
                  dropout=tuple(c.get("dropout", (0.0, 0.0))))
        return kw

    def batch(self, s, prefix=None):
        p = prefix or f"step{s}"
        return self.z[p + ".indptr"], self.z[p + ".indices"], self.z[p + ".values"]

    def masks(self, s):
        out, j = [], 0
        while f"step{s}.mask{j}" in self.z.files:
            out.append(self.z[f"step{s}.mask{j}"])
            j += 1
        return out or None

    def cond_inputs(self, s, prefix=None):
        p = prefix or f"step{s}"
        out, j = [], 0
        while f"{p}.cond{j}" in self.z.files:
            out.append(self.z[f"{p}.cond{j}"])
            j += 1
        return out or None

    def has_state(self, s):
        if "state_keys" in self.cfg:
            return True
        return f"step{s}.enc.lin1.weight" in self.z.files

    def expected_params(self, s):
        """Every parameter after step s - or, for a fixture whose config names them (state_keys: the arrays recorded after
        every step and those recorded after the last one only), exactly the named ones: a missing array is an error."""
        if "state_keys" in self.cfg:
            sk = self.cfg["state_keys"]
            keys = sk["every"] + (sk["last"] if s == self.steps - 1 else [])
            return {k: self.z[f"step{s}.{k}"] for k in keys}
        out = {}
        for net in ("enc", "dec", "disc"):
            for k in NET_KEYS:
                out[f"{net}.{k}"] = self.z[f"step{s}.{net}.{k}"]
        return out

    def expected_adam(self, s):
        """{(optimiser, 'net.key'): (m, v, t)}"""
        out = {}
        for tag, net in (("A_enc", "enc"), ("A_dec", "dec"), ("A_gen", "enc"), ("A_disc", "disc")):
            if not any(f"step{s}.{tag}.{i}.m" in self.z.files for i in range(len(NET_KEYS))):
                continue
            for i, k in enumerate(NET_KEYS):
                key = f"step{s}.{tag}.{i}.m"
                if key in self.z.files:
                    out[(tag, f"{net}.{k}")] = (self.z[key], self.z[f"step{s}.{tag}.{i}.v"],
                                                float(self.z[f"step{s}.{tag}.{i}.t"]))
        return out


BCE_CUT = 24.0 * np.log(2.0)    # fp32: 1 / (1 + exp(-l)) == 1.0f from here on (fl(1 + e) == 1 iff e <= 2^-24)


def bce_quantisation_bound(logits, indptr, indices, values=None):
    """How far the reconstruction loss of an exact zero-target form (softplus(l), the kernels') may lie from the reference's
    mean of -log(1 - fl(sigmoid(l))), from the logits alone.  Below the cut-off the reference's q = 1 - fl(sigmoid(l)) carries
    an absolute error of at most d = 1.5 * 2^-24 (half a step of 1 + e, half a step of the quotient; 1 - s is exact) and is
    at least 2^-24; the exact form has none to speak of.  A zero-target cell's term therefore differs by at most
    max(log((q + d) / q), log(q / max(q - d, 2^-24))), q = 1 / (1 + exp(l)) in fp64.  From the cut-off on both charge the
    clamped 100.  Summed over the zero-target cells, divided by B N.  (values: the targets of the CSR entries where they are
    not all 1 - a cell of target t carries the term with the weight 1 - t.)"""
    L = np.asarray(logits, dtype=np.float64)
    B, N = L.shape
    weight = np.ones((B, N))
    rows = np.repeat(np.arange(B), np.diff(indptr))
    weight[rows, indices] = 0.0 if values is None else 1.0 - np.asarray(values, dtype=np.float64)
    below = L < BCE_CUT
    q = 1.0 / (1.0 + np.exp(L[below]))
    d = 1.5 * 2.0 ** -24
    per_cell = np.maximum(np.log((q + d) / q), np.log(q / np.maximum(q - d, 2.0 ** -24)))
    return float((per_cell * weight[below]).sum() / (B * N))


# Errors of the rendezvous itself - the port a probe socket read back was taken before the ranks bound it, or the store was
# not up yet.  Nothing that a hung or crashed COLLECTIVE also prints ("timed out", "Broken pipe", "Connection reset": ADVICE r5 -
# a real intermittent distributed bug must fail the test, not be retried into green).
_RENDEZVOUS_TROUBLE = ("Address already in use", "EADDRINUSE", "Connection refused", "connect() timed out",
                       "The server socket has failed to listen", "failed to bind")


def spawn_ranks(worker, world, args_for_port, attempts=3):
    """mp.spawn of `world` ranks on a free rendezvous port: args_for_port(port) -> the worker's arguments.  A port read back from a
    probe socket can be taken by someone else before the ranks bind it (seen once in this suite): a spawn that dies with a
    BIND / CONNECT error of the rendezvous - not an assertion of the test, not a collective's time-out - is repeated on a new port,
    with the shared result dicts of the failed attempt emptied, and says so."""
    import sys
    import torch.multiprocessing as mp
    for attempt in range(attempts):
        port = free_port()
        args = args_for_port(port)
        try:
            mp.spawn(worker, args=args, nprocs=world, join=True)
            return
        except Exception as e:      # noqa: BLE001 - ProcessRaisedException / ProcessExitedException carry the worker's traceback as text
            text = str(e)
            if attempt + 1 < attempts and "AssertionError" not in text and any(t in text for t in _RENDEZVOUS_TROUBLE):
                for a in args:      # (manager dicts the dead ranks may have written to)
                    if hasattr(a, "keys") and hasattr(a, "clear"):
                        a.clear()
                print(f"spawn_ranks: rendezvous on port {port} failed ({text.strip().splitlines()[-1][:120]}); attempt {attempt + 2} of {attempts}",
                      file=sys.stderr)
                continue
            raise


def free_port():
    """A TCP port nothing listens on right now (for the rendezvous of a spawned process group): bind to 0, read it back."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]
