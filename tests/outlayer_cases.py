"""The cases of the output-layer edge sweep (tests/test_outlayer_edges_cpu.py, tests/test_outlayer_edges_gpu.py): the decoder's
output layer ALONE - HipAAE.output_layer_step on a handle with a code of 10 - at the shape edges of its kernels, every form of
the layer against a float64 restatement of the call.

A case is one shape (N items, h hidden units, B rows) and its seeded inputs; each case varies ONE edge around (167, 100, 37):

  h   h + 1 columns go into 4, 7 or 13 column blocks of 16 (64, 112 or 208 columns; k-steps of 32, two k halves; the third
      k-step of a half lives in LDS at 13 blocks only): the last column block full, holding one column and empty at each block
      count, both sides of every change of the count
  B   row blocks of 16 rows, the balanced wave map from four row blocks on at 13 column blocks, the fused limit of 109 rows -
      at h = 207 (13 blocks, the LDS k-step), a subset at h = 100 and h = 40
  N   tiles of 32 items with a ragged last tile, one tile, two items; 8500 items, where a workgroup of the deferred launch
      walks many tiles (all 266 of them at width 1)
  blocked   batches beyond one launch on a blocked_output handle under BLOCKED_ANY: row blocks of ceil(B / ceil(B / 104)) rows -
      113 (57 + 56: the last block one row shorter), 208 (two full blocks), 209 (three), 230, 313 (four)
  dense   every row holds all 32 items of tile 0: that tile's entry list has 37 * 32 = 1184 entries, more than 1024

Two consecutive calls on a different batch each, so that the second reads the parameters and moments the first stored.  Inputs
(all from the case's seed): dec.lin3.weight 0.1 N(0, 1), bias 0.05 N(0, 1) - logits within about +-5, asserted |logit| < 12:
the saturated band is tests/test_bce_saturation_gpu.py's subject; dh2 uniform in [0, 1) with about 30 % exact zeros and the
constant-1 column; Adam moments m ~ 1e-4 N(0, 1), v = 1e-8 + 1e-7 U[0, 1) at step count 5, so that no update hinges on a
gradient of the order of Adam's eps; lr 1e-3, grad_scale 0.5; targets a CSR with values from {1, 1, 0.25, 0.5, 0.75}, empty rows,
one row that holds every item, the last item of the ragged tile hit; odd cases read the batch through a permutation window
(rows=) into a corpus three times as long.

The reference is Restatement64 below.  Beside it runs test_bce_saturation_gpu.Restatement, the same call in the reference's fp32
arithmetic; how far that one lies from float64 - per quantity, relative to the quantity's largest magnitude - is the measure of
what fp32 alone costs, and every tolerance is FOUR times the largest such figure over the list (the factor of
tests/bf16_cases.py: a quarter for the reference, three quarters for the device's summation order and the 2^-23 cross terms its
three-term product drops).  tests/test_outlayer_edges_cpu.py asserts the quarter for every case."""
import functools
import zlib

import numpy as np

LR, GRAD_SCALE, ADAM_STEP = 1e-3, 0.5, 5
BASE = (167, 100, 37)
K_DEC_BCE_FWD, K_DEC_FUSED, K_DEC_CRIT, K_DEC_OPT = 1, 5, 7, 8        # aaerec._hip kernel ids of the profile

# form -> (constructor keywords, library option around the creation, aae_set_split width or None, kernel ids that must have
# run, kernel ids that must not)
FORMS = {
    "single": ({}, None, None, (K_DEC_FUSED,), (K_DEC_CRIT, K_DEC_OPT, K_DEC_BCE_FWD)),
    "split": ({}, "SPLIT_ANY", None, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    "split1": ({}, "SPLIT_ANY", 1, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    "three": (dict(unfused_decoder=True), None, None, (K_DEC_BCE_FWD,), (K_DEC_FUSED, K_DEC_CRIT, K_DEC_OPT)),
    "blocked": (dict(blocked_output=True), "BLOCKED_ANY", None, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    "split-sgd": (dict(optimizer="sgd"), "SPLIT_ANY", None, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    "split1-sgd": (dict(optimizer="sgd"), "SPLIT_ANY", 1, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
    "blocked-sgd": (dict(blocked_output=True, optimizer="sgd"), "BLOCKED_ANY", None, (K_DEC_CRIT, K_DEC_OPT), (K_DEC_FUSED, K_DEC_BCE_FWD)),
}
ONE_LAUNCH = ("single", "split", "split1", "three")

H_EDGES = [1, 2, 15, 16, 47, 62, 63, 64, 95, 96, 110, 111, 112, 175, 191, 192, 206, 207]
B_EDGES = [1, 15, 16, 17, 48, 49, 63, 64, 65, 96, 97, 104, 108, 109]
N_EDGES = [2, 31, 32, 33, 63, 64, 65, 167]
BLOCKED_ROWS = [113, 208, 209, 230, 313]


def _cases():
    N0, h0, B0 = BASE
    out = [(f"h{h}", N0, h, B0, ONE_LAUNCH) for h in H_EDGES]
    out += [(f"B{B}-h207", N0, 207, B, ONE_LAUNCH) for B in B_EDGES]
    out += [(f"B{B}-h100", N0, 100, B, ONE_LAUNCH) for B in (1, 16, 17, 64, 109)]
    out += [(f"B{B}-h40", N0, 40, B, ONE_LAUNCH) for B in (15, 49, 96, 109)]
    out += [(f"N{N}", N, h0, B0, ONE_LAUNCH) for N in N_EDGES]        # (N167: the base shape itself)
    out += [("N8500", 8500, h0, B0, ONE_LAUNCH)]
    out += [("dense-tile0", N0, h0, B0, ONE_LAUNCH)]
    out += [(f"blocked-B{B}-h{h}", N0, h, B, ("blocked",)) for h in (100, 207) for B in BLOCKED_ROWS]
    out += [(f"blocked-B{B}-h{h}-N33", 33, h, B, ("blocked",)) for h in (100, 207) for B in (113, 313)]
    # (a case's seed is a digest of its id: adding a case moves no other case's inputs)
    sgd = {"N167": ("split-sgd", "split1-sgd"), "B109-h207": ("split-sgd",), "N8500": ("split1-sgd",), "blocked-B230-h207": ("blocked-sgd",)}
    return [dict(id=cid, N=N, h=h, B=B, forms=tuple(forms) + sgd.get(cid, ()), seed=zlib.crc32(cid.encode()), window=bool(i % 2), dense=cid == "dense-tile0")
            for i, (cid, N, h, B, forms) in enumerate(out)]


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
RUNS = [(c["id"], form) for c in CASES for form in c["forms"]]


def _targets(rng, N, B, dense):
    """Item lists of B rows: some rows empty, row 0 every item, the last item hit; dense: all 32 items of tile 0 in every row."""
    rows = []
    for b in range(B):
        if b == 0:
            items = np.arange(N)
        elif b % 5 == 2 and not dense:
            items = np.zeros(0, dtype=np.int64)
        else:
            items = rng.choice(N, size=int(rng.integers(1, min(N, 12) + 1)), replace=False)
            if b % 3 == 1:
                items = np.union1d(items, [N - 1])
        if dense:
            items = np.union1d(items, np.arange(32))
        rows.append(np.sort(items).astype(np.int32))
    return rows


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """The seeded inputs of a case (host arrays, shared by every form): w, b, the four moments, per call dh2 [B, h + 1] and the dense
    targets T [B, N]; the resident corpus as CSR arrays and per call the rows of the batch in it (None: rows c B .. (c + 1) B - 1)."""
    c = BY_ID[cid]
    N, h, B = c["N"], c["h"], c["B"]
    rng = np.random.default_rng(c["seed"])
    w = (rng.standard_normal((N, h)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(N) * 0.05).astype(np.float32)
    mom = dict(m_w=(rng.standard_normal((N, h)) * 1e-4).astype(np.float32), v_w=(1e-8 + 1e-7 * rng.random((N, h))).astype(np.float32),
               m_b=(rng.standard_normal(N) * 1e-4).astype(np.float32), v_b=(1e-8 + 1e-7 * rng.random(N)).astype(np.float32))
    dh2 = []
    for call in range(2):
        d = np.ones((B, h + 1), dtype=np.float32)
        d[:, :h] = rng.random((B, h)).astype(np.float32) * (rng.random((B, h)) > 0.3)
        dh2.append(d)
    batch_rows = [_targets(rng, N, B, c["dense"]) for call in range(2)]
    n_docs = 6 * B if c["window"] else 2 * B
    docs = [None] * n_docs
    pick = None
    if c["window"]:
        place = rng.permutation(n_docs)[:2 * B].astype(np.int32)
        pick = [place[:B], place[B:]]
        for call in range(2):
            for j, doc in enumerate(pick[call]):
                docs[doc] = batch_rows[call][j]
        for doc in range(n_docs):
            if docs[doc] is None:
                docs[doc] = np.sort(rng.choice(N, size=int(rng.integers(0, min(N, 12) + 1)), replace=False)).astype(np.int32)
    else:
        docs = batch_rows[0] + batch_rows[1]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64)
    indices = np.concatenate(docs).astype(np.int32)
    values = np.asarray([1.0, 1.0, 0.25, 0.5, 0.75], dtype=np.float32)[np.arange(len(indices)) % 5]
    T = []
    for call in range(2):
        t = np.zeros((B, N), dtype=np.float32)
        for j in range(B):
            doc = int(pick[call][j]) if pick else call * B + j
            t[j, indices[indptr[doc]:indptr[doc + 1]]] = values[indptr[doc]:indptr[doc + 1]]
        T.append(t)
    return dict(w=w, b=b, mom=mom, dh2=dh2, T=T, corpus=(indptr, indices, values), n_docs=n_docs, pick=pick)


class Restatement64:
    """aae_output_layer_step in float64: logits = dh2 V3^T + b3; F.binary_cross_entropy(sigmoid + 1e-12, T + 1e-12) with its clamped
    logs, and its gradient as autograd forms it (the 1e-12 floor of the denominator), times grad_scale / (B N); dA2 = G V3;
    dV3 = G^T dh2, db3 = sum_b G; torch.optim.Adam from the loaded moments and step count, or SGD."""

    def __init__(self, w, b, lr, scale, moments=None, step=0, optimizer="adam"):
        f64 = np.float64
        self.p = {"w": w.astype(f64), "b": b.astype(f64)}
        self.lr, self.scale, self.t, self.adam = float(lr), float(scale), int(step), optimizer == "adam"
        z = lambda k: np.zeros_like(self.p[k])       # noqa: E731
        self.m = {"w": moments["m_w"].astype(f64), "b": moments["m_b"].astype(f64)} if moments else {"w": z("w"), "b": z("b")}
        self.v = {"w": moments["v_w"].astype(f64), "b": moments["v_b"].astype(f64)} if moments else {"w": z("w"), "b": z("b")}

    def step(self, dh2, T):
        B, N = T.shape
        h2 = dh2[:, :-1].astype(np.float64)
        logits = h2 @ self.p["w"].T + self.p["b"]
        s = 1.0 / (1.0 + np.exp(-logits))
        x, t = s + 1e-12, T.astype(np.float64) + 1e-12
        cells = -(t * np.maximum(np.log(x), -100.0) + (1.0 - t) * np.maximum(np.log1p(-x), -100.0))
        G = (x - t) / np.maximum((1.0 - x) * x, 1e-12) * (self.scale / (B * N)) * s * (1.0 - s)
        da2 = G @ self.p["w"]
        grads = {"w": G.T @ h2, "b": G.sum(0)}
        self.t += 1
        for k, g in grads.items():
            if not self.adam:
                self.p[k] -= self.lr * g
                continue
            b1, b2, eps = 0.9, 0.999, 1e-8
            self.m[k] += (1 - b1) * (g - self.m[k])
            self.v[k] = b2 * self.v[k] + (1 - b2) * g * g
            self.p[k] -= (self.lr / (1 - b1 ** self.t)) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(1 - b2 ** self.t) + eps)
        return float(cells.mean()), da2, logits


QUANTITIES = ("loss", "da2", "w", "b", "m_w", "v_w", "m_b", "v_b")


def _collect(losses, da2s, p, m, v):
    return dict(loss=np.asarray(losses), da2=np.stack(da2s), w=p["w"], b=p["b"], m_w=m["w"], v_w=v["w"], m_b=m["b"], v_b=v["b"])


@functools.lru_cache(maxsize=None)
def reference(cid, optimizer="adam"):
    """The float64 restatement's results over the two calls, by QUANTITIES (loss [2], da2 [2, B, h]; the rest after the second
    call), and the largest |logit|."""
    x = inputs(cid)
    ref = Restatement64(x["w"], x["b"], LR, GRAD_SCALE, x["mom"], ADAM_STEP, optimizer)
    out = [ref.step(x["dh2"][call], x["T"][call]) for call in range(2)]
    res = _collect([o[0] for o in out], [o[1] for o in out], ref.p, ref.m, ref.v)
    res["max_logit"] = max(float(np.abs(o[2]).max()) for o in out)
    return res


def restated_fp32(cid, optimizer="adam"):
    """The same two calls through test_bce_saturation_gpu.Restatement (the reference's fp32 arithmetic), by QUANTITIES.  The loss is
    rounded to float32: the reference's loss is an fp32 tensor, and the device hands back an fp32 number."""
    from test_bce_saturation_gpu import Restatement
    x = inputs(cid)
    emu = Restatement(x["w"], x["b"], LR, GRAD_SCALE, False, moments=x["mom"], step=ADAM_STEP, optimizer=optimizer)
    out = [emu.step(x["dh2"][call], x["T"][call]) for call in range(2)]
    m = {k: emu.opt.m.get(k, x["mom"]["m_" + k]) for k in ("w", "b")}
    v = {k: emu.opt.v.get(k, x["mom"]["v_" + k]) for k in ("w", "b")}
    return _collect([np.float32(o[0]) for o in out], [o[1] for o in out], emu.p, m, v)


def distance(got, ref, optimizer="adam"):
    """Per quantity: the largest |got - ref| relative to the largest |ref| (the loss: per call, relative to that call's loss).
    SGD: the moments take no part (they must come back bitwise as loaded)."""
    out = {}
    for q in QUANTITIES:
        if optimizer != "adam" and q[:2] in ("m_", "v_"):
            continue
        g, r = np.asarray(got[q], dtype=np.float64), np.asarray(ref[q], dtype=np.float64)
        out[q] = float(np.max(np.abs(g - r) / np.abs(r))) if q == "loss" else float(np.abs(g - r).max() / np.abs(r).max())
    return out


# The largest distance of the fp32 restatement from the float64 one over CASES (tests/test_outlayer_edges_cpu.py prints every
# case's OUTPAIR line and asserts these maxima), and the cases that set them.  Each tolerance is four times its figure.
# Measured, then rounded up to two digits: loss 4.59e-8 (N167; the rounding of the loss to float32 alone can reach 6e-8), da2
# 7.35e-7 (B17-h100), w 8.22e-8 (N33), b 9.95e-8 (blocked-B230-h207), m_w 4.67e-7 and v_b 3.87e-7 (both blocked-B313-h207-N33:
# 313-term column sums in fp32), v_w 2.81e-7 (N2), m_b 3.93e-7 (blocked-B208-h100).  In absolute terms (largest |w| ~ 0.45,
# |m| ~ 4.5e-4, v ~ 1.1e-7): parameters 1.5e-7, m 8.5e-10, v 1.3e-13 - the first two tighter than the 2e-6 and 1e-9 (+ 1e-4
# relative) at which tests/test_dec_opt_pipeline_gpu.py holds the split form to the three-kernel path, the third about its 1e-13
# (+ 1e-4 relative).
PAIR_MAX = {"loss": 4.6e-8, "da2": 7.4e-7, "w": 8.3e-8, "b": 1.0e-7, "m_w": 4.7e-7, "v_w": 2.9e-7, "m_b": 4.0e-7, "v_b": 3.9e-7}
TOL ={q: 4.0 * v for q, v in PAIR_MAX.items()}
