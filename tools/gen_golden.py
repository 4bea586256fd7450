#!/usr/bin/env python3
"""Generate golden fixtures for the AAE hot path from the *real* reference.

Runs ONLY in the build container (needs /root/reference).  It imports the
reference package unmodified (with the three import shims listed in SURVEY.md
section 8c), drives `AdversarialAutoEncoder.partial_fit` (aaerec/aae.py:745-766)
step by step with recorded randomness, and dumps inputs + expected outputs as
small .npz files under tests/golden/.  Only data is written: no reference
source travels.

    python tools/gen_golden.py            # regenerate every fixture

Randomness capture:
  * `prior_sampler` is wrapped so every z_real drawn in disc_step
    (aae.py:716) is recorded.
  * every nn.Dropout / nn.AlphaDropout of enc/dec/disc is replaced (after
    construction, before the first step) by a recording module that draws the
    same Bernoulli noise torch draws and stores the keep-mask in call order.
    The generator asserts once that the recording modules reproduce torch's
    own dropout bit for bit under the same seed.
"""
import json
import os
import sys
import types

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

REF = "/root/reference"
# (AAE_GOLDEN_OUT: another directory - a fixture whose seed is still being chosen is generated to a scratch directory first)
OUT = os.environ.get("AAE_GOLDEN_OUT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def import_reference():
    """stand-in modules, then import."""
    for name in ("gensim", "gensim.models", "gensim.models.keyedvectors",
                 "docutils", "docutils.nodes"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["gensim.models.keyedvectors"].KeyedVectors = type("KeyedVectors", (), {})
    sys.modules["gensim.models"].keyedvectors = sys.modules["gensim.models.keyedvectors"]
    sys.modules["gensim"].models = sys.modules["gensim.models"]
    sys.modules["docutils.nodes"].inline = object
    if not hasattr(np, "product"):
        np.product = np.prod
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import aaerec.aae as ref_aae          # noqa
    import aaerec.condition as ref_cond   # noqa
    return ref_aae, ref_cond


# ----------------------------------------------------------------------------
# recording dropouts
# ----------------------------------------------------------------------------
class RecDropout(nn.Module):
    """x * bernoulli(1-p) / (1-p); records the keep mask (uint8)."""

    def __init__(self, p, log, tag):
        super().__init__()
        self.p, self.log, self.tag = float(p), log, tag

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        noise = torch.empty_like(x).bernoulli_(1 - self.p)
        self.log.append((self.tag, noise.numpy().astype(np.uint8).copy()))
        return x * noise.div(1 - self.p)


class RecAlphaDropout(nn.Module):
    """torch's alpha_dropout (aten/src/ATen/native/Dropout.cpp, feature=False,
    alpha=True): a = 1/sqrt((alpha^2 p + 1)(1-p)); b = (noise-1)*alpha*a + alpha*a*p;
    out = x * (noise*a) + b."""
    ALPHA = 1.7580993408473766

    def __init__(self, p, log, tag):
        super().__init__()
        self.p, self.log, self.tag = float(p), log, tag

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        p = self.p
        noise = torch.empty_like(x).bernoulli_(1 - p)
        self.log.append((self.tag, noise.numpy().astype(np.uint8).copy()))
        a = 1.0 / np.sqrt((self.ALPHA ** 2 * p + 1) * (1 - p))
        b = noise.add(-1).mul_(self.ALPHA * a).add_(self.ALPHA * a * p)
        return x * noise.mul(a) + b


def _selfcheck_recording_dropouts():
    x = torch.randn(7, 13)
    for cls, ref in ((RecDropout, nn.Dropout), (RecAlphaDropout, nn.AlphaDropout)):
        log = []
        torch.manual_seed(123)
        got = cls(0.3, log, "t").train()(x)
        torch.manual_seed(123)
        want = ref(0.3).train()(x)
        assert torch.equal(got, want), cls.__name__


# ----------------------------------------------------------------------------
# synthetic batches
# ----------------------------------------------------------------------------
def make_batch(rng, B, N, min_len=1, max_len=8, dup_row=None, empty_row=None):
    rows = []
    for b in range(B):
        n = int(rng.integers(min_len, max_len + 1))
        rows.append(list(rng.choice(N, size=n, replace=False)))
    if dup_row is not None:          # duplicate item -> value 2.0 after tocsr(); NOTE: the
        # reference then fails in F.binary_cross_entropy ("all elements of target should be
        # between 0 and 1", torch>=1.x) - our partial_fit mirrors that error, no fixture.
        rows[dup_row] = rows[dup_row] + [rows[dup_row][0]]
    if empty_row is not None and empty_row < B:
        rows[empty_row] = []
    ind0 = [b for b, r in enumerate(rows) for _ in r]
    ind1 = [i for r in rows for i in r]
    X = sp.coo_matrix((np.ones(len(ind0)), (ind0, ind1)), shape=(B, N)).tocsr()
    X.sum_duplicates()
    X.sort_indices()
    return X


def state_np(module):
    return {k: v.detach().numpy().copy() for k, v in module.state_dict().items()}


def optim_np(opt, params):
    """Adam: exp_avg / exp_avg_sq / step per parameter, in `params` order.
    SGD: nothing (momentum=0)."""
    out = {}
    for i, p in enumerate(params):
        st = opt.state.get(p, {})
        if "exp_avg" in st:
            out[f"{i}.m"] = st["exp_avg"].numpy().copy()
            out[f"{i}.v"] = st["exp_avg_sq"].numpy().copy()
            out[f"{i}.t"] = np.asarray(float(st["step"]))
    return out


# CategoricalCondition variants (condition.py:397-508): optimiser (sparse=True -> SparseAdam), reduction over the
# padded list (None = one value per document), and whether a constant 30-wide block precedes it in the ConditionList
CAT_KINDS = {
    "categorical": dict(sparse=False, reduce="sum", concat=False),
    "cat_sparse_sum": dict(sparse=True, reduce="sum", concat=False),
    "cat_sparse_mean": dict(sparse=True, reduce="mean", concat=False),
    "cat_single": dict(sparse=True, reduce=None, concat=False),
    "concat30+cat": dict(sparse=True, reduce="sum", concat=True),
    "cat_max": dict(sparse=True, reduce="max", concat=False),
    "cat_max_dense": dict(sparse=False, reduce="max", concat=False),
}

# EmbeddingBagCondition(12, 8, **kwargs) (condition.py:372-394): nn.EmbeddingBag over [B, 3] index blocks + its own Adam
BAG_KINDS = {
    "bag_mean": dict(),                 # nn.EmbeddingBag's default mode
    "bag_max": dict(mode="max"),
    "bag_sum": dict(mode="sum"),
}
BAG_VOCAB, BAG_DIM, BAG_WIDTH = 12, 8, 3


def max_categorical(ref_cond, *a, **k):
    """CategoricalCondition(reduce="max") in a form that runs.  The reference's encode() hands the (values, indices) pair of
    hid.max(1) on to torch.cat (condition.py:494), which raises; the values are what its docstring's 'max' means, so the
    recorded runs take element 0 of the pair and leave everything else - nn.Embedding(padding_idx=0), the padding, the
    optimiser - to the reference's own code."""
    class MaxCategorical(ref_cond.CategoricalCondition):
        def encode(self, inputs):
            return super().encode(inputs)[0]
    return MaxCategorical(*a, **k)


def bag_record(out, prefix, bag):
    """The condition table and its optimiser state (Adam: exp_avg, exp_avg_sq, step) of an EmbeddingBagCondition."""
    w = bag.embedding_bag.weight
    out[f"{prefix}.cond.embedding"] = w.detach().numpy().copy()
    st = bag.optimizer.state[w]
    out[f"{prefix}.cond.m"] = st["exp_avg"].numpy().copy()
    out[f"{prefix}.cond.v"] = st["exp_avg_sq"].numpy().copy()
    out[f"{prefix}.cond.t"] = np.asarray(float(st["step"]))


def _pad_lists(lists):
    if not isinstance(lists[0], list):
        return np.asarray(lists, dtype=np.int64)
    L = max(len(l) for l in lists)
    return np.asarray([l + [0] * (L - len(l)) for l in lists], dtype=np.int64)


def gen_embedded_vectorizer():
    """EmbeddedVectorizer.fit / transform of the reference (ub.py:38-68) on a small corpus: TF-IDF over the embedding's
    vocabulary times the embedding.  Its constructor hands `self` to TfidfVectorizer positionally, which the
    scikit-learn of this image rejects, so the object is built by calling TfidfVectorizer.__init__ with the same
    keyword arguments; fit and transform are the reference's own methods."""
    from sklearn.feature_extraction.text import TfidfVectorizer
    import aaerec.ub as ref_ub
    rng = np.random.default_rng(77)
    words = ["w%d" % i for i in range(400)]
    emb = rng.standard_normal((400, 300)).astype(np.float32)
    docs = [" ".join(rng.choice(words + ["unknown", "oov"], size=int(rng.integers(0, 15)))) for _ in range(120)]
    test = [" ".join(rng.choice(words + ["unseen"], size=int(rng.integers(1, 10)))) for _ in range(40)]
    out = {"words": np.asarray(json.dumps(words)), "docs": np.asarray(json.dumps(docs)),
           "test": np.asarray(json.dumps(test)), "embedding": emb}
    for tag, kw in (("default", {}), ("sublinear", dict(sublinear_tf=True, norm="l1"))):
        v = ref_ub.EmbeddedVectorizer.__new__(ref_ub.EmbeddedVectorizer)
        TfidfVectorizer.__init__(v, vocabulary=words, **kw)
        v.embedding, v.index2word = emb, words            # (get_params reads the constructor arguments back)
        out[f"{tag}.train"] = np.asarray(ref_ub.EmbeddedVectorizer.fit_transform(v, docs))
        out[f"{tag}.test"] = np.asarray(ref_ub.EmbeddedVectorizer.transform(v, test))
        out[f"{tag}.kwargs"] = np.asarray(json.dumps(kw))
    path = os.path.join(OUT, "embedded_vectorizer.npz")
    np.savez_compressed(path, **out)
    print(f"embedded_vectorizer: {os.path.getsize(path) / 1024:.0f} KiB, train {out['default.train'].shape} "
          f"{out['default.train'].dtype}")


ENC_KEYS = ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias"]


def run_case(ref_aae, ref_cond, name, N=300, h=20, c=10, B=16, steps=3, seed=0,
             cond=None, batch_kw=None, last_B=None, capture_acts=True, states='all', init_scale=None, init_from=None,
             state_keys=None, predict_B=None, finish=None, **model_kw):
    """Drive `steps` partial_fit calls on the reference; return a flat dict of arrays.
    init_scale {"dec.lin3.weight": 400.0}: initial parameters multiplied (in fp32) after the nets are built, before init.* is
    recorded.  init_from: the fixture whose init.* arrays (rescaled by init_scale) these are - asserted bit for bit, then left
    out of the file.  state_keys {"every": [...], "last": [...], "adam": [...]}: record only these parameters after every /
    the last step, Adam moments for "adam" only (a fixture at the headline widths within the size limit of a committed
    file).  finish(out, cfg, logits): called before the file is written, with dec.lin3's output of every training step."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(1000 + seed)
    model_kw.setdefault("dropout", (0.0, 0.0))
    conditions = None
    cond_inc = 0
    cond_batches = None
    concat_w = int(cond[6:]) if cond and cond.startswith("concat") and cond[6:].isdigit() else 0
    if concat_w:            # a constant concatenated block: "concat30", "concat300" (config C4's 300-d title vectors)
        class ConstConcat(ref_cond.ConcatenationBasedConditioning):
            def size_increment(self):
                return concat_w

            def encode(self, inputs):
                return torch.as_tensor(inputs, dtype=torch.float32)
        conditions = ref_cond.ConditionList([("title", ConstConcat())])
        cond_inc = concat_w
    elif cond in CAT_KINDS:
        kind = CAT_KINDS[cond]
        make = (lambda *a, **k: max_categorical(ref_cond, *a, **k)) if kind["reduce"] == "max" else ref_cond.CategoricalCondition
        cc = make(8, sparse=kind["sparse"], use_cuda=False, reduce=kind["reduce"], lr=1e-2)
        items = [("authors", cc)]
        cond_inc = 8
        if kind["concat"]:
            class ConstConcat(ref_cond.ConcatenationBasedConditioning):
                def size_increment(self):
                    return 30

                def encode(self, inputs):
                    return torch.as_tensor(inputs, dtype=torch.float32)
            items.insert(0, ("title", ConstConcat()))
            cond_inc = 38
        conditions = ref_cond.ConditionList(items)
    elif cond in BAG_KINDS:
        bag = ref_cond.EmbeddingBagCondition(BAG_VOCAB, BAG_DIM, **BAG_KINDS[cond])
        conditions = ref_cond.ConditionList([("authors", bag)])
        cond_inc = BAG_DIM
    elif cond == "concat30+bias":
        class ConstConcat(ref_cond.ConcatenationBasedConditioning):
            def size_increment(self):
                return 30

            def encode(self, inputs):
                return torch.as_tensor(inputs, dtype=torch.float32)

        class ConstBias(ref_cond.ConditionalBiasing):
            def encode(self, inputs):
                return torch.as_tensor(inputs, dtype=torch.float32)
        conditions = ref_cond.ConditionList([("title", ConstConcat()), ("b", ConstBias())])
        cond_inc = 30

    m = ref_aae.AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=B, n_epochs=1,
                                       conditions=conditions, verbose=True, **model_kw)
    # build nets + optimisers exactly as fit() does (aae.py:782-804)
    m.enc = ref_aae.Encoder(N, h, c, final_activation=m.encoder_activation,
                            normalize_inputs=m.normalize_inputs, activation=m.activation,
                            dropout=m.dropout)
    m.dec = ref_aae.Decoder(c + cond_inc, h, N, activation=m.activation, dropout=m.dropout)
    m.disc = ref_aae.Discriminator(c, h, dropout=m.dropout, activation=m.activation)
    og = ref_aae.TORCH_OPTIMIZERS[m.optimizer]
    m.enc_optim = og(m.enc.parameters(), lr=m.gen_lr)
    m.dec_optim = og(m.dec.parameters(), lr=m.gen_lr)
    m.gen_optim = og(m.enc.parameters(), lr=m.reg_lr)
    m.disc_optim = og(m.disc.parameters(), lr=m.reg_lr)

    for k, f in (init_scale or {}).items():
        net_name, key = k.split(".", 1)
        with torch.no_grad():
            getattr(m, net_name).state_dict()[key].mul_(float(f))
    logits_log = []
    if finish is not None:
        m.dec.lin3.register_forward_hook(lambda mod, inp, outp: logits_log.append(outp.detach().numpy().copy()))

    # recording dropouts
    masks_log = []
    selu = (m.activation == "SELU")
    for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", m.disc)):
        for li, attr in enumerate(("drop1", "drop2")):
            cls = RecAlphaDropout if selu else RecDropout
            setattr(net, attr, cls(m.dropout[li], masks_log, f"{net_name}.{attr}"))

    # recording prior
    z_log = []
    orig_sampler = m.prior_sampler

    def rec_sampler(size):
        z = orig_sampler(size)
        z_log.append(z.numpy().copy())
        return z
    m.prior_sampler = rec_sampler

    # loss capture
    loss_log = []
    ref_aae.log_losses = lambda *l: loss_log.append(l)
    ref_aae.USE_WANDB = False

    out = {}
    cfg = dict(N=N, h=h, c=c, B=B, steps=steps, cond=cond or "", cond_inc=cond_inc,
               n_hidden=h, n_code=c, **{k: (list(v) if isinstance(v, tuple) else v)
                                        for k, v in model_kw.items()})
    for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", m.disc)):
        for k, v in state_np(net).items():
            out[f"init.{net_name}.{k}"] = v
    if init_scale:
        cfg["init_scale"] = {k: float(f) for k, f in init_scale.items()}
    if init_from:
        base = np.load(os.path.join(OUT, init_from + ".npz"))
        for k in [k for k in out if k.startswith("init.")]:
            want = base[k] * np.float32((init_scale or {}).get(k[len("init."):], 1.0))
            assert want.dtype == np.float32 and np.array_equal(out[k], want), (init_from, k)
            del out[k]
        cfg["init_from"] = init_from
    if state_keys:
        cfg["state_keys"] = dict(every=list(state_keys["every"]), last=list(state_keys["last"]))
    order = {n: [k for k, _ in net.named_parameters()] for n, net in (("enc", m.enc), ("dec", m.dec), ("disc", m.disc))}
    if any(len(v) != 6 for v in order.values()):      # an activation with parameters (PReLU): what index i of A_*.<i>.m names
        cfg["param_order"] = order

    if cond in CAT_KINDS:
        # fit the vocabulary on all raw inputs first (AAERecommender.train -> fit_transform)
        raw_all = [[f"a{int(x)}" for x in rng.integers(0, 12, size=int(rng.integers(1, 4)))]
                   for _ in range(B * steps)]
        if kind["reduce"] is None:
            raw_all = [r[0] for r in raw_all]
        cc.fit(raw_all)
        cdata = cc.transform(raw_all)
        out["init.cond.embedding"] = cc.embedding.weight.detach().numpy().copy()
        cfg["cat"] = dict(kind, lr=1e-2)
    if cond in BAG_KINDS:
        out["init.cond.embedding"] = bag.embedding_bag.weight.detach().numpy().copy()
        cfg["bag"] = dict(num_embeddings=BAG_VOCAB, dim=BAG_DIM, mode=bag.embedding_bag.mode, kwargs=BAG_KINDS[cond],
                          lr=bag.optimizer.param_groups[0]["lr"])
        bag_block = lambda n: rng.integers(0, BAG_VOCAB, size=(n, BAG_WIDTH)).astype(np.int64)      # noqa: E731

    acts = {}
    if capture_acts:
        def hook(tag):
            def fn(mod, inp, outp):
                acts.setdefault(tag, []).append(outp.detach().numpy().copy())
            return fn
        m.enc.lin1.register_forward_hook(hook("enc_a1"))
        m.enc.register_forward_hook(hook("enc_z"))
        m.dec.register_forward_hook(hook("dec_xhat"))

    for s in range(steps):
        Bs = last_B if (last_B is not None and s == steps - 1) else B
        X = make_batch(rng, Bs, N, **(batch_kw or {}))
        out[f"step{s}.indptr"] = X.indptr.astype(np.int64)
        out[f"step{s}.indices"] = X.indices.astype(np.int32)
        out[f"step{s}.values"] = X.data.astype(np.float32)
        cbatch = None
        if concat_w:
            cv = (rng.standard_normal((Bs, concat_w)) * (0.5 if concat_w <= 30 else 0.1)).astype(np.float32)
            out[f"step{s}.cond0"] = cv
            cbatch = [cv]
        elif cond == "concat30+bias":
            cv = (rng.standard_normal((Bs, 30)) * 0.5).astype(np.float32)
            bv = (rng.standard_normal((Bs, c + 30)) * 0.1).astype(np.float32)
            out[f"step{s}.cond0"] = cv
            out[f"step{s}.cond1"] = bv
            cbatch = [cv, bv]
        elif cond in CAT_KINDS:
            lists = cdata[s * B: s * B + Bs]
            cbatch = [lists]
            if kind["concat"]:
                cv = (rng.standard_normal((Bs, 30)) * 0.5).astype(np.float32)
                out[f"step{s}.cond0"] = cv
                cbatch = [cv, lists]
            out[f"step{s}.cond{len(cbatch) - 1}"] = _pad_lists(lists)
        elif cond in BAG_KINDS:
            out[f"step{s}.cond0"] = bag_block(Bs)
            cbatch = [torch.from_numpy(out[f"step{s}.cond0"])]
        n_masks0, n_z0 = len(masks_log), len(z_log)
        m.partial_fit(X.toarray(), condition_data=cbatch, step=s)
        out[f"step{s}.losses"] = np.asarray(loss_log[-1], dtype=np.float64)
        out[f"step{s}.z_real"] = z_log[n_z0]
        for j, (tag, mk) in enumerate(masks_log[n_masks0:]):
            out[f"step{s}.mask{j}"] = mk
            cfg.setdefault("mask_order", []).append(tag) if s == 0 else None
        if states == 'last' and s != steps - 1:
            continue
        keep = None
        if state_keys:
            keep = set(state_keys["every"]) | (set(state_keys["last"]) if s == steps - 1 else set())
        for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", m.disc)):
            for k, v in state_np(net).items():
                if keep is None or f"{net_name}.{k}" in keep:
                    out[f"step{s}.{net_name}.{k}"] = v
        ep, dp, xp = list(m.enc.parameters()), list(m.dec.parameters()), list(m.disc.parameters())
        for tag, net_name, opt, ps in (("A_enc", "enc", m.enc_optim, ep), ("A_dec", "dec", m.dec_optim, dp),
                                       ("A_gen", "enc", m.gen_optim, ep), ("A_disc", "disc", m.disc_optim, xp)):
            for k, v in optim_np(opt, ps).items():
                if state_keys is None or f"{net_name}.{ENC_KEYS[int(k.split('.')[0])]}" in state_keys["adam"]:
                    out[f"step{s}.{tag}.{k}"] = v
        if cond in CAT_KINDS:
            out[f"step{s}.cond.embedding"] = cc.embedding.weight.detach().numpy().copy()
            st = cc.optimizer.state[cc.embedding.weight]
            out[f"step{s}.cond.m"] = st["exp_avg"].numpy().copy()
            out[f"step{s}.cond.v"] = st["exp_avg_sq"].numpy().copy()
            out[f"step{s}.cond.t"] = np.asarray(float(st["step"]))
        if cond in BAG_KINDS:
            bag_record(out, f"step{s}", bag)
        if capture_acts and s == 0:
            # forward order inside partial_fit: ae (train), disc (eval), gen (train)
            out["step0.act.enc_a1_ae"] = acts["enc_a1"][0]
            out["step0.act.enc_z_ae"] = acts["enc_z"][0]
            out["step0.act.dec_xhat"] = acts["dec_xhat"][0]
            out["step0.act.enc_z_disc"] = acts["enc_z"][1]
            out["step0.act.enc_z_gen"] = acts["enc_z"][2]

    # predict with the trained model on the last batch (eval mode; aae.py:840-870)
    Xp = make_batch(rng, predict_B or B, N, **(batch_kw or {}))
    out["predict.indptr"] = Xp.indptr.astype(np.int64)
    out["predict.indices"] = Xp.indices.astype(np.int32)
    out["predict.values"] = Xp.data.astype(np.float32)
    pc = None
    if concat_w:
        pcv = (rng.standard_normal((B, concat_w)) * (0.5 if concat_w <= 30 else 0.1)).astype(np.float32)
        out["predict.cond0"] = pcv
        pc = [pcv]
    elif cond == "concat30+bias":
        pcv = (rng.standard_normal((B, 30)) * 0.5).astype(np.float32)
        pbv = (rng.standard_normal((B, c + 30)) * 0.1).astype(np.float32)
        out["predict.cond0"], out["predict.cond1"] = pcv, pbv
        pc = [pcv, pbv]
    elif cond in CAT_KINDS:
        lists = cdata[:B]
        pc = [lists]
        if kind["concat"]:
            pcv = (rng.standard_normal((B, 30)) * 0.5).astype(np.float32)
            out["predict.cond0"] = pcv
            pc = [pcv, lists]
        out[f"predict.cond{len(pc) - 1}"] = _pad_lists(lists)
    elif cond in BAG_KINDS:
        out["predict.cond0"] = bag_block(predict_B or B)
        pc = [torch.from_numpy(out["predict.cond0"])]
    m.batch_size = 7   # exercises the ragged last predict batch
    out["predict.out"] = m.predict(Xp, condition_data=pc).astype(np.float32)
    if finish is not None:
        finish(out, cfg, logits_log[:steps])
    out["config_json"] = np.asarray(json.dumps(cfg))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB, "
          f"losses step0={out['step0.losses']}")
    return out


def run_ae_only_case(ref_aae, name, N=300, h=20, c=10, B=16, steps=3, seed=0, dropout=(0.2, 0.2), lr=2e-3):
    """The reference's plain AutoEncoder (aae.py:221-458): ae_step only, one learning rate."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(2000 + seed)
    m = ref_aae.AutoEncoder(n_hidden=h, n_code=c, lr=lr, batch_size=B, n_epochs=1, dropout=dropout, verbose=True)
    m.enc = ref_aae.Encoder(N, h, c, final_activation='linear', normalize_inputs=m.normalize_inputs,
                            dropout=m.dropout, activation=m.activation)
    m.dec = ref_aae.Decoder(c, h, N, dropout=m.dropout, activation=m.activation)
    og = ref_aae.TORCH_OPTIMIZERS[m.optimizer]
    m.enc_optim, m.dec_optim = og(m.enc.parameters(), lr=m.lr), og(m.dec.parameters(), lr=m.lr)
    masks_log = []
    for net_name, net in (("enc", m.enc), ("dec", m.dec)):
        for li, attr in enumerate(("drop1", "drop2")):
            setattr(net, attr, RecDropout(m.dropout[li], masks_log, f"{net_name}.{attr}"))
    loss_log = []
    ref_aae.log_losses = lambda *l: loss_log.append(l)
    ref_aae.USE_WANDB = False
    out = {}
    cfg = dict(N=N, h=h, c=c, B=B, steps=steps, cond="", cond_inc=0, n_hidden=h, n_code=c, ae_only=1,
               gen_lr=lr, reg_lr=lr, dropout=list(dropout))
    for net_name, net in (("enc", m.enc), ("dec", m.dec)):
        for k, v in state_np(net).items():
            out[f"init.{net_name}.{k}"] = v
    # the kernels' model always has a discriminator; give it fixed (unused) weights
    disc = ref_aae.Discriminator(c, h)
    for k, v in state_np(disc).items():
        out[f"init.disc.{k}"] = v
    for s in range(steps):
        X = make_batch(rng, B, N)
        out[f"step{s}.indptr"] = X.indptr.astype(np.int64)
        out[f"step{s}.indices"] = X.indices.astype(np.int32)
        out[f"step{s}.values"] = X.data.astype(np.float32)
        n0 = len(masks_log)
        m.partial_fit(X.toarray(), step=s)
        out[f"step{s}.losses"] = np.asarray(loss_log[-1], dtype=np.float64)
        out[f"step{s}.z_real"] = np.zeros((B, c), dtype=np.float32)
        for j, (tag, mk) in enumerate(masks_log[n0:]):
            out[f"step{s}.mask{j}"] = mk
        for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", disc)):
            for k, v in state_np(net).items():
                out[f"step{s}.{net_name}.{k}"] = v
        ep, dp = list(m.enc.parameters()), list(m.dec.parameters())
        for tag, opt, ps in (("A_enc", m.enc_optim, ep), ("A_dec", m.dec_optim, dp)):
            for k, v in optim_np(opt, ps).items():
                out[f"step{s}.{tag}.{k}"] = v
    Xp = make_batch(rng, B, N)
    out["predict.indptr"] = Xp.indptr.astype(np.int64)
    out["predict.indices"] = Xp.indices.astype(np.int32)
    out["predict.values"] = Xp.data.astype(np.float32)
    out["predict.out"] = m.predict(Xp).astype(np.float32)
    out["config_json"] = np.asarray(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: losses step0={out['step0.losses']}")


def run_decoding_case(ref_aae, ref_cond, name, N=300, h=20, B=16, steps=3, seed=0, dropout=(0.2, 0.2), lr=2e-3,
                      incs=(12, 8), trainable=False):
    """The reference's DecodingRecommender (aae.py:461-584): conditions -> 3-layer decoder -> BCE against the
    item rows.  Conditions: constant concatenated blocks (first one is the base input, the others are imposed,
    aae.py:494-502); trainable=True makes the first one a CategoricalCondition (embedding sum, own optimiser)."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(3000 + seed)

    def const_concat(inc):
        class ConstConcat(ref_cond.ConcatenationBasedConditioning):
            def size_increment(self):
                return inc

            def encode(self, inputs):
                return torch.as_tensor(inputs, dtype=torch.float32)
        return ConstConcat()
    items = []
    if trainable:
        items.append(("authors", ref_cond.CategoricalCondition(incs[0], sparse=False, use_cuda=False, reduce="sum",
                                                                lr=1e-2)))
    else:
        items.append(("title", const_concat(incs[0])))
    for j, inc in enumerate(incs[1:]):
        items.append((f"c{j}", const_concat(inc)))
    conditions = ref_cond.ConditionList(items)
    vocab = 40
    if trainable:
        conditions["authors"].fit([[f"a{i}"] for i in range(vocab)])
    m = ref_aae.DecodingRecommender(conditions, n_epochs=1, batch_size=B, n_hidden=h, lr=lr, verbose=False,
                                    dropout=dropout)
    m.mlp = ref_aae.Decoder(conditions.size_increment(), h, N, **m.model_params)
    m.mlp_optim = ref_aae.TORCH_OPTIMIZERS[m.optimizer](m.mlp.parameters(), lr=m.lr)
    masks_log = []
    for li, attr in enumerate(("drop1", "drop2")):
        setattr(m.mlp, attr, RecDropout(dropout[li], masks_log, f"dec.{attr}"))
    ref_aae.USE_WANDB = False
    losses = []
    orig_bce = ref_aae.F.binary_cross_entropy

    def rec_bce(*a, **k):
        out = orig_bce(*a, **k)
        losses.append(float(out.detach()))
        return out
    out = {}
    cfg = dict(N=N, h=h, c=int(conditions.size_increment()), B=B, steps=steps, cond="", cond_inc=0, n_hidden=h,
               n_code=int(conditions.size_increment()), decoder_only=1, incs=list(incs), trainable=int(trainable),
               gen_lr=lr, reg_lr=lr, dropout=list(dropout), vocab=vocab)
    for k, v in state_np(m.mlp).items():
        out[f"init.dec.{k}"] = v
    if trainable:
        out["init.cond.embedding"] = conditions["authors"].embedding.weight.detach().numpy().copy()

    def cond_batch(n):
        cb = []
        if trainable:
            raw = [[f"a{int(i)}" for i in rng.integers(0, vocab, size=int(rng.integers(1, 4)))] for _ in range(n)]
            cb.append(conditions["authors"].transform(raw))       # list of index lists (0 = padding / unknown)
        else:
            cb.append(rng.normal(size=(n, incs[0])).astype(np.float32))
        for inc in incs[1:]:
            cb.append(rng.normal(size=(n, inc)).astype(np.float32))
        return cb

    def save_cond(prefix, cb):
        for j, x in enumerate(cb):
            if trainable and j == 0:
                L = max(len(l) for l in x)      # padded exactly as CategoricalCondition._pad_batch does
                out[f"{prefix}.cond{j}"] = np.asarray([l + [0] * (L - len(l)) for l in x], dtype=np.int64)
            else:
                out[f"{prefix}.cond{j}"] = np.asarray(x, dtype=np.float32)
    ref_aae.F.binary_cross_entropy = rec_bce
    try:
        for s in range(steps):
            Y = make_batch(rng, B, N)
            cb = cond_batch(B)
            out[f"step{s}.indptr"] = Y.indptr.astype(np.int64)
            out[f"step{s}.indices"] = Y.indices.astype(np.int32)
            out[f"step{s}.values"] = Y.data.astype(np.float32)
            save_cond(f"step{s}", cb)
            n0 = len(masks_log)
            m.partial_fit(cb, torch.FloatTensor(Y.toarray()), step=s)
            out[f"step{s}.losses"] = np.asarray([losses[-1], 0.0, 0.0], dtype=np.float64)
            for j, (tag, mk) in enumerate(masks_log[n0:]):
                out[f"step{s}.mask{j}"] = mk
            for k, v in state_np(m.mlp).items():
                out[f"step{s}.dec.{k}"] = v
            for k, v in optim_np(m.mlp_optim, list(m.mlp.parameters())).items():
                out[f"step{s}.A_dec.{k}"] = v
            if trainable:
                out[f"step{s}.cond.embedding"] = conditions["authors"].embedding.weight.detach().numpy().copy()
    finally:
        ref_aae.F.binary_cross_entropy = orig_bce
    # predict (aae.py:560-583) on a fresh condition batch
    cb = cond_batch(B)
    save_cond("predict", cb)
    m.mlp.eval()
    conditions.eval()
    with torch.no_grad():
        enc = conditions.encode(cb)
        inputs = enc[0]
        for cnd, cd in zip(list(conditions.values())[1:], enc[1:]):
            inputs = cnd.impose(inputs, cd)
        out["predict.out"] = m.mlp(inputs).numpy().astype(np.float32)
    out["config_json"] = np.asarray(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: losses {[round(l, 6) for l in losses]}")


def gen_metric_known_answers():
    """Known answers for the metric side, produced by calling the reference's own
    evaluation functions on literal inputs (evaluation.py:94-115,183-199)."""
    import aaerec.evaluation as ev
    rng = np.random.default_rng(7)
    y_true = (rng.random((40, 60)) < 0.08).astype(np.float64)
    y_pred = rng.random((40, 60))
    x_test = (rng.random((40, 60)) < 0.05).astype(np.float64)
    out = {"y_true": y_true, "y_pred": y_pred, "x_test": x_test}
    out["removed"] = ev.remove_non_missing(y_pred, sp.csr_matrix(x_test), copy=True)
    for key in ("mrr", "mrr@5", "mrr@10", "map", "map@10", "P@1", "P@5", "P@10"):
        if key in ev.METRICS:
            mean, std = ev.METRICS[key](y_true, out["removed"])
            out["metric." + key] = np.asarray([mean, std])
    np.savez_compressed(os.path.join(OUT, "metrics.npz"), **out)
    print("metrics:", {k: v for k, v in out.items() if k.startswith("metric.")})


def gen_e2e_c1(ref_aae):
    """Config C1 end to end on the reference: prototype-set generator,
    Evaluation-free (direct train/predict on CSR) so the same spec runs on our side.
    Stores the spec + the reference's MRR@10 (mean over docs)."""
    import aaerec.evaluation as ev
    rng = np.random.RandomState(42)
    N, n_proto, n_docs = 1000, 100, 2000
    protos = [rng.choice(N, size=10, replace=False) for _ in range(n_proto)]
    docs = []
    for _ in range(n_docs):
        p = protos[rng.randint(n_proto)]
        k = rng.randint(6, 10)
        docs.append(sorted(rng.choice(p, size=k, replace=False).tolist()))
    n_test = 200
    train, test = docs[:-n_test], docs[-n_test:]
    # hide one item of every test doc
    test_in, test_out = [], []
    for d in test:
        j = rng.randint(len(d))
        test_out.append([d[j]])
        test_in.append(d[:j] + d[j + 1:])

    def csr(rows):
        i0 = [b for b, r in enumerate(rows) for _ in r]
        i1 = [i for r in rows for i in r]
        return sp.coo_matrix((np.ones(len(i0)), (i0, i1)), shape=(len(rows), N)).tocsr()

    Xtr, Xin, Yout = csr(train), csr(test_in), csr(test_out)
    mrrs = []
    for seed in range(8):
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = ref_aae.AdversarialAutoEncoder(n_hidden=50, n_code=50, n_epochs=100, batch_size=100,
                                           gen_lr=0.01, reg_lr=0.001, verbose=False)
        m.fit(Xtr)
        pred = m.predict(Xin)
        pred = ev.remove_non_missing(pred, Xin, copy=True)
        mean, std = ev.METRICS["mrr@10"](Yout.toarray(), pred)
        mrrs.append(mean)
        print("e2e_c1 seed", seed, "MRR@10", mean)
    # short run: the reference's predictions after 3 epochs pin the whole fit() pipeline
    # (initialisation order, shuffling, batching incl. the short last batch, dropout/prior draws)
    torch.manual_seed(7)
    np.random.seed(7)
    m = ref_aae.AdversarialAutoEncoder(n_hidden=50, n_code=50, n_epochs=3, batch_size=100,
                                       gen_lr=0.01, reg_lr=0.001, verbose=False)
    m.fit(Xtr)
    pred_short = m.predict(Xin[:40]).astype(np.float32)
    out = dict(pred_short=pred_short, short_seed=np.asarray(7),
               train_indptr=Xtr.indptr, train_indices=Xtr.indices,
               in_indptr=Xin.indptr, in_indices=Xin.indices,
               out_indptr=Yout.indptr, out_indices=Yout.indices,
               N=np.asarray(N), ref_mrr10=np.asarray(mrrs))
    np.savez_compressed(os.path.join(OUT, "e2e_c1.npz"), **out)
    # the plain AutoEncoder (aae.py:221-458) on the same data, 3 epochs, for tests/test_host_gpu.py
    torch.manual_seed(7)
    np.random.seed(7)
    ae = ref_aae.AutoEncoder(n_hidden=50, n_code=50, n_epochs=3, batch_size=100, lr=0.01, verbose=False)
    ae.fit(Xtr)
    np.savez_compressed(os.path.join(OUT, "e2e_ae_short.npz"), pred_short=ae.predict(Xin[:40]).astype(np.float32),
                        seed=np.asarray(7))


def gen_e2e_c1_big(ref_aae, n_seeds=16):
    """A config-C1-shaped end-to-end run sized so that MRR@10 parity at the north star's +-0.001 is a meaningful
    statement: 1 000 items in 100 prototype sets, 4 000 training docs, 10 000 test docs (one hidden item
    each: sampling s.e. of a mean reciprocal rank ~0.003), and a recipe that CONVERGES - dropout (0, 0), 120 epochs of
    40 steps, gen_lr 0.01 - so that the reference's own seed-to-seed spread is ~3e-4 instead of the 0.05 of e2e_c1.
    Stores the corpus, the reference's MRR@10 per seed and its predictions after 3 epochs (seed 7) for the first 200
    test docs."""
    import aaerec.evaluation as ev
    rng = np.random.RandomState(4242)
    N, n_proto, n_train, n_test = 1000, 100, 4000, 10000
    protos = [rng.choice(N, size=10, replace=False) for _ in range(n_proto)]
    docs = []
    for _ in range(n_train + n_test):
        p = protos[rng.randint(n_proto)]
        k = rng.randint(6, 10)
        docs.append(sorted(rng.choice(p, size=k, replace=False).tolist()))
    train, test = docs[:n_train], docs[n_train:]
    test_in, test_out = [], []
    for d in test:
        j = rng.randint(len(d))
        test_out.append([d[j]])
        test_in.append(d[:j] + d[j + 1:])

    def csr(rows):
        i0 = [b for b, r in enumerate(rows) for _ in r]
        i1 = [i for r in rows for i in r]
        return sp.coo_matrix((np.ones(len(i0)), (i0, i1)), shape=(len(rows), N)).tocsr()

    Xtr, Xin, Yout = csr(train), csr(test_in), csr(test_out)
    Y = Yout.toarray()
    kw = dict(n_hidden=50, n_code=50, batch_size=100, gen_lr=0.01, reg_lr=0.001, dropout=(0., 0.), verbose=False)
    mrrs = []
    for seed in range(n_seeds):
        torch.manual_seed(seed)
        np.random.seed(seed)
        m = ref_aae.AdversarialAutoEncoder(n_epochs=120, **kw)
        m.fit(Xtr)
        pred = ev.remove_non_missing(m.predict(Xin), Xin, copy=True)
        mean, _ = ev.METRICS["mrr@10"](Y, pred)
        mrrs.append(mean)
        print("e2e_c1_big seed", seed, "MRR@10", mean, flush=True)
    torch.manual_seed(7)
    np.random.seed(7)
    m = ref_aae.AdversarialAutoEncoder(n_epochs=3, **kw)
    m.fit(Xtr)
    pred_short = m.predict(Xin[:200]).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "e2e_c1_big.npz"), pred_short=pred_short, short_seed=np.asarray(7),
                        train_indptr=Xtr.indptr, train_indices=Xtr.indices, in_indptr=Xin.indptr, in_indices=Xin.indices,
                        out_indptr=Yout.indptr, out_indices=Yout.indices, N=np.asarray(N), ref_mrr10=np.asarray(mrrs),
                        recipe=np.asarray(json.dumps(dict(kw, n_epochs=120, dropout=[0., 0.]))))


def gen_e2e_c3(ref_aae, n_epochs=3, out_name="e2e_c3.npz", gen_lr=0.001):
    """The ranking check at config C3's SHAPE (SURVEY 8d "scale the same recipe for the C3 MRR check"):
    |items| = 100 000, hidden 200, code 50, batch 100 - the benchmark's layer sizes (3 125 item tiles in the output layer,
    13-block layer chains) - on a prototype-structured corpus small enough for the reference to train on the build
    container's CPU in about a minute: 200 prototype sets of 10 items drawn from the 100 000, 2 000 training docs (6-9
    items of one prototype each), 200 test docs with one item hidden, n_epochs x 20 steps at the reference's default
    learning rates without dropout (every draw is then the weight initialisation, the epoch permutations and z_real:
    replayed by rng_mode='reference').  (gen_lr = 0.01, the C1 recipe's rate, is no use at this width: 200 weights per
    logit moving by 0.01 per step drive every sigmoid to exactly 0 within the first epoch - the reference's own MRR@10 is
    0.0 after 1, 2 and 3 epochs - and the recovery out of that saturated state is decided by rounding.)
    The [200, 100 000] prediction matrix stays here (80 MB); the fixture holds what the reference's evaluation makes of it -
    evaluation.remove_non_missing + argtopk (evaluation.py:183-199, 20-58): the 12 best items per test doc with their
    scaled scores, MRR@10 / MAP@10 / P@5 - plus the raw sigmoid outputs at 32 probe items per doc."""
    import aaerec.evaluation as ev
    rng = np.random.RandomState(31337)
    N, n_proto, n_train, n_test = 100000, 200, 2000, 200
    protos = [rng.choice(N, size=10, replace=False) for _ in range(n_proto)]
    docs = []
    for _ in range(n_train + n_test):
        p = protos[rng.randint(n_proto)]
        k = rng.randint(6, 10)
        docs.append(sorted(rng.choice(p, size=k, replace=False).tolist()))
    train, test = docs[:n_train], docs[n_train:]
    test_in, test_out = [], []
    for d in test:
        j = rng.randint(len(d))
        test_out.append([d[j]])
        test_in.append(d[:j] + d[j + 1:])

    def csr(rows):
        i0 = [b for b, r in enumerate(rows) for _ in r]
        i1 = [i for r in rows for i in r]
        return sp.coo_matrix((np.ones(len(i0)), (i0, i1)), shape=(len(rows), N)).tocsr()

    Xtr, Xin, Yout = csr(train), csr(test_in), csr(test_out)
    kw = dict(n_hidden=200, n_code=50, batch_size=100, gen_lr=gen_lr, reg_lr=0.001, dropout=(0., 0.), verbose=False)
    seed = 11
    torch.manual_seed(seed)
    np.random.seed(seed)
    import time
    t0 = time.time()
    m = ref_aae.AdversarialAutoEncoder(n_epochs=n_epochs, **kw)
    m.fit(Xtr)
    raw = m.predict(Xin).astype(np.float32)
    print("e2e_c3: reference fit + predict", round(time.time() - t0, 1), "s", flush=True)
    pred = ev.remove_non_missing(raw, Xin, copy=True)
    Y = Yout.toarray()
    metrics = {name: [float(v) for v in ev.METRICS[name](Y, pred)] for name in ("mrr@10", "map@10", "p@5")}
    print("e2e_c3 reference metrics", metrics, flush=True)
    top_idx = np.asarray(ev.argtopk(pred, 12)[1])
    top_val = np.take_along_axis(pred, top_idx, axis=1).astype(np.float32)
    probe = np.stack([np.concatenate([Yout[i].indices[:1], rng.choice(N, size=31, replace=False)]) for i in range(n_test)]).astype(np.int32)
    probe_raw = np.take_along_axis(raw, probe, axis=1).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, out_name), seed=np.asarray(seed), N=np.asarray(N), n_epochs=np.asarray(n_epochs),
                        train_indptr=Xtr.indptr, train_indices=Xtr.indices, in_indptr=Xin.indptr, in_indices=Xin.indices,
                        out_indptr=Yout.indptr, out_indices=Yout.indices, top_idx=top_idx.astype(np.int32), top_val=top_val,
                        probe=probe, probe_raw=probe_raw, metrics=np.asarray(json.dumps(metrics)),
                        row_min=raw.min(1).astype(np.float32), row_max=raw.max(1).astype(np.float32),
                        recipe=np.asarray(json.dumps(dict(kw, n_epochs=n_epochs, dropout=[0., 0.]))))


def gen_dae():
    """The reference's DenoisingAutoEncoder (dae.py:144-314), corrupt='zeros' (its default): the batch tensor is
    thinned IN PLACE by zeros_noise (dae.py:48-52), so encoder input and BCE target are both the thinned batch.
    step_dae.npz: three recorded steps (per-entry keep flags, dropout masks, losses, parameters, Adam state);
    e2e_dae_short.npz: 3 epochs of DenoisingAutoEncoder.fit on the C1 corpus -> predictions."""
    import_reference()
    import aaerec.dae as ref_dae
    N, h, c, B, steps, seed, lr, nf, dropout = 300, 20, 10, 16, 3, 41, 2e-3, 0.3, (0.2, 0.2)
    rng = np.random.default_rng(seed)
    torch.manual_seed(4000 + seed)
    m = ref_dae.DenoisingAutoEncoder(n_hidden=h, n_code=c, lr=lr, batch_size=B, n_epochs=1, dropout=dropout,
                                     noise_factor=nf, corrupt='zeros', verbose=True)
    m.enc = ref_dae.Encoder(N, h, c, final_activation='linear', normalize_inputs=m.normalize_inputs,
                            dropout=m.dropout, activation=m.activation)
    m.dec = ref_dae.Decoder(c, h, N, dropout=m.dropout, activation=m.activation)
    og = ref_dae.TORCH_OPTIMIZERS[m.optimizer]
    m.enc_optim, m.dec_optim = og(m.enc.parameters(), lr=m.lr), og(m.dec.parameters(), lr=m.lr)
    masks_log, corrupted, loss_log = [], [], []
    for net_name, net in (("enc", m.enc), ("dec", m.dec)):
        for li, attr in enumerate(("drop1", "drop2")):
            setattr(net, attr, RecDropout(m.dropout[li], masks_log, f"{net_name}.{attr}"))
    orig_corrupt = m.corrupt

    def rec_corrupt(batch, noise_factor):
        out = orig_corrupt(batch, noise_factor)
        corrupted.append(out.detach().numpy().copy())
        return out
    m.corrupt = rec_corrupt
    ref_dae.log_losses = lambda *l: loss_log.append(l)
    out = {}
    cfg = dict(N=N, h=h, c=c, B=B, steps=steps, cond="", cond_inc=0, n_hidden=h, n_code=c, ae_only=1, gen_lr=lr,
               reg_lr=lr, dropout=list(dropout), noise_factor=nf, corrupt="zeros")
    import aaerec.aae as ref_aae
    disc = ref_aae.Discriminator(c, h)            # the kernels' model always carries one (unused here)
    for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", disc)):
        for k, v in state_np(net).items():
            out[f"init.{net_name}.{k}"] = v
    for s in range(steps):
        X = make_batch(rng, B, N, max_len=12)
        out[f"step{s}.indptr"] = X.indptr.astype(np.int64)
        out[f"step{s}.indices"] = X.indices.astype(np.int32)
        out[f"step{s}.values"] = X.data.astype(np.float32)
        n0 = len(masks_log)
        m.partial_fit(X.toarray())
        C = corrupted[-1]
        rows = np.repeat(np.arange(B), np.diff(X.indptr))
        out[f"step{s}.keep"] = (C[rows, X.indices] != 0).astype(np.uint8)       # per CSR entry
        assert np.count_nonzero(C) == int(out[f"step{s}.keep"].sum())           # noise only removes entries
        out[f"step{s}.losses"] = np.asarray(loss_log[-1], dtype=np.float64)
        out[f"step{s}.z_real"] = np.zeros((B, c), dtype=np.float32)
        for j, (tag, mk) in enumerate(masks_log[n0:]):
            out[f"step{s}.mask{j}"] = mk
        for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", disc)):
            for k, v in state_np(net).items():
                out[f"step{s}.{net_name}.{k}"] = v
        ep, dp = list(m.enc.parameters()), list(m.dec.parameters())
        for tag, opt, ps in (("A_enc", m.enc_optim, ep), ("A_dec", m.dec_optim, dp)):
            for k, v in optim_np(opt, ps).items():
                out[f"step{s}.{tag}.{k}"] = v
    Xp = make_batch(rng, B, N)
    out["predict.indptr"] = Xp.indptr.astype(np.int64)
    out["predict.indices"] = Xp.indices.astype(np.int32)
    out["predict.values"] = Xp.data.astype(np.float32)
    out["predict.out"] = m.predict(Xp).astype(np.float32)
    out["config_json"] = np.asarray(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, "step_dae.npz"), **out)
    print("step_dae: losses", [l[0] for l in loss_log], "kept", [int(out[f'step{s}.keep'].sum()) for s in range(steps)],
          "of", [len(out[f'step{s}.keep']) for s in range(steps)])
    # 3 epochs of fit() on the C1 corpus (tests/golden/e2e_c1.npz holds it)
    z = np.load(os.path.join(OUT, "e2e_c1.npz"))
    Nc = int(z["N"])

    def csr(ip, idx):
        return sp.csr_matrix((np.ones(len(idx)), idx, ip), shape=(len(ip) - 1, Nc))
    Xtr, Xin = csr(z["train_indptr"], z["train_indices"]), csr(z["in_indptr"], z["in_indices"])
    torch.manual_seed(7)
    np.random.seed(7)
    d = ref_dae.DenoisingAutoEncoder(n_hidden=50, n_code=50, n_epochs=3, batch_size=100, lr=0.01, verbose=False)
    d.fit(Xtr)
    np.savez_compressed(os.path.join(OUT, "e2e_dae_short.npz"), pred_short=d.predict(Xin[:40]).astype(np.float32),
                        seed=np.asarray(7))
    print("e2e_dae_short written")


def gen_dae_gauss():
    """DenoisingAutoEncoder(corrupt='gauss') (dae.py:40-45, 191): the encoder input is the dense batch + N(0, noise_factor)
    on ALL N columns (recorded), the BCE target the clean batch.  step_dae_gauss.npz: three recorded steps."""
    import_reference()
    import aaerec.dae as ref_dae
    import aaerec.aae as ref_aae
    N, h, c, B, steps, seed, lr, nf, dropout = 300, 20, 10, 16, 3, 43, 2e-3, 0.2, (0.2, 0.2)
    rng = np.random.default_rng(seed)
    torch.manual_seed(4000 + seed)
    m = ref_dae.DenoisingAutoEncoder(n_hidden=h, n_code=c, lr=lr, batch_size=B, n_epochs=1, dropout=dropout,
                                     noise_factor=nf, corrupt='gauss', verbose=True)
    m.enc = ref_dae.Encoder(N, h, c, final_activation='linear', normalize_inputs=m.normalize_inputs,
                            dropout=m.dropout, activation=m.activation)
    m.dec = ref_dae.Decoder(c, h, N, dropout=m.dropout, activation=m.activation)
    og = ref_dae.TORCH_OPTIMIZERS[m.optimizer]
    m.enc_optim, m.dec_optim = og(m.enc.parameters(), lr=m.lr), og(m.dec.parameters(), lr=m.lr)
    masks_log, noisy, loss_log = [], [], []
    for net_name, net in (("enc", m.enc), ("dec", m.dec)):
        for li, attr in enumerate(("drop1", "drop2")):
            setattr(net, attr, RecDropout(m.dropout[li], masks_log, f"{net_name}.{attr}"))
    orig_corrupt = m.corrupt

    def rec_corrupt(batch, noise_factor):
        clean = batch.detach().numpy().copy()
        out = orig_corrupt(batch, noise_factor)
        noisy.append(out.detach().numpy() - clean)          # the scaled noise itself
        return out
    m.corrupt = rec_corrupt
    ref_dae.log_losses = lambda *l: loss_log.append(l)
    out = {}
    cfg = dict(N=N, h=h, c=c, B=B, steps=steps, cond="", cond_inc=0, n_hidden=h, n_code=c, ae_only=1, gen_lr=lr,
               reg_lr=lr, dropout=list(dropout), noise_factor=nf, corrupt="gauss")
    disc = ref_aae.Discriminator(c, h)
    for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", disc)):
        for k, v in state_np(net).items():
            out[f"init.{net_name}.{k}"] = v
    for s in range(steps):
        X = make_batch(rng, B, N, max_len=12)
        out[f"step{s}.indptr"] = X.indptr.astype(np.int64)
        out[f"step{s}.indices"] = X.indices.astype(np.int32)
        out[f"step{s}.values"] = X.data.astype(np.float32)
        n0 = len(masks_log)
        m.partial_fit(X.toarray())
        out[f"step{s}.noise"] = noisy[-1].astype(np.float32)
        out[f"step{s}.losses"] = np.asarray(loss_log[-1], dtype=np.float64)
        out[f"step{s}.z_real"] = np.zeros((B, c), dtype=np.float32)
        for j, (tag, mk) in enumerate(masks_log[n0:]):
            out[f"step{s}.mask{j}"] = mk
        for net_name, net in (("enc", m.enc), ("dec", m.dec), ("disc", disc)):
            for k, v in state_np(net).items():
                out[f"step{s}.{net_name}.{k}"] = v
        ep, dp = list(m.enc.parameters()), list(m.dec.parameters())
        for tag, opt, ps in (("A_enc", m.enc_optim, ep), ("A_dec", m.dec_optim, dp)):
            for k, v in optim_np(opt, ps).items():
                out[f"step{s}.{tag}.{k}"] = v
    Xp = make_batch(rng, B, N)
    out["predict.indptr"] = Xp.indptr.astype(np.int64)
    out["predict.indices"] = Xp.indices.astype(np.int32)
    out["predict.values"] = Xp.data.astype(np.float32)
    out["predict.out"] = m.predict(Xp).astype(np.float32)
    out["config_json"] = np.asarray(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, "step_dae_gauss.npz"), **out)
    print("step_dae_gauss: losses", [l[0] for l in loss_log])


# (see gen_vae: each passes both oracle replays of its whole fixture, tests/test_vae_wide_cpu.py)
WIDE_SEEDS = {"step_vae_wide": 55, "step_vae_wide5": 55}
# (the same two screens, tests/test_vae_hwide_cpu.py - seed 62: float32 replay 1.6e-6 / 1.5e-6, float64 3.6e-7 / 2.0e-6 for the two
#  cases; at 63 both hold an element 1.7e-5 / 1.6e-5 off in float32 and 8.8e-6 / 1.9e-5 from exact arithmetic)
HWIDE_SEEDS = {"step_vae_hwide": 62, "step_vae_hwide_cond": 62}


def gen_vae(only=None):
    """The reference's VAE (vae.py:47-266): step_vae.npz (no condition) and step_vae_cond.npz (30-d constant
    concatenated condition): recorded eps of reparametrize(), losses (loss.item() / B as the reference logs it),
    parameters and Adam state after every step, a (stochastic: eps recorded) predict; e2e_vae_short.npz: 3
    epochs of VAE.fit on the C1 corpus and the eps-free part of the prediction pipeline (mu of the first rows).
    step_vae_wide / step_vae_wide5: a decoder input wider than one 208-column slot of the layer-chain kernel, as every driver
    of the reference builds it (main.py: CONDITIONS = a 300-d constant block, then trainable CategoricalConditions, in ONE
    ConditionList) - a constant block of 300 (900) columns + CategoricalCondition(32, reduce="sum", sparse=True) behind it:
    343 (943) columns, fc3 in two (five) k-parts, the trainable columns in the last one.  The constant block holds multiples
    of 1/8 (it compresses); both record the Adam moments after the last step only (a fixture stays well below 1 MiB)."""
    _, ref_cond = import_reference()
    import aaerec.vae as ref_vae
    names = ("fc1", "fc21", "fc22", "fc3", "fc4")

    def run(name, seed, cond, activation=None, hwide=None):
        N, h, c, B, steps, lr = 300, 20, 10, 16, 3, 2e-3
        if hwide:                  # (N, h, c, B): a hidden layer / code wider than a chain slot (step_vae_hwide*)
            N, h, c, B = hwide
        rng = np.random.default_rng(seed)
        torch.manual_seed(5000 + seed)
        conditions, inc = None, 0
        wide = cond[1] if isinstance(cond, tuple) else 0          # ("wide", columns of the constant block[, the categorical's])
        cat_dim = cond[2] if isinstance(cond, tuple) and len(cond) > 2 else 32
        if cond:
            class ConstConcat(ref_cond.ConcatenationBasedConditioning):
                def size_increment(self):
                    return wide or 30

                def encode(self, inputs):
                    return torch.as_tensor(inputs, dtype=torch.float32)
            conditions, inc = ref_cond.ConditionList([("title", ConstConcat())]), 30
        cc = cdata = None
        if cond == "cat":          # a trainable CategoricalCondition (condition.py:397-508: embedding sum + SparseAdam)
            cc = ref_cond.CategoricalCondition(8, sparse=True, use_cuda=False, reduce="sum", lr=1e-2)
            raw_all = [[f"a{int(x)}" for x in rng.integers(0, 12, size=int(rng.integers(1, 4)))] for _ in range(B * (steps + 1))]
            cc.fit(raw_all)
            cdata = cc.transform(raw_all)
            conditions, inc = ref_cond.ConditionList([("authors", cc)]), 8
        bag = None
        if cond in BAG_KINDS:      # a trainable EmbeddingBagCondition (condition.py:372-394) behind the code
            bag = ref_cond.EmbeddingBagCondition(BAG_VOCAB, BAG_DIM, **BAG_KINDS[cond])
            conditions, inc = ref_cond.ConditionList([("authors", bag)]), BAG_DIM
            bag_block = lambda: rng.integers(0, BAG_VOCAB, size=(B, BAG_WIDTH)).astype(np.int64)      # noqa: E731
        if wide:
            cc = ref_cond.CategoricalCondition(cat_dim, sparse=True, use_cuda=False, reduce="sum", lr=1e-2)
            raw_all = [[f"a{int(x)}" for x in rng.integers(0, 12, size=int(rng.integers(1, 4)))] for _ in range(B * (steps + 1))]
            cc.fit(raw_all)
            cdata = cc.transform(raw_all)
            conditions, inc = ref_cond.ConditionList([("title", ConstConcat()), ("authors", cc)]), wide + cat_dim
        adam_every = not wide and not hwide                           # (the wide cases: moments after the last step only)
        const_block = lambda: (rng.integers(-8, 9, size=(B, wide)) / 8.0).astype(np.float32)      # noqa: E731
        m = ref_vae.VAE(N, N, n_hidden=h, n_code=c, lr=lr, batch_size=B, n_epochs=1, conditions=conditions,
                        verbose=True, device=torch.device("cpu"), **(dict(activation=activation) if activation else {}))
        if hwide:
            # the reference starts from ITS initialisation rounded to multiples of 2^-12 (as the constant block holds multiples of
            # 1/8: the initial parameters are a quarter of such a fixture, and these compress)
            with torch.no_grad():
                for n in names:
                    for t in (getattr(m, n).weight, getattr(m, n).bias):
                        t.copy_(torch.round(t * 4096.0) / 4096.0)
        eps_log, loss_log = [], []
        orig_randn_like = torch.randn_like

        def rec_randn_like(*a, **k):
            e = orig_randn_like(*a, **k)
            eps_log.append(e.detach().numpy().copy())
            return e
        ref_vae.log_losses = lambda l: loss_log.append(l)
        out = {}
        cfg = dict(N=N, h=h, c=c, B=B, steps=steps, cond_inc=inc, seed=seed,
                   cond=f"concat{wide}+cat" if wide else "cat" if cc is not None else cond if bag is not None else "concat30" if cond else "",
                   n_hidden=h, n_code=c, vae=1, gen_lr=lr, reg_lr=lr, dropout=[0.0, 0.0])
        if bag is not None:
            out["init.cond.embedding"] = bag.embedding_bag.weight.detach().numpy().copy()
            cfg["bag"] = dict(num_embeddings=BAG_VOCAB, dim=BAG_DIM, mode=bag.embedding_bag.mode, kwargs=BAG_KINDS[cond],
                              lr=bag.optimizer.param_groups[0]["lr"])
        if cc is not None:
            out["init.cond.embedding"] = cc.embedding.weight.detach().numpy().copy()
            cfg["cat"] = dict(sparse=True, reduce="sum", concat=False, lr=1e-2)
        if wide:
            cfg["cat"]["dim"], cfg["concat"] = cat_dim, wide
        for n in names:
            lin = getattr(m, n)
            out[f"init.{n}.weight"] = lin.weight.detach().numpy().copy()
            out[f"init.{n}.bias"] = lin.bias.detach().numpy().copy()
        if activation:
            # (vae.py:94-96 builds the optimiser before self.act exists: a weight of the activation is in no optimiser)
            cfg["activation"] = activation
            act_params = dict(m.act.named_parameters())
            assert all(not any(p is q for g in m.optimizer.param_groups for q in g["params"]) for p in act_params.values())
            for k, v in act_params.items():
                out[f"init.act.{k}"] = v.detach().numpy().copy()
        torch.randn_like = rec_randn_like
        try:
            for s in range(steps):
                X = make_batch(rng, B, N)
                out[f"step{s}.indptr"] = X.indptr.astype(np.int64)
                out[f"step{s}.indices"] = X.indices.astype(np.int32)
                out[f"step{s}.values"] = X.data.astype(np.float32)
                cb = None
                if wide:                   # cond0 = the constant block, cond1 = the categorical's batch-padded index lists
                    cv, lists = const_block(), cdata[s * B:(s + 1) * B]
                    out[f"step{s}.cond0"], out[f"step{s}.cond1"] = cv, _pad_lists(lists)
                    cb = [cv, lists]
                elif cc is not None:
                    lists = cdata[s * B:(s + 1) * B]
                    out[f"step{s}.cond0"] = _pad_lists(lists)
                    cb = [lists]
                elif bag is not None:
                    out[f"step{s}.cond0"] = bag_block()
                    cb = [torch.from_numpy(out[f"step{s}.cond0"])]
                elif cond:
                    cv = (rng.standard_normal((B, 30)) * 0.5).astype(np.float32)
                    out[f"step{s}.cond0"] = cv
                    cb = [cv]
                m.partial_fit(X, condition_data=cb)
                if bag is not None:
                    bag_record(out, f"step{s}", bag)
                if cc is not None:
                    out[f"step{s}.cond.embedding"] = cc.embedding.weight.detach().numpy().copy()
                    st = cc.optimizer.state[cc.embedding.weight]
                    out[f"step{s}.cond.m"] = st["exp_avg"].numpy().copy()
                    out[f"step{s}.cond.v"] = st["exp_avg_sq"].numpy().copy()
                    out[f"step{s}.cond.t"] = np.asarray(float(st["step"]))
                out[f"step{s}.eps"] = eps_log[-1]
                out[f"step{s}.losses"] = np.asarray([loss_log[-1], 0.0, 0.0], dtype=np.float64)   # (BCE + KLD) / B
                if activation:
                    for k, v in m.act.named_parameters():
                        out[f"step{s}.act.{k}"] = v.detach().numpy().copy()
                params = list(m.parameters())
                for n in names:
                    lin = getattr(m, n)
                    if hwide and s != steps - 1:           # (parameters and moments after the last step only)
                        continue
                    out[f"step{s}.{n}.weight"] = lin.weight.detach().numpy().copy()
                    out[f"step{s}.{n}.bias"] = lin.bias.detach().numpy().copy()
                    for tag, t in (("weight", lin.weight), ("bias", lin.bias)):
                        if (not adam_every and s != steps - 1) or (hwide and n not in ("fc3", "fc21")):
                            continue
                        st = m.optimizer.state[t]
                        out[f"step{s}.A.{n}.{tag}.m"] = st["exp_avg"].numpy().copy()
                        out[f"step{s}.A.{n}.{tag}.v"] = st["exp_avg_sq"].numpy().copy()
                        out[f"step{s}.A.{n}.{tag}.t"] = np.asarray(float(st["step"]))
            Xp = make_batch(rng, B, N)
            out["predict.indptr"] = Xp.indptr.astype(np.int64)
            out["predict.indices"] = Xp.indices.astype(np.int32)
            out["predict.values"] = Xp.data.astype(np.float32)
            pc = None
            if wide:
                pcv, lists = const_block(), cdata[steps * B:(steps + 1) * B]
                out["predict.cond0"], out["predict.cond1"] = pcv, _pad_lists(lists)
                pc = [pcv, lists]
            elif cc is not None:
                lists = cdata[steps * B:(steps + 1) * B]
                out["predict.cond0"] = _pad_lists(lists)
                pc = [lists]
            elif bag is not None:
                out["predict.cond0"] = bag_block()
                pc = [torch.from_numpy(out["predict.cond0"])]
            elif cond:
                pcv = (rng.standard_normal((B, 30)) * 0.5).astype(np.float32)
                out["predict.cond0"] = pcv
                pc = [pcv]
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                out["predict.out"] = m.predict(Xp, condition_data=pc).astype(np.float32)
            out["predict.eps"] = eps_log[-1]
        finally:
            torch.randn_like = orig_randn_like
        out["config_json"] = np.asarray(json.dumps(cfg))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        assert os.path.getsize(os.path.join(OUT, name + ".npz")) < (1 << 20), name + ": a fixture stays below 1 MiB"
        print(f"{name}: losses {[round(float(l), 5) for l in loss_log]}")
    # The wide cases' seeds are chosen by the ORACLE alone (tests/test_vae_wide_cpu.py): Adam's first step moves an element
    # whose gradient is near its eps by up to lr whatever the arithmetic, and the wider fc3 is, the likelier one such element
    # is in it.  (a) the oracle's float32 replay of the whole fixture passes test_oracle_golden.py's tolerances (step_vae_wide
    # at seeds 52, 54, 56, 59: one fc3 element 5e-6 .. 8e-6 off after step 0); (b) so does its restatement in float64 - what
    # exact arithmetic gives, i.e. how far the reference's OWN rounding moved its most sensitive element: step_vae_wide5 at
    # seed 52 passes (a) with 1.3e-6 and has one fc3 element 1.25e-5 from exact arithmetic, at 57 1.5e-5 - no implementation
    # can be held to 1e-5 of such a number.  Seed 55: (a) 1.2e-7 / 3.2e-7, (b) 4.7e-7 / 4.7e-7 for the two cases.
    # `vae_wide:<name>:<seed>` tries another seed (into AAE_GOLDEN_OUT).
    wide_cases = {"step_vae_wide": ("step_vae_wide", WIDE_SEEDS["step_vae_wide"], ("wide", 300)),
                  "step_vae_wide5": ("step_vae_wide5", WIDE_SEEDS["step_vae_wide5"], ("wide", 900))}
    # A hidden layer and a code wider than a chain slot (cfg.vae_wide; tests/test_vae_hwide_*.py): step_vae_hwide one past both
    # bounds at once (209, 105), step_vae_hwide_cond the reference grid's hidden width (300) behind the wide cases' condition
    # scheme - a 30-column constant block + CategoricalCondition(8).  Their seeds pass the same two screens (HWIDE_SEEDS).
    wide_cases["step_vae_hwide"] = ("step_vae_hwide", HWIDE_SEEDS["step_vae_hwide"], False, None, (100, 209, 105, 17))
    wide_cases["step_vae_hwide_cond"] = ("step_vae_hwide_cond", HWIDE_SEEDS["step_vae_hwide_cond"], ("wide", 30, 8), None, (100, 300, 40, 16))
    if only:
        if isinstance(only, tuple):             # (name, seed): a scratch fixture of a wide case at another seed
            run(only[0], only[1], *wide_cases[only[0]][2:])
            return
        if isinstance(only, str) and only.startswith("step_vae_bag"):      # (step_vae_bag[:<seed>])
            run("step_vae_bag", int(only.split(":")[1]) if ":" in only else BAG_SEEDS["step_vae_bag"], "bag_sum")
            return
        run(*dict({"step_vae": ("step_vae", 51, False), "step_vae_cond": ("step_vae_cond", 52, True),
                   "step_vae_cat": ("step_vae_cat", 53, "cat"), "step_vae_prelu": ("step_vae_prelu", 54, False, "PReLU")},
                  **wide_cases)[only])
        return
    run("step_vae", 51, False)
    run("step_vae_cond", 52, True)
    run("step_vae_cat", 53, "cat")
    for case in wide_cases.values():
        if not case[0].startswith("step_vae_hwide"):       # (those two: `vae_hwide`)
            run(*case)
    # 3 epochs of fit() on the C1 corpus with the reference's seeds; predict() itself is stochastic, so the pinned
    # quantity is the encoder mean of the first rows (deterministic given the trained weights)
    z = np.load(os.path.join(OUT, "e2e_c1.npz"))
    Nc = int(z["N"])

    def csr(ip, idx):
        return sp.csr_matrix((np.ones(len(idx)), idx, ip), shape=(len(ip) - 1, Nc))
    Xtr, Xin = csr(z["train_indptr"], z["train_indices"]), csr(z["in_indptr"], z["in_indices"])
    torch.manual_seed(7)
    np.random.seed(7)
    v = ref_vae.VAE(Nc, Nc, n_hidden=50, n_code=50, n_epochs=3, batch_size=100, lr=0.01, verbose=False,
                    device=torch.device("cpu"))
    v.fit(Xtr)
    with torch.no_grad():
        x = torch.as_tensor(Xin[:40].toarray(), dtype=torch.float32)
        mu, logvar = v.encode(F.normalize(x, 1))
        recon_mu = v.decode(mu)                       # the prediction with eps = 0
    np.savez_compressed(os.path.join(OUT, "e2e_vae_short.npz"), mu=mu.numpy(), logvar=logvar.numpy(),
                        recon_mu=recon_mu.numpy().astype(np.float32), seed=np.asarray(7))
    print("e2e_vae_short written")


SAT_SCALE = 400.0           # dec.lin3.weight of step_headline's initial model times this (chosen by the search described below)
SAT_STATE_KEYS = dict(
    # N = 330, h = 200: the whole state after every step is 4.3 MB per step.  Recorded after EVERY step: every bias and the two
    # small matrices next to the output layer's gradient path (dec.lin1.weight: what da2 becomes after two layers back;
    # disc.lin3.weight), each with both Adam moments in every optimiser that owns it - a cell whose gradient is gscale where
    # the reference's is 0 shows in dec.lin3.bias's first moment at once (0.1 gscale of ~1e-5 against rtol 1e-4).
    # dec.lin3.weight itself after every step too (without its moments), enc.lin3.weight after the last.
    every=["enc.lin1.bias", "enc.lin2.bias", "enc.lin3.bias", "dec.lin1.bias", "dec.lin2.bias", "dec.lin3.bias",
           "disc.lin1.bias", "disc.lin2.bias", "disc.lin3.bias", "dec.lin1.weight", "disc.lin3.weight"],
    last=["enc.lin3.weight"])
SAT_STATE_KEYS["adam"] = list(SAT_STATE_KEYS["every"])
SAT_STATE_KEYS["every"].append("dec.lin3.weight")


def gen_saturated(ref_aae, ref_cond, scale=SAT_SCALE, seed=16, name="step_saturated"):
    """step_headline's model (same seed, shape, batches, masks) with dec.lin3.weight x `scale`: hundreds of zero-target logits
    beyond the point where the reference's fp32 sigmoid is exactly 1.0 (24 ln 2: loss 100, gradient 0), hundreds just below
    it where 1 - sigmoid is quantised in steps of 2^-23.  Asserts what the tests built on this fixture rely on and records it
    in config_json["saturation"]:
      * per step: zero-target cells with sigmoid == 1.0f / with 24 ln 2 <= l <= 25 ln 2 / with 10 < l < 24 ln 2 (each >= 50 at
        step 0), target cells below -20 and above 24 ln 2 (each >= 20 at step 0);
      * guard: no zero-target cell of any step has |l - 24 ln 2| < guard, guard = 20 x the largest |l_oracle - l_reference|
        over both steps (two independent fp32 implementations of the same step, MKL's summation order against NumPy's; a
        device's order is a third one, and at step 1 it starts from parameters that may differ by the parity tolerance) -
        a cell that close could saturate on one implementation and not on the other for no fault of either.
    The scale was searched by hand (python tools/gen_golden.py saturated:<scale>[:<seed>] writes tmp_step_saturated.npz and
    prints the figures or the failed assertion); the committed one is SAT_SCALE."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from golden_util import Fixture
    from oracle import aae_oracle as O
    CUT, CUT25 = 24 * np.log(2.0), 25 * np.log(2.0)

    def finish(out, cfg, logits):
        assert len(logits) == cfg["steps"]
        # the oracle on the recorded inputs (the replay of tests/test_oracle_golden.py)
        class _Z(dict):
            files = property(lambda self: list(self.keys()))
        fx = Fixture.__new__(Fixture)
        fx.name, fx.z, fx.cfg, fx.steps = name, _Z(out), cfg, cfg["steps"]
        ora = O.OracleAAE(fx.init_params(), **fx.model_kwargs())
        stats, diff, near = [], 0.0, np.inf
        for s, L in enumerate(logits):
            ip, idx, val = fx.batch(s)
            ora.partial_fit(ip, idx, val, out[f"step{s}.z_real"], fx.masks(s), None)
            diff = max(diff, float(np.abs(ora.last["logits"].astype(np.float64) - L).max()))
            T = np.zeros(L.shape, dtype=bool)
            T[np.repeat(np.arange(len(ip) - 1), np.diff(ip)), idx] = True
            sig = torch.sigmoid(torch.from_numpy(L)).numpy()
            Z = ~T
            stats.append(dict(zero_sigmoid_is_one=int((Z & (sig == 1.0)).sum()),
                              zero_in_band=int((Z & (L >= CUT) & (L <= CUT25)).sum()),
                              zero_10_to_cut=int((Z & (L > 10) & (L < CUT)).sum()),
                              target_below_m20=int((T & (L < -20)).sum()), target_above_cut=int((T & (L > CUT)).sum()),
                              logit_min=float(L.min()), logit_max=float(L.max())))
            near = min(near, float(np.abs(L[Z].astype(np.float64) - CUT).min()))
            # the reference's own sigmoid saturates exactly at the cut-off, on every zero-target cell of this step
            assert np.array_equal(sig[Z] == 1.0, L[Z] >= CUT), ("sigmoid == 1 is not l >= 24 ln 2", s)
        guard = 20.0 * diff
        print(f"{name}: scale {scale} per-step {stats}\n  max |l_oracle - l_reference| {diff:.3e}, guard {guard:.3e}, "
              f"nearest zero-target cell to 24 ln 2: {near:.3e}")
        s0 = stats[0]
        assert min(s0["zero_sigmoid_is_one"], s0["zero_in_band"], s0["zero_10_to_cut"]) >= 50, s0
        assert min(s0["target_below_m20"], s0["target_above_cut"]) >= 20, s0
        assert near >= guard, ("a zero-target cell inside the guard", near, guard)
        cfg["saturation"] = dict(scale=float(scale), cut=float(CUT), oracle_vs_reference_logit_diff=diff, guard=guard,
                                 nearest_zero_target_cell=near, steps=stats)

    return run_case(ref_aae, ref_cond, name, seed=seed, N=330, h=200, c=50, B=100, steps=2, dropout=(0.2, 0.2),
                    batch_kw=dict(max_len=24), capture_acts=False, states='all',
                    init_scale={"dec.lin3.weight": scale}, init_from="step_headline" if seed == 16 else None,
                    state_keys=SAT_STATE_KEYS, predict_B=32, finish=finish)


def svd_corpus(seed, n_docs=700, n_items=330, n_proto=30):
    """A small citation-like corpus with titles: documents draw most of their items from one of n_proto item pools and
    most of their title words from that pool's word list, over the years 2000-2009.  (tokens as int ids, titles as text)"""
    rng = np.random.RandomState(seed)
    pools = [rng.choice(n_items, size=14, replace=False) for _ in range(n_proto)]
    words = [["w%dx%d" % (p, j) for j in range(6)] for p in range(n_proto)]
    common = ["study", "analysis", "model", "data", "effect", "system", "method", "review"]
    docs, titles, years = [], [], []
    for i in range(n_docs):
        p = rng.randint(n_proto)
        own = rng.choice(pools[p], size=rng.randint(4, 9), replace=False).tolist()
        stray = rng.choice(n_items, size=rng.randint(0, 3), replace=False).tolist()
        docs.append(sorted(set(int(t) for t in own + stray)))
        title = rng.choice(words[p], size=rng.randint(2, 5), replace=False).tolist() + \
            rng.choice(common, size=rng.randint(1, 4), replace=False).tolist()
        if rng.rand() < 0.15:
            title += rng.choice(words[rng.randint(n_proto)], size=1).tolist()
        titles.append(" ".join(title))
        years.append(2000 + (i * 10) // n_docs)
    return docs, titles, years


def gen_svd():
    """The reference's SVDRecommender (svd.py:15-57) on the CPU behind the reference's own Bags / Evaluation.setup split
    (year 2009, min_elements 2, drop 1): svd_plain.npz (dims 12, items only) and svd_titles.npz (dims 20, use_title).
    Data only: the corpus (token ids, title strings, years), the split as the reference made it (train / test / held-out CSR,
    the titles of both sides, the item vocabulary), components_ (float64), the tf-idf vocabulary with its idf, str(model)
    and the reference's predict() output."""
    import_reference()
    import aaerec.datasets as ref_ds
    import aaerec.evaluation as ref_ev
    import aaerec.svd as ref_svd
    for name, seed, dims, use_title, random_state in (("svd_plain", 5, 12, False, 11), ("svd_titles", 6, 20, True, 12)):
        docs, titles, years = svd_corpus(seed)
        owners = ["d%d" % i for i in range(len(docs))]
        bags = ref_ds.Bags([["i%d" % t for t in d] for d in docs], owners,
                           {"year": dict(zip(owners, years)), "title": dict(zip(owners, titles))})
        ev = ref_ev.Evaluation(bags, 2009, metrics=["mrr@10"], logfile=os.devnull)
        ev.setup(seed=42, min_elements=2, drop=1)
        train_set, test_set = ev.train_set.clone(), ev.test_set.clone()
        rec = ref_svd.SVDRecommender(dims, use_title=use_title, random_state=random_state)
        rec.train(train_set)
        pred = np.asarray(rec.predict(test_set), dtype=np.float64)
        Xtr, Xte, Yte = train_set.tocsr(), sp.csr_matrix(ev.x_test), sp.csr_matrix(ev.y_test)
        for M in (Xtr, Xte, Yte):
            M.sum_duplicates()
            M.sort_indices()
        out = dict(dims=np.asarray(dims), use_title=np.asarray(int(use_title)), random_state=np.asarray(random_state),
                   split_year=np.asarray(2009), setup_seed=np.asarray(42), min_elements=np.asarray(2), drop=np.asarray(1),
                   doc_indptr=np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64),
                   doc_tokens=np.asarray([t for d in docs for t in d], dtype=np.int32),
                   doc_years=np.asarray(years, dtype=np.int32), doc_titles=np.asarray(titles),
                   item_vocab=np.asarray([train_set.index2token[i] for i in range(len(train_set.index2token))]),
                   train_indptr=Xtr.indptr.astype(np.int64), train_indices=Xtr.indices.astype(np.int32), train_data=Xtr.data.astype(np.float64),
                   test_indptr=Xte.indptr.astype(np.int64), test_indices=Xte.indices.astype(np.int32), test_data=Xte.data.astype(np.float64),
                   truth_indptr=Yte.indptr.astype(np.int64), truth_indices=Yte.indices.astype(np.int32),
                   n_items=np.asarray(Xtr.shape[1]),
                   train_titles=np.asarray(train_set.get_single_attribute("title")),
                   test_titles=np.asarray(test_set.get_single_attribute("title")),
                   components=np.asarray(rec.svd.components_, dtype=np.float64), model_str=np.asarray(str(rec)),
                   pred=pred)
        if use_title:
            terms = sorted(rec.tfidf.vocabulary_, key=rec.tfidf.vocabulary_.get)
            out.update(tfidf_terms=np.asarray(terms), tfidf_idf=np.asarray(rec.tfidf.idf_, dtype=np.float64))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, "train", Xtr.shape, "test", Xte.shape, "features", rec.svd.components_.shape[1], "bytes", os.path.getsize(path))


def gen_mi():
    """The reference's compute_mutual_info (utils.py:10-71) on a tiny synthetic Bags: 48 bags over 30 items drawn from 6 item
    pools, one title per bag from the pool's words, one CountCondition on the titles.  All three input forms - labels only,
    the condition imposed on the labels, the condition alone - normalised and not.  mutual_info.npz holds the bags as index
    lists, the titles and the six results: data only."""
    import_reference()
    import aaerec.datasets as ref_ds
    import aaerec.utils as ref_utils
    import aaerec.condition as ref_cond
    rng = np.random.RandomState(23)
    n_bags, n_items, n_pools = 48, 30, 6
    pools = [rng.choice(n_items, size=8, replace=False) for _ in range(n_pools)]
    words = [["p%dw%d" % (p, j) for j in range(4)] for p in range(n_pools)]
    raw, titles = [], []
    for _ in range(n_bags):
        p = rng.randint(n_pools)
        raw.append(["i%d" % t for t in rng.choice(pools[p], size=rng.randint(2, 7), replace=False)])
        titles.append(" ".join(rng.choice(words[p], size=rng.randint(1, 4), replace=False).tolist() +
                               rng.choice(["study", "data", "model"], size=rng.randint(0, 3), replace=False).tolist()))
    owners = ["d%d" % i for i in range(n_bags)]
    bags = ref_ds.Bags(raw, owners, {"title": dict(zip(owners, titles))}).build_vocab(apply=True)
    forms = (("labels", False, True), ("imposed", True, True), ("conditions", True, False))
    out = dict(bag_indptr=np.concatenate([[0], np.cumsum([len(b) for b in bags.data])]).astype(np.int64),
               bag_tokens=np.asarray([t for b in bags.data for t in b], dtype=np.int32), n_items=np.asarray(len(bags.vocab)),
               titles=np.asarray(titles), forms=np.asarray([f[0] for f in forms]))
    for name, with_cond, include_labels in forms:
        for normalize in (False, True):
            conditions = ref_cond.ConditionList([("title", ref_cond.CountCondition())]) if with_cond else None
            mi = ref_utils.compute_mutual_info(bags, conditions=conditions, include_labels=include_labels, normalize=normalize)
            out["mi.%s.%s" % (name, "normalized" if normalize else "raw")] = np.asarray(float(mi), dtype=np.float64)
    path = os.path.join(OUT, "mutual_info.npz")
    np.savez_compressed(path, **out)
    print("mutual_info:", {k: float(v) for k, v in out.items() if k.startswith("mi.")}, "bytes", os.path.getsize(path))


def gen_popular():
    """The reference's MostPopular (baselines.py:46-58) behind the reference's own BagsWithVocab: train on 200 bags over 120
    items (skewed popularity, a few repeated items, the last four items in no bag), predict for 9 test bags (one empty).
    most_popular.npz holds arrays only: the two sets as CSR, the counts and the prediction with their dtypes, str(model)."""
    import_reference()
    import aaerec.baselines as ref_bl
    import aaerec.datasets as ref_ds
    rng = np.random.RandomState(31)
    n_train, n_test, n_items = 200, 9, 120
    vocab = {"i%d" % i: i for i in range(n_items)}
    p = 1.0 / (np.arange(n_items - 4) + 3.0)
    p /= p.sum()

    def bag(lo, hi):
        b = rng.choice(n_items - 4, size=rng.randint(lo, hi), replace=False, p=p).tolist()
        return b + b[:1] if rng.rand() < 0.1 else b                      # (now and then an item twice)

    train = ref_ds.BagsWithVocab([bag(2, 9) for _ in range(n_train)], vocab, owners=["d%d" % i for i in range(n_train)])
    test = ref_ds.BagsWithVocab([bag(1, 7) for _ in range(n_test - 1)] + [[]], vocab, owners=["t%d" % i for i in range(n_test)])
    rec = ref_bl.MostPopular()
    rec.train(train)
    pred = rec.predict(test)
    Xtr, Xte = train.tocsr(), test.tocsr()
    assert isinstance(rec.most_popular, np.matrix) and pred.shape == (n_test, n_items)
    out = dict(n_items=np.asarray(n_items),
               train_indptr=Xtr.indptr.astype(np.int64), train_indices=Xtr.indices.astype(np.int32), train_data=np.asarray(Xtr.data),
               test_indptr=Xte.indptr.astype(np.int64), test_indices=Xte.indices.astype(np.int32), test_data=np.asarray(Xte.data),
               most_popular=np.asarray(rec.most_popular), pred=np.asarray(pred), pred_is_matrix=np.asarray(int(isinstance(pred, np.matrix))),
               model_str=np.asarray(str(rec)))
    path = os.path.join(OUT, "most_popular.npz")
    np.savez_compressed(path, **out)
    print("most_popular: train", Xtr.shape, Xtr.dtype, "counts", out["most_popular"].dtype, "max", int(out["most_popular"].max()),
          "pred", pred.shape, type(pred).__name__, "bytes", os.path.getsize(path))


def gen_challenge():
    """The three metrics of the RecSys-2018 challenge (eval/mpd/mpd_metrics.py:43-144, as eval/evaluate_dev.py uses them) and the
    reference's METRICS, per row, on fixed-seed rankings: 700 items, every row a permutation of them (the ranking, best first)
    and 1 to 200 targets, no row empty.  challenge_metrics.npz holds arrays only: the rankings, the targets as CSR, and per k of
    CHALLENGE_KS the per-row r_precision / ndcg / playlist_extender_clicks of the ranking cut at k, and per name of METRICS the
    per-row values of METRICS[name](y_true, y_pred, average=False) on scores that order the items as the ranking does."""
    import_reference()
    import aaerec.evaluation as ref_ev
    import aaerec.rank_metrics_with_std as ref_rm    # noqa: F401  (what ref_ev.METRICS computes with)
    import eval.mpd.mpd_metrics as ref_mpd
    rng = np.random.RandomState(2018)
    n_items, ks = 700, (1, 10, 64, 65, 500)
    lengths = [1, 2, 3, 63, 64, 65, 200, 1, 2, 5, 10, 11, 20, 21, 100, 199] + rng.randint(1, 201, size=24).tolist()
    n = len(lengths)
    perms = np.stack([rng.permutation(n_items) for _ in range(n)]).astype(np.int32)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    targets = []
    for r, m in enumerate(lengths):
        # the first rows keep their targets near the head of the ranking, so that small k see hits; the rest anywhere
        pool = perms[r][:max(m, 40)] if r % 3 == 0 else perms[r]
        targets.append(np.sort(rng.choice(pool, size=m, replace=False)))
    indices = np.concatenate(targets).astype(np.int32)
    out = dict(n_items=np.asarray(n_items), ks=np.asarray(ks, dtype=np.int64), rankings=perms, indptr=indptr, indices=indices)
    rprec, ndcg, clicks = (np.zeros((len(ks), n)) for _ in range(3))
    for i, k in enumerate(ks):
        for r in range(n):
            t, pred = targets[r].tolist(), perms[r].tolist()
            rprec[i, r] = ref_mpd.r_precision(t, pred, k)
            ndcg[i, r] = ref_mpd.ndcg(t, pred, k)
            clicks[i, r] = ref_mpd.playlist_extender_clicks(t, pred, k)
    out.update({"r-prec": rprec, "ndcg": ndcg, "clicks": clicks})
    y_true = np.zeros((n, n_items))
    y_pred = np.zeros((n, n_items))
    for r in range(n):
        y_true[r, targets[r]] = 1.0
        y_pred[r, perms[r]] = np.arange(n_items, 0, -1, dtype=np.float64)
    names = sorted(ref_ev.METRICS)
    out["metric_names"] = np.asarray(names)
    out["metric_values"] = np.stack([np.asarray(ref_ev.METRICS[name](y_true, y_pred, average=False), dtype=np.float64) for name in names])
    path = os.path.join(OUT, "challenge_metrics.npz")
    np.savez_compressed(path, **out)
    print("challenge_metrics:", n, "rows, lengths", min(lengths), "-", max(lengths), "names", names, "bytes", os.path.getsize(path))


IRGAN_CASES = {
    # name: (users, items, (fewest, most) items per user, batch_size, seed)
    "irgan_small": (7, 40, (1, 4), 4, 91),
    "irgan_dup": (5, 9, (3, 6), 16, 92),
}


def gen_irgan(only=None):
    """The reference's IRGAN (irgan/cf_gan.py) on two toy problems, on the CPU, in a temporary working directory (fit writes
    dis-train.txt where it stands).  np.random.choice is wrapped to record every result; generate_for_d is wrapped to record the
    lines it wrote; both nets' step() to record every loss; the states are snapshot at the first all_logits call behind a
    generate_for_d (the end of a D-epoch block) and at the first generate_for_d of the next epoch / the end of fit (the end of
    a G-epoch block).  n_epochs=2, d_epochs=6 (generate_for_d runs twice per epoch), g_epochs=2, lr=0.05, emb_dim=5 (the
    reference's all_rating hard-codes it).  irgan_*.npz hold arrays only.

    ONE INTERVENTION: fit reads its batches with linecache.getline, which never looks at the file again once it has cached it, so
    in a fresh process every D step of the reference trains on the FIRST dis-train.txt it wrote (and, in a process that has run
    another model, on that model's) while generate_for_d goes on drawing and writing new ones.  That depends on what the process
    did before, not on the model; the wrapper clears linecache behind every generate_for_d, so the recorded run trains on the
    lines it has just generated - what cf_gan.py's loop is written to do, and what aaerec/irgan.py does."""
    import linecache
    import tempfile
    import_reference()
    import irgan.cf_gan as ref_gan
    for name, (users, items, (lo, hi), batch_size, seed) in IRGAN_CASES.items():
        if only is not None and name != only:
            continue
        rng = np.random.RandomState(seed)
        X = {u: rng.choice(items, size=rng.randint(lo, hi + 1), replace=False).tolist() for u in range(users)}
        torch.manual_seed(seed)
        np.random.seed(seed)
        n_epochs, d_epochs, g_epochs, lr = 2, 6, 2, 0.05
        model = ref_gan.IRGAN(users, items, batch_size=batch_size, emb_dim=5, lr=lr, n_epochs=n_epochs, d_epochs=d_epochs,
                              g_epochs=g_epochs, verbose=False)
        G, D = model.generator, model.discriminator

        def state(out, prefix):
            for tag, net, params in (("g", G, G.g_params), ("d", D, D.d_param)):
                for key, p in zip(("user_emb", "item_emb", "item_bias"), params):
                    buf = net.optimizer.state[p].get("momentum_buffer") if p in net.optimizer.state else None
                    out["%s.%s.%s" % (prefix, tag, key)] = p.detach().numpy().copy()
                    out["%s.%s.m_%s" % (prefix, tag, key)] = np.zeros_like(p.detach().numpy()) if buf is None else buf.numpy().copy()

        out = {}
        state(out, "init")
        draws, line_sets, d_losses, g_losses, blocks = [], [], [], [], []
        pending = [False]          # a generate_for_d has run since the last G step
        calls = [0]
        per_epoch = (d_epochs + 4) // 5
        real_choice, real_gen, real_logits = np.random.choice, model.generate_for_d, G.all_logits
        real_dstep, real_gstep = D.step, G.step

        def rec_choice(*a, **k):
            r = real_choice(*a, **k)
            draws.append(np.asarray(r, dtype=np.int64).copy())
            return r

        def rec_gen(filename, condition_data=None):
            if calls[0] and calls[0] % per_epoch == 0:
                state(out, "block%d" % len(blocks)); blocks.append(1)       # (the G-epoch block of the epoch before)
            calls[0] += 1
            real_gen(filename, condition_data)
            linecache.clearcache()      # (see the docstring: fit then reads the file it has just written)
            with open(filename) as fh:
                line_sets.append(np.asarray([[int(v) for v in ln.split()] for ln in fh.read().split("\n")], dtype=np.int32))
            pending[0] = True

        def rec_logits(*a, **k):
            if pending[0]:
                pending[0] = False
                state(out, "block%d" % len(blocks)); blocks.append(0)       # (a D-epoch block)
            return real_logits(*a, **k)

        def rec_dstep(loss):
            d_losses.append(float(loss.item()))
            return real_dstep(loss)

        def rec_gstep(loss):
            g_losses.append(float(loss.item()))
            return real_gstep(loss)

        np.random.choice = rec_choice
        model.generate_for_d = rec_gen
        object.__setattr__(G, "all_logits", rec_logits)
        object.__setattr__(D, "step", rec_dstep)
        object.__setattr__(G, "step", rec_gstep)
        here = os.getcwd()
        try:
            with tempfile.TemporaryDirectory() as tmp:
                os.chdir(tmp)
                model.fit(X)
        finally:
            os.chdir(here)
            np.random.choice = real_choice
        state(out, "block%d" % len(blocks)); blocks.append(1)
        assert blocks == [0, 1] * n_epochs and len(line_sets) == per_epoch * n_epochs, (blocks, len(line_sets))
        rating = G.all_rating(list(range(users))).detach().numpy()
        pred = np.stack([model.simple_test_one_user((rating[u], u)) for u in range(users)])
        lens = [len(X[u]) for u in range(users)]
        out.update(cfg=np.asarray(json.dumps(dict(users=users, items=items, batch_size=batch_size, emb_dim=5, lr=lr, n_epochs=n_epochs,
                                                  d_epochs=d_epochs, g_epochs=g_epochs, momentum=0.9, n_blocks=len(blocks)))),
                   pos_indptr=np.concatenate(([0], np.cumsum(lens))).astype(np.int64),
                   pos_items=np.concatenate([X[u] for u in range(users)]).astype(np.int32),
                   draw_indptr=np.concatenate(([0], np.cumsum([d.size for d in draws]))).astype(np.int64),
                   draws=np.concatenate(draws).astype(np.int32),
                   line_indptr=np.concatenate(([0], np.cumsum([ls.shape[0] for ls in line_sets]))).astype(np.int64),
                   lines=np.concatenate(line_sets).astype(np.int32),
                   d_losses=np.asarray(d_losses), g_losses=np.asarray(g_losses), pred=pred)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name + ":", users, "users", items, "items", len(draws), "draws", len(d_losses), "D steps", len(g_losses), "G steps",
              "bytes", os.path.getsize(path))


ACT_NAMES = ["Softplus", "Hardtanh", "ReLU6", "CELU", "Softsign", "Hardsigmoid", "LogSigmoid", "Softshrink", "Hardshrink",
             "Identity", "GELU", "SiLU", "Mish", "Hardswish", "ELU", "LeakyReLU", "Sigmoid"]
# added after r6: seeds go on from ACT_NAMES', whose fixtures regenerate bit for bit.  PReLU's six weights (enc.act1 .. disc.act2)
# are in the recorded states like every parameter, their moments under the index config.param_order gives them
ACT_NAMES_MORE = ["Tanhshrink", "PReLU"]


# The conditions the bag kernels train (csrc/cond_bag.h): fixture -> the run_case / gen_vae condition kind.
BAG_CASES = {"step_cat_max": "cat_max", "step_cat_max_dense": "cat_max_dense", "step_bag_mean": "bag_mean",
             "step_bag_max": "bag_max", "step_vae_bag": "bag_sum"}
# Seeds screened on the CPU alone, as gen_vae's comment describes for the wide cases: Adam's first step moves an element whose
# gradient is near its eps by up to lr whatever the arithmetic, so a fixture holding one pins the reference's own rounding,
# not the model.  A seed is kept when the float32 oracle's replay (tests/test_cond_bag_cpu.py, which prints the figure) stays
# within a fifth of test_oracle_golden.py's 5e-6 on every parameter and on the condition table after every step: a near-eps
# element shows as a difference of 1e-6 and more there (the wide VAE cases above).  The first seeds tried, 71 .. 75, gave
# 1.2e-7, 1.2e-7, 6.0e-8, 8.1e-8 and 3.0e-8 - float32 rounding alone - and were kept.
# `bagcond:<name>:<seed>` tries another seed (into AAE_GOLDEN_OUT).
BAG_SEEDS = {"step_cat_max": 71, "step_cat_max_dense": 72, "step_bag_mean": 73, "step_bag_max": 74, "step_vae_bag": 75}


def run_bag_case(ref_aae, ref_cond, name, seed):
    kind = BAG_CASES[name]
    if name == "step_vae_bag":
        gen_vae(only=f"step_vae_bag:{seed}")
    else:
        run_case(ref_aae, ref_cond, name, seed=seed, cond=kind, steps=4, dropout=(0.2, 0.2) if kind == "cat_max" else (0.0, 0.0))


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_aae, ref_cond = import_reference()
    _selfcheck_recording_dropouts()
    which = set(sys.argv[1:])

    def want(n):
        return not which or n in which

    if want("steps"):
        run_case(ref_aae, ref_cond, "step_nodrop_gauss", seed=0)
        run_case(ref_aae, ref_cond, "step_masks", seed=1, dropout=(0.2, 0.2))
        run_case(ref_aae, ref_cond, "step_masks_uneven", seed=2, dropout=(0.1, 0.3), B=13)
        run_case(ref_aae, ref_cond, "step_cond_concat", seed=3, cond="concat30", dropout=(0.2, 0.2))
        run_case(ref_aae, ref_cond, "step_cond_categorical", seed=4, cond="categorical")
        run_case(ref_aae, ref_cond, "step_cond_concat_bias", seed=12, cond="concat30+bias")
        run_case(ref_aae, ref_cond, "step_selu", seed=5, activation="SELU", dropout=(0.2, 0.2))
        run_case(ref_aae, ref_cond, "step_categorical_prior", seed=6, prior="categorical")
        run_case(ref_aae, ref_cond, "step_bernoulli_prior", seed=7, prior="bernoulli")
        run_case(ref_aae, ref_cond, "step_prior_scale", seed=8, prior_scale=2.0)
        run_case(ref_aae, ref_cond, "step_sgd", seed=9, optimizer="sgd", gen_lr=0.05, reg_lr=0.02)
        run_case(ref_aae, ref_cond, "step_nonorm", seed=10, normalize_inputs=False)
        run_case(ref_aae, ref_cond, "step_ragged", seed=11, dropout=(0.2, 0.2),
                 batch_kw=dict(empty_row=5, max_len=12), last_B=5)
        run_case(ref_aae, ref_cond, "step_tanh", seed=13, activation="Tanh", dropout=(0.2, 0.2))
        run_case(ref_aae, ref_cond, "step_lrs", seed=14, gen_lr=0.01, reg_lr=0.0005, steps=5,
                 dropout=(0.2, 0.2))
        # one wider case so multi-tile kernel paths are pinned too
        run_case(ref_aae, ref_cond, "step_wide", seed=15, N=1100, h=72, c=24, B=40, steps=2,
                 dropout=(0.2, 0.2), batch_kw=dict(max_len=20), capture_acts=False, states='last')
    if want("acts"):
        # r6: one case per further activation class name the reference's getattr(nn, activation)() accepts (aae.py:110) and the
        # kernels cover; small states (last step only) - what differs from step_masks is the activation and its derivative
        for i, a in enumerate(ACT_NAMES):
            run_case(ref_aae, ref_cond, "step_act_" + a.lower(), seed=60 + i, activation=a, dropout=(0.2, 0.2),
                     capture_acts=False, states='last')
    if want("acts") or "acts_more" in which:      # (acts_more: only the classes added since)
        for i, a in enumerate(ACT_NAMES_MORE):
            run_case(ref_aae, ref_cond, "step_act_" + a.lower(), seed=60 + len(ACT_NAMES) + i, activation=a, dropout=(0.2, 0.2),
                     capture_acts=False, states='last')
        run_case(ref_aae, ref_cond, "step_act_prelu_sgd", seed=60 + len(ACT_NAMES) + len(ACT_NAMES_MORE), activation="PReLU",
                 optimizer="sgd", gen_lr=0.05, reg_lr=0.02, dropout=(0.2, 0.2), capture_acts=False, states='last')
        gen_vae(only="step_vae_prelu")
    if want("headline"):
        # the headline layer widths (h=200, c=50, batch 100: 13 column blocks in the layer chains and in the fused
        # decoder output layer, 7 row blocks) on a small vocabulary, straight from the reference
        run_case(ref_aae, ref_cond, "step_headline", seed=16, N=330, h=200, c=50, B=100, steps=2,
                 dropout=(0.2, 0.2), batch_kw=dict(max_len=24), capture_acts=False, states='last')
    if want("saturated"):
        gen_saturated(ref_aae, ref_cond)
    for w in which:             # saturated:<scale>[:<seed>] -> a scratch fixture (the search for the scale; not committed)
        if w.startswith("saturated:"):
            f = w.split(":")
            gen_saturated(ref_aae, ref_cond, scale=float(f[1]), seed=int(f[2]) if len(f) > 2 else 16, name="tmp_step_saturated")
    if want("c4"):
        # config C4's widths: a 300-d constant title block concatenated to the 50-d code (condition.py:345-369,
        # aae.py:688-690) -> dec.lin1 is [350 -> 200], beyond the layer-chain kernels; batch > 104 rows (the reference's
        # EconBiz driver uses 1000, eval/econis.py:45): the three-kernel output layer
        run_case(ref_aae, ref_cond, "step_c4", seed=17, N=460, h=200, c=50, B=128, steps=2, cond="concat300",
                 dropout=(0.2, 0.2), batch_kw=dict(max_len=24), capture_acts=False, states='last')
    if want("catcond"):
        # trainable CategoricalCondition variants: SparseAdam (the reference's default), mean / no reduction, and
        # behind a constant concatenated block
        run_case(ref_aae, ref_cond, "step_cat_sparse_sum", seed=41, cond="cat_sparse_sum", dropout=(0.2, 0.2), steps=4)
        run_case(ref_aae, ref_cond, "step_cat_sparse_mean", seed=42, cond="cat_sparse_mean", steps=4)
        run_case(ref_aae, ref_cond, "step_cat_single", seed=43, cond="cat_single", steps=4)
        run_case(ref_aae, ref_cond, "step_concat_cat", seed=44, cond="concat30+cat", dropout=(0.2, 0.2), steps=4)
    if want("bagcond"):
        # CategoricalCondition(reduce="max") under SparseAdam / Adam, and EmbeddingBagCondition in its three modes
        for name in BAG_CASES:
            run_bag_case(ref_aae, ref_cond, name, BAG_SEEDS[name])
    for w in which:             # bagcond:<name>:<seed> -> that case at another seed (the search for the seed: AAE_GOLDEN_OUT)
        if w.startswith("bagcond:"):
            f = w.split(":")
            run_bag_case(ref_aae, ref_cond, f[1], int(f[2]))
    if want("ae_only"):
        run_ae_only_case(ref_aae, "step_ae_only", seed=21)
    if want("decoding"):
        run_decoding_case(ref_aae, ref_cond, "step_decoding", seed=31)
        run_decoding_case(ref_aae, ref_cond, "step_decoding_trainable", seed=32, incs=(8, 10), trainable=True)
    if want("dae"):
        gen_dae()
    if want("vae"):
        gen_vae()
    if "dae_gauss" in which:    # (only the DenoisingAutoEncoder(corrupt='gauss') case)
        gen_dae_gauss()
    if "vae_cat" in which:      # (only the VAE + trainable CategoricalCondition case)
        gen_vae(only="step_vae_cat")
    if "vae_wide" in which:     # (only the two cases with a decoder input beyond one slot)
        gen_vae(only="step_vae_wide")
        gen_vae(only="step_vae_wide5")
    if "vae_hwide" in which:    # (only the two cases with a hidden layer / code beyond one slot)
        gen_vae(only="step_vae_hwide")
        gen_vae(only="step_vae_hwide_cond")
    for w in which:             # vae_wide:<name>:<seed> -> that case at another seed (the search for the seed: AAE_GOLDEN_OUT)
        if w.startswith("vae_wide:"):
            f = w.split(":")
            gen_vae(only=(f[1], int(f[2])))
    if want("vectorizer"):
        gen_embedded_vectorizer()
    if want("svd"):
        gen_svd()
    if want("mi"):
        gen_mi()
    if want("popular"):
        gen_popular()
    if want("irgan"):
        gen_irgan()
    if want("metrics"):
        gen_metric_known_answers()
    if want("challenge"):
        gen_challenge()
    if want("e2e"):
        gen_e2e_c1(ref_aae)
    if want("e2e_big"):
        gen_e2e_c1_big(ref_aae)
    if "e2e_c3" in which:       # (only on request: a minute or two of CPU at |items| = 100 000)
        gen_e2e_c3(ref_aae)
    for w in which:             # e2e_c3:<epochs> -> a scratch fixture at another horizon (debugging; not committed)
        if w.startswith("e2e_c3:"):
            f = w.split(":")
            gen_e2e_c3(ref_aae, n_epochs=int(f[1]), out_name="tmp_e2e_c3_{}.npz".format(f[1]), gen_lr=float(f[2]) if len(f) > 2 else 0.01)


if __name__ == "__main__":
    main()
