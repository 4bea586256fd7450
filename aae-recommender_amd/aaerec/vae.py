""" Variational autoencoder recommender (mirror of the reference's aaerec/vae.py:47-345 on the HIP kernels).

x -> L1 normalise -> fc1 -> act -> (fc21 = mu, fc22 = logvar) -> z = mu + eps * exp(logvar / 2) -> [conditions]
-> fc3 -> act -> fc4 -> sigmoid;  loss = nn.BCELoss() (mean) + KL sum (vae.py:132-145);  one optimiser.
The step is `aae_vae_step` of libaaerec_hip.so (cfg.reserved[2] = 3): the sparse first-layer gather/scatter with
lazy Adam, the fused vocabulary-wide output layer and the layer-chain kernel with two VAE ops (reparametrise and
its backward incl. the KL gradient).  Parameter names in the kernels' model: enc.lin1 = fc1, enc.lin3 =
[fc21; fc22], dec.lin1 = fc3, dec.lin3 = fc4.

Like the reference, predict() samples eps as well (vae.py:229-266 runs the same forward in eval mode).
Conditions: constant concatenated blocks (e.g. PretrainedWordEmbeddingCondition) and CategoricalConditions whose
table lives on this GPU ride in aae_vae_step (encoded and trained by aae_bag_encode / aae_bag_update around the step, as
in the AAE - condition.py:397-508); any other plugin runs with torch autograd between the code and the decoder: the step
is cut at the condition boundary (aae_vae_encode -> encode_impose -> aae_vae_decode_backward -> the plugins' backward and
step -> aae_vae_encoder_backward).
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _hip, ranking
from .aae import TORCH_OPTIMIZERS, AdversarialAutoEncoder, _take, _validate_targets, loss_targets, resident_condition_data
from .base import Recommender
from .condition import _check_conditions, device_native_conditions

STATUS_FORMAT = "[ R: {:.4f}]"
# widest decoder input [z | conditions | 1] of a VAE handle: fc3 in up to five k-parts of 208 columns (csrc/abi_model.h
# kVaeDecInMax, include/aaerec_hip.h) - the reference drivers' CONDITIONS need 383 and, eval/mpd/mpd.py, 983
DEC_IN_MAX = 1040
# widest hidden layer and code (csrc/abi_model.h kVaeWideHiddenMax / kVaeWideCodeMax, include/aaerec_hip.h): beyond a chain
# slot - n_hidden > 207 or 2 * n_code > 208, the reference's own grid point (300, 100) - the handle is asked for cfg.vae_wide
# and runs its hidden half one launch per layer
HIDDEN_MAX, CODE_MAX = _hip.VAE_WIDE_HIDDEN_MAX, _hip.VAE_WIDE_CODE_MAX
assert (HIDDEN_MAX, CODE_MAX) == (1024, 512)


def log_losses(loss):
    print('\r' + STATUS_FORMAT.format(loss), end='', flush=True)


class VAE:
    def __init__(self, inp, out, n_hidden=100, n_code=50, lr=0.001, batch_size=100, n_epochs=500, optimizer='adam',
                 normalize_inputs=True, activation='ReLU', final_activation='Sigmoid', conditions=None, verbose=True,
                 log_interval=1, device=None, rng_mode="device", seed=None):
        if inp != out:
            raise ValueError("the bag-of-items VAE reconstructs its input: inp must equal out")
        if final_activation != 'Sigmoid':
            raise NotImplementedError("final_activation='{}': the fused output layer is sigmoid + BCE".format(
                final_activation))
        if optimizer.lower() not in TORCH_OPTIMIZERS:
            raise KeyError(optimizer.lower())
        if rng_mode not in ("device", "reference"):
            raise ValueError("rng_mode must be 'device' or 'reference'")
        self.normalize_inputs = normalize_inputs
        self.inp, self.n_hidden, self.n_code = inp, n_hidden, n_code
        self.n_epochs, self.verbose, self.batch_size, self.lr = n_epochs, verbose, batch_size, lr
        self.activation, self.conditions, self.log_interval = activation, conditions, log_interval
        self.rng_mode = rng_mode
        self.training = True
        self.last_loss = None
        self.last_test_loss = None
        code_inc = int(conditions.size_increment()) if conditions else 0
        if n_code + code_inc + 1 > DEC_IN_MAX:
            raise ValueError("the VAE's decoder input [z | conditions | 1] is n_code + conditions.size_increment() + 1 = "
                             "{} + {} + 1 columns: the kernels take at most {} (five parts of 208)".format(
                                 n_code, code_inc, DEC_IN_MAX))
        if n_hidden > HIDDEN_MAX or n_code > CODE_MAX:
            raise ValueError("the VAE's kernels take n_hidden <= {} and n_code <= {}: got n_hidden = {}, n_code = {}".format(
                HIDDEN_MAX, CODE_MAX, n_hidden, n_code))
        # a model that fits a chain slot creates the handle it always did
        vae_wide = n_hidden > _hip.VAE_CHAIN_HIDDEN_MAX or 2 * n_code > _hip.VAE_CHAIN_CODE2_MAX
        dev_probe = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # conditions the kernels produce / train themselves ride in aae_vae_step; any other plugin gets the step cut at
        # the condition boundary and runs with torch autograd in between (aae_vae_encode / _decode_backward / ...)
        self._cond_native = not conditions or device_native_conditions(conditions, dev_probe)
        self._dp = None
        seed = seed if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) \
            if rng_mode == "device" else 0
        self.hip = _hip.HipAAE(inp, n_hidden, n_code, cond_inc=code_inc, max_batch=batch_size, max_nnz=batch_size * 4096,
                               activation=activation, optimizer=optimizer.lower(), normalize_inputs=normalize_inputs,
                               dropout=(0.0, 0.0), gen_lr=lr, reg_lr=lr,
                               rng_mode="device" if rng_mode == "device" else "inject", seed=seed, device=device,
                               vae=True, **({"vae_wide": True} if vae_wide else {}))
        self.device = self.hip.device
        # nn.Linear default initialisation in the reference's construction order: fc1, fc21, fc22, fc3, fc4
        fc1, fc21, fc22 = torch.nn.Linear(inp, n_hidden), torch.nn.Linear(n_hidden, n_code), torch.nn.Linear(n_hidden, n_code)
        fc3, fc4 = torch.nn.Linear(n_code + code_inc, n_hidden), torch.nn.Linear(n_hidden, out)
        n = lambda t: t.detach().numpy()                                              # noqa: E731
        self.hip.load_params({
            "enc.lin1.weight": n(fc1.weight), "enc.lin1.bias": n(fc1.bias),
            "enc.lin3.weight": np.vstack([n(fc21.weight), n(fc22.weight)]),
            "enc.lin3.bias": np.concatenate([n(fc21.bias), n(fc22.bias)]),
            "dec.lin1.weight": n(fc3.weight), "dec.lin1.bias": n(fc3.bias),
            "dec.lin3.weight": n(fc4.weight), "dec.lin3.bias": n(fc4.bias)})

    def __str__(self):
        return "VAE ({} -> {} -> 2x{} -> {} -> {}), lr {}".format(self.inp, self.n_hidden, self.n_code, self.n_hidden,
                                                                 self.inp, self.lr)

    # ---- nn.Module-like surface the drivers touch ----------------------------------------------------
    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def cuda(self):
        return self

    def state_dict(self):
        """The reference's parameter names (fc1, fc21, fc22, fc3, fc4)."""
        sd, c = self.hip.state_dict(), self.n_code
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                      # noqa: E731
        return {"fc1.weight": t(sd["enc.lin1.weight"]), "fc1.bias": t(sd["enc.lin1.bias"]),
                "fc21.weight": t(sd["enc.lin3.weight"][:c]), "fc21.bias": t(sd["enc.lin3.bias"][:c]),
                "fc22.weight": t(sd["enc.lin3.weight"][c:]), "fc22.bias": t(sd["enc.lin3.bias"][c:]),
                "fc3.weight": t(sd["dec.lin1.weight"]), "fc3.bias": t(sd["dec.lin1.bias"]),
                "fc4.weight": t(sd["dec.lin3.weight"]), "fc4.bias": t(sd["dec.lin3.bias"])}

    # ---- internals ------------------------------------------------------------------------------------
    def _eps(self, B):
        """reparametrize()'s torch.randn_like(std) (vae.py:117) off the global CPU generator in 'reference' mode."""
        return torch.randn(B, self.n_code) if self.rng_mode == "reference" else None

    # the condition block of a batch / the update of trainable tables from its gradient: the AAE's helpers
    _is_constant_concat = AdversarialAutoEncoder._is_constant_concat
    _native_cond_block = AdversarialAutoEncoder._native_cond_block
    _native_cond_update = AdversarialAutoEncoder._native_cond_update

    def _cond(self, c_batch):
        return self._native_cond_block(c_batch, len(c_batch[0]) if not hasattr(c_batch[0], "shape") else c_batch[0].shape[0])

    _cond_fn = AdversarialAutoEncoder._cond_fn

    # True: device-native trainable conditions read their data from HBM, uploaded once per fit / ranking call (aae.py:
    # resident_condition_data); False (the default): the padded per-step route
    resident_conditions = False

    def _is_device_native(self):
        return self._cond_native

    def _step(self, csr, n_rows, rows, c_batch):
        if c_batch is not None and not self._cond_native:
            # the step cut at the condition boundary (vae.py:120-130, 175-181)
            z = self.hip.vae_encode(csr, 0, n_rows, rows=rows, eps=self._eps(n_rows), train=True)
            zc, back = self._cond_fn(c_batch)(z)
            self.hip.vae_encoder_backward(back(self.hip.vae_decode_backward(zc)))
            self._last_rows = n_rows
            if self.verbose:
                log_losses(self.loss())
            return
        self.hip.vae_step(csr, 0, n_rows, rows=rows, cond=self._cond(c_batch) if c_batch is not None else None,
                          eps=self._eps(n_rows))
        if c_batch is not None and not self._is_constant_concat():
            self._native_cond_update(n_rows)           # conditions.zero_grad / backward / step, vae.py:175-181
        self._last_rows = n_rows
        if self.verbose:
            log_losses(self.loss())

    def loss(self):
        """(mean BCE + KL sum) / rows of the last step: loss.item() / len(X) as the reference logs it (vae.py:185)."""
        l = self.hip.losses()
        self.last_loss = (l[0] + l[1]) / self._last_rows
        return self.last_loss

    # ---- public API (vae.py:147-266) --------------------------------------------------------------------
    def partial_fit(self, X, y=None, condition_data=None):
        use_condition = _check_conditions(self.conditions, condition_data)
        if y is not None:
            raise ValueError("(Semi-)supervised usage not supported")
        Xs = sp.csr_matrix(X) if not sp.issparse(X) else X.tocsr()
        _validate_targets(Xs)
        if Xs.shape[0] > self.hip.max_batch:
            raise ValueError("batch of {} rows exceeds batch_size={}".format(Xs.shape[0], self.hip.max_batch))
        self.train()
        if self.conditions:
            self.conditions.train()
        self._step(_hip.DeviceCSR(Xs, self.device), Xs.shape[0], None, condition_data if use_condition else None)
        return self

    def fit(self, X, y=None, condition_data=None):
        if y is not None:
            raise NotImplementedError("(Semi-)supervised usage not supported")
        use_condition = _check_conditions(self.conditions, condition_data)
        X = X.tocsr()
        _validate_targets(X)
        csr = _hip.DeviceCSR(X, self.device)             # the corpus stays resident in HBM
        if use_condition:
            condition_data = resident_condition_data(self, condition_data)
        n_docs = X.shape[0]
        self.train()
        if self.conditions:
            self.conditions.train()
        for epoch in range(self.n_epochs):
            if self.verbose:
                print("Epoch", epoch + 1)
            perm = np.arange(n_docs)                     # sklearn.utils.shuffle(X, *condition_data), vae.py:207-211
            np.random.shuffle(perm)
            perm_dev = torch.as_tensor(perm.astype(np.int32), device=self.device)
            for start in range(0, n_docs, self.batch_size):
                idx = perm[start:start + self.batch_size]
                rows = perm_dev[start:start + len(idx)]
                c_batch = [_take(c, idx, rows) for c in condition_data] if use_condition else None
                self._step(csr, len(idx), rows, c_batch)
            if self.verbose:
                print()
        self.loss()
        return self

    def predict(self, X, condition_data=None, test_loss=False):
        """test_loss: also evaluate the reference's loss_function on every batch (vae.py:243-264) - on the device, with the
        eps rows the batch's scores were made from -, print its `====> Test set loss:` line and keep the value in
        last_test_loss."""
        use_condition = _check_conditions(self.conditions, condition_data)
        self.eval()
        if self.conditions:
            self.conditions.eval()
        Xs = sp.csr_matrix(X) if not sp.issparse(X) else X.tocsr()
        if test_loss:
            _validate_targets(Xs)
        csr = _hip.DeviceCSR(Xs, self.device)
        if use_condition:
            condition_data = resident_condition_data(self, condition_data)
        pred = _hip.HostRows(Xs.shape[0], Xs.shape[1], self.device)
        bce, kl = [], []
        with torch.no_grad():
            for start in range(0, Xs.shape[0], self.batch_size):
                n = min(self.batch_size, Xs.shape[0] - start)
                cond = None
                c_batch = [_take(c, slice(start, start + n)) for c in condition_data] if use_condition else None
                eps = self._eps(n)
                if use_condition and not self._cond_native:
                    z = self.hip.vae_encode(csr, start, n, eps=eps, train=False)
                    zc = self.conditions.encode_impose(z, c_batch)
                    pred.put(start, self.hip.decode(zc))
                    if test_loss:
                        bce.append(self.hip.vae_decode_loss(zc, csr, start))
                        kl.append(self._kl_rows(csr, start, n))
                    continue
                if use_condition:
                    cond = self._cond(c_batch)
                pred.put(start, self.hip.vae_predict(csr, start, n, cond=cond, eps=eps))
                if test_loss:       # (the device generator counts a batch's rows from 0 in vae_predict: row0 = 0 repeats its draws)
                    b, k = self.hip.vae_predict_loss(csr, start, n, cond=cond, eps=eps, row0=0)
                    bce.append(b)
                    kl.append(k)
        if test_loss:
            self.last_test_loss = self._test_loss(torch.cat(bce).cpu().numpy(), torch.cat(kl).cpu().numpy(), Xs.shape[1])
            print('====> Test set loss: {:.4f}'.format(self.last_test_loss))
        return pred.numpy()

    # ---- the loss on held-out rows (aae_vae_predict_loss / aae_vae_decode_loss) --------------------------------
    def _kl_rows(self, csr, start, n):
        """The rows' KL terms where the decoder input is a plugin's: they depend on the encoder alone, so the predict form
        with a zero condition block and zero draws answers them (its BCE sums are dropped)."""
        ci = self.hip.cfg.cond_inc
        cond = torch.zeros(n, ci, device=self.device) if ci else None
        return self.hip.vae_predict_loss(csr, start, n, cond=cond, eps=torch.zeros(n, self.n_code, device=self.device))[1]

    def _test_loss(self, row_bce, row_kl, n_items):
        """The reference's test loss from the per-row sums: sum over the batches of batch_size rows of (mean BCE of the
        batch + its KL sum), over the number of rows (vae.py:243-263)."""
        total, n_rows, bs = 0.0, len(row_bce), self.batch_size
        for s0 in range(0, n_rows, bs):
            b = row_bce[s0:s0 + bs]
            total += b.sum() / (len(b) * n_items) + row_kl[s0:s0 + bs].sum()
        return float(total / n_rows) if n_rows else 0.0

    def eval_loss(self, X, condition_data=None, targets=None, per_row=False):
        """The reference's test loss of the model on rows it was not trained on (vae.py:243-264: per batch of batch_size rows
        mean BCE + KL sum, summed, over the rows), without the [n, N] score matrix.  targets: None = X, or any matrix of X's
        shape with values in [0, 1].  per_row: (row_bce, row_kl) instead, the float64 sums over the items / the code of every
        row.  eps as predict_topk() draws it; on the device generator every row of the call has its own draw (row0)."""
        Xs = sp.csr_matrix(X) if not sp.issparse(X) else X.tocsr()
        tdev = loss_targets(targets, Xs.shape, self.device)
        if tdev is None:
            _validate_targets(Xs)
        parts = self._rank_chunks(
            Xs, condition_data, ranking.chunk_rows(self.batch_size, self.hip.loss_max_rows()),
            lambda csr, start, n, cond, eps: self.hip.vae_predict_loss(csr, start, n, cond=cond, eps=eps, row0=start, targets=tdev),
            lambda csr, start, zc: (self.hip.vae_decode_loss(zc, csr, start, targets=tdev), self._kl_rows(csr, start, zc.shape[0])))
        cat = lambda i: (torch.cat([p[i] for p in parts]) if parts else torch.zeros(0, dtype=torch.float64)).cpu().numpy()  # noqa: E731
        row_bce, row_kl = cat(0), cat(1)
        return (row_bce, row_kl) if per_row else self._test_loss(row_bce, row_kl, Xs.shape[1])

    # ---- ranking on the device (aae_vae_predict_topk / aae_vae_predict_ranks) ----------------------------------
    def _rank_chunks(self, Xs, condition_data, chunk, fused, decode):
        """The rows of Xs, `chunk` at a time, through fused(start, n, cond, eps) - conditions the kernels take ride in the
        call - or, behind any other plugin, decode(start, zc): aae_vae_encode -> encode_impose as predict() cuts it.  In
        rng_mode='reference' eps is drawn as predict() draws it - torch.randn per batch_size rows, in row order - so the
        same torch seed gives the scores of predict()."""
        use_condition = _check_conditions(self.conditions, condition_data)
        self.eval()
        if self.conditions:
            self.conditions.eval()
        csr = _hip.DeviceCSR(Xs, self.device)
        if use_condition:
            condition_data = resident_condition_data(self, condition_data)
        n_rows, bs = Xs.shape[0], self.batch_size
        eps_all = None
        if self.rng_mode == "reference":
            draws = [self._eps(min(bs, n_rows - s)) for s in range(0, n_rows, bs)]
            eps_all = torch.cat(draws).to(self.device) if draws else None
        out = []
        with torch.no_grad():
            for start, n in ranking.row_chunks(n_rows, chunk):
                eps = None if eps_all is None else eps_all[start:start + n]
                c_batch = [_take(c, slice(start, start + n)) for c in condition_data] if use_condition else None
                if use_condition and not self._cond_native:
                    z = torch.cat([self.hip.vae_encode(csr, s0, min(bs, start + n - s0), train=False,
                                                       eps=None if eps is None else eps[s0 - start:s0 - start + bs])
                                   for s0 in range(start, start + n, bs)])
                    out.append(decode(csr, start, self.conditions.encode_impose(z, c_batch)))
                else:
                    out.append(fused(csr, start, n, self._cond(c_batch) if use_condition else None, eps))
        return out

    def predict_topk(self, X, k=10, condition_data=None, exclude_known=True, y_true=None, metrics=None):
        """(item ids [n, k], scaled scores [n, k]) of predict -> remove_non_missing -> argtopk (vae.py:229-266,
        evaluation.py:183-199, 20-58) without the [n, N] score matrix: see AdversarialAutoEncoder.predict_topk.
        metrics: [(mean, std)] per bounded metric name against y_true instead (ranking.rank_metrics)."""
        Xs = sp.csr_matrix(X) if not sp.issparse(X) else X.tocsr()
        return ranking.finish_lists(self._rank_chunks(
            Xs, condition_data, ranking.chunk_rows(self.batch_size, self.hip.vae_rank_max_rows(k)),
            lambda csr, start, n, cond, eps: self.hip.vae_predict_topk(csr, start, n, k, cond=cond, eps=eps,
                                                                       exclude_known=exclude_known),
            lambda csr, start, zc: self.hip.vae_decode_topk(zc, csr, start, k, exclude_known=exclude_known)), k, metrics, y_true,
            Xs.shape)

    def predict_ranks(self, X, Y, condition_data=None, exclude_known=True, metrics=None):
        """A scipy CSR with Y's (canonical) pattern whose data are the int32 1-based ranks of the held-out items in the full
        ranking of their rows: see AdversarialAutoEncoder.predict_ranks.  metrics: [(mean, std)] per metric name instead."""
        Xs = sp.csr_matrix(X) if not sp.issparse(X) else X.tocsr()
        Ys = ranking.canonical_truth(Y, Xs.shape)
        truth = _hip.DeviceCSR(Ys, self.device)
        return ranking.finish_ranks(self._rank_chunks(
            Xs, condition_data, ranking.chunk_rows(self.batch_size, self.hip.vae_rank_full_max_rows()),
            lambda csr, start, n, cond, eps: self.hip.vae_predict_ranks(csr, start, n, truth, cond=cond, eps=eps,
                                                                        exclude_known=exclude_known),
            lambda csr, start, zc: self.hip.vae_decode_ranks(zc, csr, start, truth, exclude_known=exclude_known)), Ys, metrics)


class VAERecommender(Recommender):
    """
    Varietional Autoencoder Recommender
    =====================================
    Keyword arguments are forwarded to VAE (n_hidden, n_code, n_epochs, batch_size, lr, normalize_inputs, verbose, ...).
    """

    def __init__(self, conditions=None, **kwargs):
        super().__init__()
        self.verbose = kwargs.get('verbose', True)
        self.conditions = conditions
        self.model_params = kwargs
        self.model = None

    def __str__(self):
        desc = "Variational Autoencoder"
        if self.conditions:
            desc += " conditioned on: " + ', '.join(self.conditions.keys())
        desc += '\nModel Params: ' + str(self.model_params)
        return desc

    def train(self, training_set):
        X = training_set.tocsr()
        if self.conditions:
            condition_data = self.conditions.fit_transform(training_set.get_attributes(self.conditions.keys()))
        else:
            condition_data = None
        self.model = VAE(X.shape[1], X.shape[1], conditions=self.conditions, **self.model_params)
        print(self)
        print(self.model)
        print(self.conditions)
        self.model.fit(X, condition_data=condition_data)

    def predict(self, test_set):
        X = test_set.tocsr()
        if self.conditions:
            # Important to not call fit here, but just transform
            condition_data = self.conditions.transform(test_set.get_attributes(self.conditions.keys()))
        else:
            condition_data = None
        return self.model.predict(X, condition_data=condition_data)

    def _conditions_of(self, test_set):
        if not self.conditions:
            return None
        return self.conditions.transform(test_set.get_attributes(self.conditions.keys()))

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None):
        """(item ids [n, k], scaled scores [n, k]) of the k best new items per test bag; with metrics, [(mean, std)] per name
        against y_true."""
        return self.model.predict_topk(test_set.tocsr(), k=k, condition_data=self._conditions_of(test_set), y_true=y_true,
                                       metrics=metrics)

    def predict_ranks(self, test_set, y_true, metrics=None):
        """CSR with y_true's pattern: the rank of every held-out item in the full ranking of its test bag; with metrics,
        [(mean, std)] per name."""
        return self.model.predict_ranks(test_set.tocsr(), y_true, condition_data=self._conditions_of(test_set), metrics=metrics)

    def eval_loss(self, test_set, targets=None):
        """The reference's test loss of the model on the test bags (VAE.eval_loss), computed on the device."""
        return self.model.eval_loss(test_set.tocsr(), condition_data=self._conditions_of(test_set), targets=targets)
