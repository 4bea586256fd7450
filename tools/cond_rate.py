#!/usr/bin/env python3
"""Host-level throughput of the conditioned model variants at the headline widths.

    python tools/cond_rate.py        fit() in docs/s: no condition, a constant concatenated block (pretrained-embedding style), a
                                     trainable categorical condition (embedding on CPU = the reference's default, and on the GPU)
    python tools/cond_rate.py bag    partial_fit() in ms/step at batch 100 behind the conditions the bag kernels train
                                     (csrc/cond_bag.h): CategoricalCondition(reduce="max") under SparseAdam and Adam,
                                     EmbeddingBagCondition in its default mode and in mode="max" - on the native route and,
                                     forced by a subclass whose device_native returns False, on the bridged one
    python tools/cond_rate.py ragged a|b resident|padded [steps a pass]
                                     fit() in ms/step behind a trainable condition whose value lists are resident bags
                                     (csrc/cond_csr.h) or padded on the host every step: see ragged_rates
    python tools/cond_rate.py opts [fit [reversed]]
                                     max_norm and scale_grad_by_freq behind a CategoricalCondition(reduce="sum", sparse=False)
                                     with either option: partial_fit(), and fit() with the value lists as resident bags - native
                                     against the bridged route
    python tools/cond_rate.py const  fit() in ms/step behind constant 300-column blocks with resident_conditions False against True
                                     (DESIGN 4.1h): AdversarialAutoEncoder and DecodingRecommender, see const_rates
    python tools/cond_rate.py const split
                                     the AAE's MPD cell of that table taken apart (blocks, table, a synchronize per step)
Everything but `ragged b` (the VAE) and `const`'s DecodingRecommender rows runs through AdversarialAutoEncoder."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aae-recommender_amd"))
import numpy as np
import torch
from aaerec.aae import AdversarialAutoEncoder
from aaerec import condition as C
from tools.synth import throughput_corpus

N, h, c, B = 100000, 200, 50, 100
DOCS = 6400
X = throughput_corpus(DOCS, N, seed=1234)
rng = np.random.default_rng(0)


class ConstConcat(C.ConcatenationBasedConditioning):
    constant_concat = True

    def __init__(self, width):
        self.width = width

    def fit(self, raw):
        return self

    def transform(self, raw):
        return raw

    def encode(self, inputs):
        return torch.as_tensor(np.asarray(inputs), dtype=torch.float32)

    def size_increment(self):
        return self.width


def rate(tag, conditions, data, epochs=25):
    m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=B, n_epochs=1, conditions=conditions, verbose=False, seed=1)
    m.fit(X, condition_data=data)          # builds + warms
    torch.cuda.synchronize()
    m2 = m
    t0 = time.perf_counter()
    # fit() rebuilds the model; time whole calls (what a user sees), then subtract the build measured separately
    m2.n_epochs = epochs
    m2.fit(X, condition_data=data)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m2.n_epochs = 0
    m2.fit(X, condition_data=data)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    dt = (t1 - t0) - (t2 - t1)
    print(f"{tag:34s} {epochs * DOCS / dt:10.0f} docs/s   ({1e3 * dt / (epochs * DOCS / B):.3f} ms/step, build {t2 - t1:.2f} s)", flush=True)


def partial_fit_rates(rounds=9, warm=2, opts=False):
    """Median over `rounds` passes of 64 partial_fit calls (after `warm` passes), every pass closed by a synchronize.
    opts: the rows of DESIGN 4.1f (a max_norm table, a frequency-scaled one) instead of 4.1c's."""
    batches = [X[i:i + B] for i in range(0, DOCS, B)]
    authors = [[int(a) for a in rng.integers(0, 5000, rng.integers(1, 5))] for _ in range(DOCS)]
    # (a LongTensor on the GPU: the form nn.EmbeddingBag itself takes, so the bridged route needs no conversion)
    bags = torch.from_numpy(rng.integers(0, 5000, size=(DOCS, 4)).astype(np.int64)).cuda()

    def cat(sparse, reduce="max", **kw):
        def make(bridged):
            cls = C.CategoricalCondition
            if bridged:
                cls = type("Bridged", (cls,), {"device_native": lambda self, device: False})
            cond = cls(32, use_cuda=True, reduce=reduce, sparse=sparse, **kw)
            return cond, cond.fit_transform(authors)
        return make

    def bag(**kw):
        def make(bridged):
            cls = C.EmbeddingBagCondition
            if bridged:
                cls = type("Bridged", (cls,), {"device_native": lambda self, device: False})
            cond = cls(5001, 32, **kw)
            cond.embedding_bag.cuda()
            return cond, bags
        return make

    def ms_per_step(make, bridged):
        cond, data = make(bridged)
        m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=B, n_epochs=1, conditions=C.ConditionList([("authors", cond)]),
                                   verbose=False, seed=1)
        times = []
        for r in range(warm + rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, b in enumerate(batches):
                m.partial_fit(b, condition_data=[data[i * B:(i + 1) * B]])
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0) / len(batches))
        native = m._is_device_native()
        assert not (bridged and native)
        return float(np.median(times[warm:])), native
    print(f"partial_fit, N={N} h={h} c={c} batch {B}: median ms/step of {rounds} passes of {DOCS // B} steps")
    print(f"{'condition':44s} {'native':>10s} {'bridged':>10s}")
    rows = (("CategoricalCondition(32, max, SparseAdam)", cat(True)), ("CategoricalCondition(32, max, Adam)", cat(False)),
            ("EmbeddingBagCondition(5001, 32)  [mean]", bag()), ("EmbeddingBagCondition(5001, 32, mode=max)", bag(mode="max")))
    if opts:
        rows = (("CategoricalCondition(32, sum, Adam, max_norm=1)", cat(False, "sum", max_norm=1.0)),
                ("Categorical(32, sum, Adam, scale_grad_by_freq)", cat(False, "sum", scale_grad_by_freq=True)))
    for tag, make in rows:
        t_nat, native = ms_per_step(make, False)
        t_br, _ = ms_per_step(make, True)
        note = "" if native else "   (no native route in this build: both columns are the bridged route)"
        print(f"{tag:44s} {t_nat:10.3f} {t_br:10.3f}{note}", flush=True)


def fit_rates():
    rate("no condition", None, None)
    vec = rng.standard_normal((DOCS, 50)).astype(np.float32)
    rate("constant concat (50)", C.ConditionList([("title", ConstConcat(50))]), [vec])
    authors = [[int(a) for a in rng.integers(0, 5000, rng.integers(1, 5))] for _ in range(DOCS)]
    for on_gpu in (False, True):
        cat = C.CategoricalCondition(32, use_cuda=True, embedding_on_gpu=on_gpu, reduce="sum")
        cl = C.ConditionList([("authors", cat)])
        data = cl.fit_transform([authors])
        rate(f"categorical (32, emb on {'gpu' if on_gpu else 'cpu'})", cl, data, epochs=25 if on_gpu else 2)
        both = C.ConditionList([("title", ConstConcat(50)), ("authors", C.CategoricalCondition(
            32, use_cuda=True, embedding_on_gpu=on_gpu, reduce="sum"))])
        d2 = both.fit_transform([vec, authors])
        rate(f"concat + categorical (emb on {'gpu' if on_gpu else 'cpu'})", both, d2, epochs=25 if on_gpu else 2)

    # the same condition forced through the torch-autograd bridge (the step cut at the condition boundary)
    cat = C.CategoricalCondition(32, use_cuda=True, reduce="sum")
    cat.device_native = lambda device: False
    cl = C.ConditionList([("authors", cat)])
    rate("categorical (emb on gpu, autograd bridge)", cl, cl.fit_transform([authors]))


def opts_fit_rates(pass_steps=64, rounds=9, warm=2, order=(0, 1)):
    """ms/step of fit() behind CategoricalCondition(32, reduce="sum", sparse=False) with max_norm or
    scale_grad_by_freq, 4.1d's cell a (batch 100, table 5001 x 32, lists of 1-4 values): native with resident bags against the
    bridged route (the parent's behaviour: torch autograd at the condition boundary, lists padded on the host every step).
    The median [fastest, slowest] of `rounds` passes of `pass_steps` steps after `warm` passes, every pass closed by a
    synchronize; the two routes take turns twice (round 1 | round 2), one model each."""
    lists = [[int(a) for a in rng.integers(0, 5000, rng.integers(1, 5))] for _ in range(DOCS)]
    passes = warm + rounds
    print(f"fit(), batch {B}, table 5001 x 32, resident bags: median ms/step of {rounds} passes of {pass_steps} steps")
    print(f"{'condition':56s} {'native':>44s} {'bridged':>44s}")
    cases = (("CategoricalCondition(32, sum, Adam, max_norm=1)", dict(max_norm=1.0)),
             ("CategoricalCondition(32, sum, Adam, scale_grad_by_freq)", dict(scale_grad_by_freq=True)))
    for tag, kw in (cases[i] for i in order):
        med = {False: [], True: []}
        for bridged in (False, True, False, True):
            cls = C.CategoricalCondition
            if bridged:
                cls = type("Bridged", (cls,), {"device_native": lambda self, device: False})
            cond = cls(32, use_cuda=True, reduce="sum", sparse=False, vocab_size=5000, **kw)
            data = cond.fit_transform(lists)
            m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=B, n_epochs=passes + 1,
                                       conditions=C.ConditionList([("authors", cond)]), verbose=False, seed=1)
            m.resident_conditions = True
            times, mark, steps = [], None, 0
            for _ in m.fit_steps(X, condition_data=[data]):
                steps += 1
                if steps % pass_steps == 0:
                    torch.cuda.synchronize()
                    now = time.perf_counter()
                    if mark is not None:
                        times.append(1e3 * (now - mark) / pass_steps)
                    mark = now
                    if len(times) == passes:
                        break
            assert m._is_device_native() == (not bridged) and len(times) == passes
            med[bridged].append(f"{np.median(times[warm:]):.3f} [{min(times[warm:]):.3f}, {max(times[warm:]):.3f}]")
        print(f"{tag:56s} {' | '.join(med[False]):>44s} {' | '.join(med[True]):>44s}", flush=True)


def ragged_rates(cell, route, pass_steps=64, rounds=9, warm=2):
    """ms/step of fit() behind a trainable CategoricalCondition(32, reduce="sum") whose value lists are resident
    bags (route 'resident') or padded on the host every step (route 'padded': resident_conditions = False, and what a tree
    without the attribute does anyway).  One model per call; the median of `rounds` passes of `pass_steps` steps after `warm`
    passes, every pass closed by a synchronize.
      cell a   4.1c's configuration: AdversarialAutoEncoder, batch 100, table 5001 x 32, lists of 1-4 values
      cell b   a long tail behind the VAE step: batch 1000, table 50001 x 32, list lengths geometric with mean 20 capped at
               250, a list of 250 in every batch (the epoch's shuffle is switched off so that the layout holds)"""
    from aaerec.vae import VAE
    passes = warm + rounds
    if cell == "a":
        batch, vocab, docs = B, 5000, DOCS
        assert docs // batch == 64
        lists = [[int(a) for a in rng.integers(0, vocab, rng.integers(1, 5))] for _ in range(docs)]
        Xc = X
    else:
        batch, vocab, docs = 1000, 50000, 64000
        lens = np.minimum(rng.geometric(1 / 20.0, size=docs), 250)
        lens[::batch] = 250
        lists = [[int(a) for a in rng.integers(0, vocab, n)] for n in lens]
        Xc = throughput_corpus(docs, N, seed=4321)
        np.random.shuffle = lambda a: None
    cond = C.CategoricalCondition(32, use_cuda=True, reduce="sum", vocab_size=vocab)
    data = cond.fit_transform(lists)
    conds = C.ConditionList([("authors", cond)])
    has = hasattr(AdversarialAutoEncoder, "resident_conditions")
    times, mark = [], [None, 0]

    def tick():
        mark[1] += 1
        if mark[1] % pass_steps == 0:
            torch.cuda.synchronize()
            now = time.perf_counter()
            if mark[0] is not None:
                times.append(1e3 * (now - mark[0]) / pass_steps)
            mark[0] = now
    if cell == "a":
        m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=batch, n_epochs=passes + 1, conditions=conds, verbose=False, seed=1)
        m.resident_conditions = route == "resident"
        for _ in m.fit_steps(Xc, condition_data=[data]):
            tick()
            if len(times) == passes:
                break
    else:
        m = VAE(N, N, n_hidden=h, n_code=c, batch_size=batch, n_epochs=1, conditions=conds, verbose=False, seed=1)
        m.resident_conditions = route == "resident"
        step = m._step

        class Done(Exception):
            pass

        def timed(*a, **k):
            step(*a, **k)
            tick()
            if len(times) == passes:
                raise Done
        m._step = timed
        m.n_epochs = 1 + (passes + 1) * pass_steps // (docs // batch)
        try:
            m.fit(Xc, condition_data=[data])
        except Done:
            pass
    assert len(times) == passes, len(times)
    med, lo, hi = float(np.median(times[warm:])), min(times[warm:]), max(times[warm:])
    print(f"ragged cell {cell} route {route:8s} (tree has resident_conditions: {has}): median {med:.3f} ms/step "
          f"[{lo:.3f}, {hi:.3f}] over {rounds} passes of {pass_steps} steps, batch {batch}, table {vocab + 1} x 32, "
          f"{sum(len(r) for r in lists) / docs:.1f} values a list", flush=True)


class _Vect:
    """A vectoriser whose documents already are their vectors (what EmbeddedVectorizer.transform hands a condition)."""

    def __init__(self, width):
        self.embedding = np.zeros((1, width), dtype=np.float32)

    def fit(self, raw):
        return self

    def transform(self, raw):
        return raw


def const_rates(pass_steps=32, rounds=7, warm=2, split=False):
    """ms/step of fit() behind constant condition blocks (PretrainedWordEmbeddingCondition, 300 columns each) with
    resident_conditions False - the per-step route: rows picked on the host and uploaded, or index_select on a CUDA tensor -
    against True - one upload per fit(), one gather launch per step -, same process, same data, one model per run, the two
    routes taking turns twice (round 1 | round 2).  Models: AdversarialAutoEncoder and DecodingRecommender.  Cells: one block at
    batch 100, one block at batch 1000, MPD's list (3 blocks + CategoricalCondition(32, sum)) at batch 1000.  Feeds: the host
    numpy array train() produces, and the CUDA tensor keep_on_device=True keeps.  The median [fastest, slowest] of `rounds`
    passes of `pass_steps` steps after `warm` passes, every pass closed by a synchronize.
    split: instead, the AAE's MPD cell (host feed) taken apart - the three blocks without the table, the table alone, the list
    with the table kept on the per-step padded route under the flag, the whole list, and the whole list with a synchronize
    after every step (the host cannot enqueue ahead: what a step's host round trip costs when nothing hides it)."""
    from aaerec.aae import DecodingRecommender
    passes = warm + rounds
    big = 1000 * 64
    Xb = throughput_corpus(big, N, seed=4321)
    vecs = [rng.standard_normal((big, 300)).astype(np.float32) for _ in range(3)]
    lists = [[int(a) for a in rng.integers(0, 5000, rng.integers(1, 5))] for _ in range(big)]

    class Done(Exception):
        pass

    def run(model, batch, n_blocks, with_cat, on_device, flag, cat_resident=True, sync=False):
        docs = batch * 64
        items, data = [], []
        for j in range(n_blocks):
            items.append((f"title{j}", C.PretrainedWordEmbeddingCondition(_Vect(300), use_cuda=True)))
            data.append(torch.from_numpy(vecs[j][:docs]).cuda() if on_device else vecs[j][:docs])
        if with_cat:
            cat = C.CategoricalCondition(32, use_cuda=True, reduce="sum", vocab_size=5000)
            data.append(cat.fit_transform(lists[:docs]))
            if not cat_resident:
                cat.resident = lambda inputs, device: None        # (the value lists padded on the host every step)
            items.append(("playlist", cat))
        conds = C.ConditionList(items)
        Xc = X if batch == B else Xb
        times, mark = [], [None, 0]

        def tick():
            mark[1] += 1
            if mark[1] % pass_steps == 0:
                torch.cuda.synchronize()
                now = time.perf_counter()
                if mark[0] is not None:
                    times.append(1e3 * (now - mark[0]) / pass_steps)
                mark[0] = now
            if len(times) == passes:
                raise Done
        epochs = 1 + (passes + 1) * pass_steps // 64
        if model == "AAE":
            m = AdversarialAutoEncoder(n_hidden=h, n_code=c, batch_size=batch, n_epochs=epochs, conditions=conds, verbose=False, seed=1)
        else:
            m = DecodingRecommender(conds, n_epochs=epochs, batch_size=batch, n_hidden=h, verbose=False, seed=1)
        m.resident_conditions = flag
        step = m._run_step if model == "AAE" else m._step

        def timed(*a, **k):
            step(*a, **k)
            if sync:
                torch.cuda.synchronize()
            tick()
        setattr(m, "_run_step" if model == "AAE" else "_step", timed)
        try:
            m.fit(Xc, condition_data=data) if model == "AAE" else m.fit(data, Xc)
        except Done:
            pass
        assert len(times) == passes, len(times)
        t = times[warm:]
        return float(np.median(t)), f"{np.median(t):.3f} [{min(t):.3f}, {max(t):.3f}]"

    print(f"fit(), N={N} h={h}: median ms/step of {rounds} passes of {pass_steps} steps; resident_conditions False | True, two rounds each")
    if split:
        parts = (("3 blocks, no table", 3, False, True, False), ("the table alone", 0, True, True, False),
                 ("MPD, the table padded per step", 3, True, False, False), ("MPD", 3, True, True, False),
                 ("MPD, a synchronize after every step", 3, True, True, True))
        for tag, n_blocks, with_cat, cat_resident, sync in parts:
            med = {False: [], True: []}
            for flag in (False, True, False, True):
                med[flag].append(run("AAE", 1000, n_blocks, with_cat, False, flag, cat_resident, sync)[1])
            print(f"AAE      {tag:44s} host     {' | '.join(med[False]):>44s} {' | '.join(med[True]):>44s}", flush=True)
        return
    print(f"{'model':8s} {'cell':44s} {'feed':8s} {'False':>44s} {'True':>44s} {'False/True':>10s}")
    cells = (("1 x 300, batch 100", B, 1, False), ("1 x 300, batch 1000", 1000, 1, False),
             ("MPD: 3 x 300 + Categorical(32, sum), batch 1000", 1000, 3, True))
    for model in ("AAE", "Decoding"):
        for tag, batch, n_blocks, with_cat in cells:
            for on_device in (False, True):
                med = {False: [], True: []}
                for flag in (False, True, False, True):
                    med[flag].append(run(model, batch, n_blocks, with_cat, on_device, flag))
                ratio = np.mean([v for v, _ in med[False]]) / np.mean([v for v, _ in med[True]])
                print(f"{model:8s} {tag:44s} {'device' if on_device else 'host':8s} {' | '.join(s for _, s in med[False]):>44s} "
                      f"{' | '.join(s for _, s in med[True]):>44s} {ratio:10.2f}", flush=True)


if __name__ == "__main__":
    if "const" in sys.argv[1:]:
        const_rates(split="split" in sys.argv[1:])
    elif "ragged" in sys.argv[1:]:
        a = sys.argv[sys.argv.index("ragged") + 1:]
        ragged_rates(a[0], a[1], pass_steps=int(a[2]) if len(a) > 2 else 64)
    elif "opts" in sys.argv[1:]:
        if "fit" not in sys.argv[1:]:
            partial_fit_rates(opts=True)
        opts_fit_rates(order=(1, 0) if "reversed" in sys.argv[1:] else (0, 1))
    else:
        partial_fit_rates() if "bag" in sys.argv[1:] else fit_rates()
