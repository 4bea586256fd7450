"""GPU checks of the full-ranking path (csrc/rank_full.h, abi_rank.h): aae_predict_ranks / aae_decode_ranks - the 1-based
rank of every held-out item among its row's items, for the unbounded metrics ('mrr', 'map') the reference's drivers ask for.
Models, corpora and case shapes are those of tests/test_rank_long_gpu.py; tolerances are that file's: 2e-6 on scaled scores
for fp32 handles, 2e-3 for bf16.

 (a) exact agreement with predict_topk's lists (k = 32 and k = 1024) on the same handle
 (b) against the host pipeline on predict()'s matrix: every rank inside the interval the tolerance leaves open
 (c) structure: distinct ranks per row, rankable items in [1, n_rankable], known items beyond
 (d) decode_ranks, the model-level call, the custom op, chunked and repeated calls give identical ranks
 (e) Evaluation end to end with ['mrr', 'map', 'mrr@10'] against the dense route

Held-out items for (b).  An interval is "wide" when another rankable item's scaled score lies within the tolerance of the
held-out item's; the bound is hollow where most are.  The helper's scale of 8 on dec.lin3 is kept and the held-out items are
drawn uniformly from the row's rankable items (one known item is added where the case asks for one): on the oracle's
eval-mode predict for the parameters of the fp32 cases with N <= 5000 that leaves 1 - 5 % of the intervals wide at 2e-6
(tests/test_rank_full_cpu.py::test_oracle_intervals_are_narrow_for_the_chosen_truths measures and bounds it without a
device), inside the 10 % the check allows.  (Case ids seed parameters and draws; the dense-form case is 21: with 20 the
one-item-per-row draw happened to put 8 % of its 113 items on a near-tie in that oracle check - too close to the bound.)"""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_rank_long_gpu import _corpus, _dense, _model

pytestmark = pytest.mark.gpu

SLOTS = 8            # kFullSlots of csrc/rank_x3.h: held-out items a row and round of launches


def _scaled(full):
    lo, hi = full.min(1, keepdims=True), full.max(1, keepdims=True)
    return (full - lo) / np.where(hi > lo, hi - lo, 1.0)


def _truths(r, N, docs):
    """Two ground truths as sorted id lists per row, drawn uniformly from the items the row does not name: ONE item per
    row, and a MIXED one - row 0 none, row 1 a known item and two others, row 2 more items than the slot count (2 * SLOTS + 4,
    one of them known), the rest 0..12."""
    one, mixed = [], []
    for b, doc in enumerate(docs):
        free = np.setdiff1d(np.arange(N), doc)
        one.append(np.sort(r.choice(free, size=1)))
        m = 0 if b == 0 else 2 if b == 1 else 2 * SLOTS + 3 if b == 2 else int(r.integers(0, 13))
        t = r.choice(free, size=m, replace=False)
        if b in (1, 2):
            t = np.concatenate([t, r.choice(doc, size=1)])
        mixed.append(np.sort(t))
    return one, mixed


def _truth_csr(rows_ids, N, device):
    from aaerec._hip import DeviceCSR
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows_ids])]).astype(np.int64)
    idx = np.concatenate(rows_ids).astype(np.int32) if ip[-1] else np.zeros(0, dtype=np.int32)
    return DeviceCSR.from_arrays(ip, idx, np.ones(int(ip[-1]), dtype=np.float32), N, device), ip


def _intervals(full, docs, truth_rows, excl, tol):
    """Per truth entry (CSR order): [lo, hi] the ranks the host pipeline allows when scaled scores within tol may swap, and
    whether the item is a known one (then lo == hi == n_rankable + 1 + #{known ids < t})."""
    sc = _scaled(full.astype(np.float64))
    lo, hi, known = [], [], []
    for b, ts in enumerate(truth_rows):
        ok = np.ones(full.shape[1], dtype=bool)
        if excl:
            ok[docs[b]] = False
        s = sc[b][ok]
        for t in ts:
            if not ok[t]:
                rk = int(ok.sum()) + 1 + int(np.count_nonzero(np.asarray(docs[b]) < t))
                lo.append(rk); hi.append(rk); known.append(True)
            else:
                lo.append(1 + int(np.count_nonzero(s > sc[b, t] + tol)))
                hi.append(int(np.count_nonzero(s >= sc[b, t] - tol)))
                known.append(False)
    return np.asarray(lo), np.asarray(hi), np.asarray(known, dtype=bool)


def _topk_chunked(dev, csr, rows, k, cdev, excl):
    cap = dev.rank_max_rows(k)
    parts = [dev.predict_topk(csr, s, min(cap, rows - s), k, cond=None if cdev is None else cdev[s:s + cap].contiguous(),
                              exclude_known=excl)[0] for s in range(0, rows, cap)]
    return torch.cat(parts).cpu().numpy()


def _check(tag, dev, csr, docs, cdev, rows, R, excl, tol, truth_rows, full, narrow):
    N = full.shape[1]
    truth, ip = _truth_csr(truth_rows, N, dev.device)
    ranks = dev.predict_ranks(csr, 0, rows, truth, cond=cdev, exclude_known=excl).cpu().numpy()
    assert ranks.dtype == np.int32 and ranks.shape == (int(ip[-1]),)
    lo, hi, known = _intervals(full, docs, truth_rows, excl, tol)
    # (b) inside the interval of the host pipeline; known held-out items exactly
    wide = float(np.mean(hi[~known] > lo[~known])) if (~known).any() else 0.0
    print(f"{tag}: {ranks.size} held-out items, {int(known.sum())} of them known, wide intervals {100 * wide:.2f} %, "
          f"largest width {int((hi - lo).max()) + 1 if ranks.size else 0}, outside {int(np.count_nonzero((ranks < lo) | (ranks > hi)))}")
    assert np.all((ranks >= lo) & (ranks <= hi)), (tag, np.flatnonzero((ranks < lo) | (ranks > hi))[:10])
    if narrow:
        assert wide <= 0.10, (tag, wide)
    # (c) structure
    for b in range(rows):
        rr = ranks[ip[b]:ip[b + 1]]
        n_rankable = N - (len(docs[b]) if excl else 0)
        kn = known[ip[b]:ip[b + 1]]
        assert len(set(rr.tolist())) == rr.size, (tag, b, rr)
        assert np.all((rr[~kn] >= 1) & (rr[~kn] <= n_rankable)) and np.all(rr[kn] > n_rankable), (tag, b, rr, n_rankable)
    # (a) exactly the positions of predict_topk's lists on the same handle
    for k in (32, 1024):
        ids = _topk_chunked(dev, csr, rows, min(k, N), cdev, excl)
        for b in range(rows):
            for e in range(ip[b], ip[b + 1]):
                t, rk = truth_rows[b][e - ip[b]], ranks[e]
                if rk <= ids.shape[1]:
                    assert ids[b, rk - 1] == t, (tag, k, b, t, rk, ids[b, max(0, rk - 3):rk + 2])
                pos = np.flatnonzero(ids[b] == t)
                if pos.size:
                    assert rk == pos[0] + 1, (tag, k, b, t, rk, pos)
    # (d) the other call forms: a decoder input the caller built, chunks, the same call again.
    # The layer-chain front end the ranking calls share with predict_topk sums a layer in k-slices for calls of more than 224
    # rows and by columns below (abi_chains.h: ChainBuilder) - other roundings of the hidden activations - and aae_encode runs
    # max_batch rows at a time.  So "identical" is asked of calls that take one form: the first min(rows, 224) rows for the
    # decoder input, and for the chunks up to 224 rows in thirds, from 450 rows on in halves, in between the first 224 rows
    # in thirds.  The decoder-input call over ALL rows is held to the intervals of (b).
    cs = (lambda a, b: None if cdev is None else cdev[a:b].contiguous())
    z = torch.cat([dev.encode(csr, s, min(R, rows - s)) for s in range(0, rows, R)])
    zc = z if cdev is None else torch.cat([z, cdev], 1)
    dec = dev.decode_ranks(zc, csr, 0, truth, exclude_known=excl).cpu().numpy()
    assert np.all((dec >= lo) & (dec <= hi)), tag
    w = min(rows, 224)
    first = ranks if w == rows else dev.predict_ranks(csr, 0, w, truth, cond=cs(0, w), exclude_known=excl).cpu().numpy()
    assert np.array_equal(dec if w == rows else dev.decode_ranks(zc[:w], csr, 0, truth, exclude_known=excl).cpu().numpy(), first), tag
    w = rows if rows <= 224 or rows >= 450 else 224
    cuts = [0, w // 2, w] if w >= 450 else [0, max(1, w // 3), w]
    whole = ranks if w == rows else dev.predict_ranks(csr, 0, w, truth, cond=cs(0, w), exclude_known=excl).cpu().numpy()
    assert whole.size == ip[w]
    parts = [dev.predict_ranks(csr, a, b - a, truth, cond=cs(a, b), exclude_known=excl) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), whole), tag
    assert np.array_equal(dev.predict_ranks(csr, 0, rows, truth, cond=cdev, exclude_known=excl).cpu().numpy(), ranks), tag
    return ranks


def _full_case(case, N, h, c, inc, R, rows, excl, dtype, fused=True):
    if fused:
        dev, csr, docs, cdev = _model(case, N, h, c, inc, R, rows, dtype)
    else:
        os.environ["AAE_NO_RANK_FUSED"] = "1"
        try:
            dev, csr, docs, cdev = _model(case, N, h, c, inc, R, rows, dtype)
        finally:
            del os.environ["AAE_NO_RANK_FUSED"]
    cap = dev.rank_full_max_rows()
    print(f"case {case}: N={N} rows={rows} max_batch={R} rank_full_max_rows={cap} rank_max_rows(32)={dev.rank_max_rows(32)}")
    assert cap >= R and (fused or cap == R), (cap, R)
    if fused and N <= 100000:
        assert cap >= rows, (cap, rows)         # (one fused call takes the whole case: the [rows][8] arrays cost no rows)
    full = _dense(dev, csr, rows, R, cdev)
    r = np.random.default_rng(700 + case)
    one, mixed = _truths(r, N, docs)
    tol = 2e-6 if dtype == "f32" else 2e-3
    narrow = dtype == "f32" and N <= 5000
    _check(f"case {case} one per row", dev, csr, docs, cdev, rows, R, excl, tol, one, full, narrow)
    _check(f"case {case} mixed", dev, csr, docs, cdev, rows, R, excl, tol, mixed, full, narrow)
    return dev


CASES = [  # N, h, c, inc, max_batch, rows, exclude_known, dtype  (tests/test_rank_long_gpu.py::FUSED_CASES)
    (5000, 200, 50, 0, 512, 64, True, "f32"),
    (4587, 200, 50, 300, 512, 60, True, "f32"),        # C4's shape: a 300-wide condition
    (47000, 100, 50, 0, 100, 300, True, "bf16"),       # C2's shape in bf16 mode
    (100000, 200, 50, 0, 100, 512, True, "f32"),       # C3 x 512 rows
    (2900000, 200, 50, 0, 32, 40, True, "f32"),        # dec.lin3 beyond 2^31 bytes: the window instantiations
    (2000, 61, 20, 7, 512, 100, False, "f32"),         # nothing excluded
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fused_ranks_agree_with_the_lists_and_the_host_pipeline(case):
    N, h, c, inc, R, rows, excl, dtype = CASES[case]
    _full_case(case, N, h, c, inc, R, rows, excl, dtype)


def test_dense_form_of_a_handle_without_the_fused_launch():
    """NO_RANK_FUSED: max_batch rows per call through the score matrix (rank_full_dense_kernel) - same contract, same checks,
    chunks of max_batch rows."""
    _full_case(21, 5000, 200, 50, 0, 50, 113, True, "f32", fused=False)


def test_model_level_predict_ranks_and_the_custom_op():
    """AdversarialAutoEncoder.predict_ranks (a scipy CSR with the truth's canonical pattern) and
    torch.ops.aaerec.predict_ranks give the handle's ranks; an unsorted truth with a duplicate comes back canonical."""
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec import ops
    from aaerec._hip import DeviceCSR
    r = np.random.default_rng(11)
    N, n = 3000, 230
    X = sp.random(n, N, density=0.004, format="csr", random_state=3, dtype=np.float32)
    X.data[:] = 1.0
    X = X[np.diff(X.indptr) > 0]
    n = X.shape[0]
    m = AdversarialAutoEncoder(n_hidden=100, n_code=30, batch_size=50, n_epochs=1, verbose=False, seed=1)
    m.fit(X)
    assert m.hip.rank_full_max_rows() > 50          # (several chunks of the model-level call would be the dense form otherwise)
    rows_i = np.repeat(np.arange(n), 3)
    cols_i = r.integers(0, N, size=3 * n)
    rows_i, cols_i = np.concatenate([rows_i, rows_i[:5]]), np.concatenate([cols_i, cols_i[:5]])      # duplicates
    Y = sp.coo_matrix((np.ones(rows_i.size), (rows_i, cols_i)), shape=(n, N))
    got = m.predict_ranks(X, Y)
    want_pat = sp.csr_matrix(Y)
    want_pat.sum_duplicates(); want_pat.sort_indices()
    assert sp.issparse(got) and got.format == "csr" and got.shape == (n, N) and got.dtype == np.int32
    assert np.array_equal(got.indptr, want_pat.indptr) and np.array_equal(got.indices, want_pat.indices)
    csr, truth = DeviceCSR(X, m.hip.device), DeviceCSR(want_pat, m.hip.device)
    direct = m.hip.predict_ranks(csr, 0, n, truth).cpu().numpy()
    assert np.array_equal(got.data, direct)
    mid = ops.register_model(m.hip)
    op = torch.ops.aaerec.predict_ranks(mid, csr.indptr, csr.indices, csr.values, 0, n, int(csr.nnz_per_row_max), None,
                                        truth.indptr, truth.indices, int(truth.nnz_per_row_max), True)
    assert op.dtype == torch.int32 and np.array_equal(op.cpu().numpy(), direct)
    # and they are ranks: against the dense pipeline on the model's own predict()
    full = m.predict(X)
    full = (full.toarray() if sp.issparse(full) else np.asarray(full)).astype(np.float32)
    docs = [X.indices[X.indptr[b]:X.indptr[b + 1]] for b in range(n)]
    tr = [want_pat.indices[want_pat.indptr[b]:want_pat.indptr[b + 1]] for b in range(n)]
    lo, hi, _ = _intervals(full, docs, tr, True, 2e-6)
    assert np.all((direct >= lo) & (direct <= hi))


def test_evaluation_with_unbounded_metrics_end_to_end(capsys):
    """Evaluation on the Bags corpus of test_host_gpu.py::test_recommender_with_bags_and_evaluation_harness with the metrics
    the reference's drivers ask for: topk=True (predict_ranks + evaluate_ranks) against topk=False (the dense route), same
    seeds.  Equal to 1e-12 when no held-out item of the run has a wide interval at 2e-6; otherwise the means lie between the
    metrics of the intervals' two ends (every metric here falls when a rank grows)."""
    from aaerec.aae import AAERecommender
    from aaerec.datasets import Bags
    from aaerec.evaluation import Evaluation, evaluate_ranks
    rng = np.random.RandomState(0)
    protos = [rng.choice(300, size=8, replace=False) for _ in range(30)]
    data, owners, years = [], [], {}
    for i in range(600):
        p = protos[rng.randint(30)]
        data.append(["i%d" % t for t in rng.choice(p, size=rng.randint(4, 8), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // 600
    bags = Bags(data, owners, {"year": years})
    metrics = ["mrr", "map", "mrr@10"]
    asked = []

    class Rec(AAERecommender):
        def predict_ranks(self, test_set, y_true):
            asked.append("ranks")
            return super().predict_ranks(test_set, y_true)

        def predict(self, test_set):
            asked.append("dense")
            return super().predict(test_set)

    def run(topk):
        np.random.seed(3)
        torch.manual_seed(3)
        e = Evaluation(bags, 2009, metrics=metrics, logfile=None, topk=topk).setup(min_elements=2, drop=1)
        rec = Rec(n_hidden=40, n_code=16, n_epochs=10, batch_size=50, gen_lr=0.01, verbose=False, seed=11)
        return e, rec, np.asarray(e([rec])[0], dtype=np.float64)

    ef, recf, fast = run(True)
    assert asked == ["ranks"]
    ed, recd, dense = run(False)
    assert asked == ["ranks", "dense"]
    assert "- mrr:" in capsys.readouterr().out
    full = np.asarray(AAERecommender.predict(recd, ed.test_set), dtype=np.float32)
    x, y = sp.csr_matrix(ed.x_test), sp.csr_matrix(ed.y_test)
    y.sort_indices()
    docs = [x.indices[x.indptr[b]:x.indptr[b + 1]] for b in range(x.shape[0])]
    tr = [y.indices[y.indptr[b]:y.indptr[b + 1]] for b in range(y.shape[0])]
    lo, hi, known = _intervals(full, docs, tr, True, 2e-6)
    wide = int(np.count_nonzero(hi > lo))
    print(f"end to end: {y.nnz} held-out items, {wide} with a wide interval; topk {fast.tolist()} dense {dense.tolist()}")
    assert not known.any()
    if wide == 0:
        np.testing.assert_allclose(fast, dense, rtol=0, atol=1e-12)
    else:
        best = np.asarray(evaluate_ranks(sp.csr_matrix((lo, y.indices, y.indptr), shape=y.shape), metrics))[:, 0]
        worst = np.asarray(evaluate_ranks(sp.csr_matrix((hi, y.indices, y.indptr), shape=y.shape), metrics))[:, 0]
        for got in (fast, dense):
            assert np.all(got[:, 0] <= best + 1e-12) and np.all(got[:, 0] >= worst - 1e-12), (got, best, worst)


def test_predict_ranks_is_ten_times_faster_than_the_dense_route():
    """C3 x 512 rows, one held-out item per row, a model trained for 20 steps: the median of 5 regions of 5 predict_ranks
    calls (ranks on the host) against the dense route of the same run - predict() per max_batch rows, remove_non_missing and
    a full argsort on the host, what Evaluation did for 'mrr' / 'map' before.  The k = 32 list call is printed beside them."""
    import time
    from aaerec.aae import AdversarialAutoEncoder
    from aaerec._hip import DeviceCSR
    from aaerec.evaluation import remove_non_missing
    from tools.synth import throughput_corpus
    N, rows, B = 100000, 512, 100
    X = throughput_corpus(2048, N, seed=1234)
    m = AdversarialAutoEncoder(n_hidden=200, n_code=50, batch_size=B, n_epochs=1, verbose=False, seed=1)
    for _ in zip(range(20), m.fit_steps(X)):
        pass
    m._fit_finish()
    hip, csr = m.hip, DeviceCSR(X, m.hip.device)
    r = np.random.default_rng(0)
    truth, _ = _truth_csr([np.asarray([int(r.integers(0, N))]) for _ in range(rows)], N, hip.device)

    def dense_route():
        full = np.concatenate([hip.predict(csr, s, min(B, rows - s)).cpu().numpy() for s in range(0, rows, B)])
        return np.argsort(remove_non_missing(full, X[:rows], copy=False), axis=1)

    def median_ms(fn, regions, calls):
        fn()
        out = []
        for _ in range(regions):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / calls * 1e3)
        return sorted(out)[len(out) // 2]

    t_ranks = median_ms(lambda: hip.predict_ranks(csr, 0, rows, truth).cpu(), 5, 5)
    t_32 = median_ms(lambda: hip.predict_topk(csr, 0, rows, 32)[0].cpu(), 5, 5)
    t_dense = median_ms(dense_route, 3, 1)
    print(f"C3 x {rows} rows: predict_ranks {t_ranks:.3f} ms | predict_topk k=32 {t_32:.3f} ms ({t_ranks / t_32:.2f}x) | "
          f"dense route {t_dense:.1f} ms ({t_dense / t_ranks:.1f}x slower)")
    assert t_dense >= 10.0 * t_ranks, (t_dense, t_ranks)
