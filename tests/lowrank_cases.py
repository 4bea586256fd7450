"""Shared by tests/test_lowrank_cpu.py and tests/test_lowrank_gpu.py: the recorded fixtures of the reference's SVDRecommender
(tests/golden/svd_*.npz, tools/gen_golden.py svd), the generated device cases, and the acceptance rule.

What "equal to the reference" means.  The reference computes in float64, the device in fp32, so near-ties are decided by
rounding.  With S the float64 scores of a row (known items removed) and

    tol_rj = c * 2^-23 * (dims + nnz_r + 8) * sum_d |h_rd| |V_dj|        (float64; c = 1: the fp32 matrix pipe, csrc/lowrank.h)

an item t reported at 0-based position p is accepted iff lo <= p <= hi,
    lo = #{j : S_j > S_t + tol_rt + tol_rj},    hi = #{j : S_j >= S_t - tol_rt - tol_rj} - 1.
So that the interval cannot hide a wrong kernel, the share of checked entries with hi > lo is at most AMBIGUOUS_CAP per case,
computed from the reference scores alone (ambiguous_share)."""
import os

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C_ARITH = 1.0                   # the fp32 pipe (an emulated form would quote DESIGN 3.1's factor here)
AMBIGUOUS_CAP = 0.05
N_ITEMS, N_FEATURES = 1003, 1003 + 37
ZERO_ITEMS = (7, 500, 1002)     # items never seen in training: zero columns of V, scores that tie exactly at 0
GPU_CASES = [(1, 70, 101), (3, 1, 102), (10, 257, 103), (100, 70, 104), (260, 257, 105)]      # (dims, rows, seed)
GPU_KS = (1, 10, 33, 500)


class Titled:
    """The slice of the Bags interface SVDRecommender reads: tocsr() and get_single_attribute('title')."""

    def __init__(self, X, titles=None):
        self.X, self.titles = sp.csr_matrix(X), None if titles is None else [str(t) for t in titles]

    def tocsr(self):
        return self.X.copy()

    def get_single_attribute(self, name):
        assert name == "title"
        return list(self.titles)


def _csr(z, prefix, n_cols, data=True):
    ip, idx = z[prefix + "_indptr"], z[prefix + "_indices"]
    val = z[prefix + "_data"] if data else np.ones(idx.size)
    return sp.csr_matrix((val.astype(np.float64), idx, ip), shape=(ip.size - 1, n_cols))


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = int(z["n_items"])
    fx = dict(name=name, dims=int(z["dims"]), use_title=bool(int(z["use_title"])), random_state=int(z["random_state"]), N=N,
              train=_csr(z, "train", N), test=_csr(z, "test", N), truth=_csr(z, "truth", N, data=False),
              train_titles=z["train_titles"].tolist(), test_titles=z["test_titles"].tolist(),
              components=z["components"], pred=z["pred"], model_str=str(z["model_str"]), z=z)
    if fx["use_title"]:
        fx["tfidf_terms"], fx["tfidf_idf"] = z["tfidf_terms"].tolist(), z["tfidf_idf"]
    return fx


def recorded_class(components):
    """SVDRecommender whose fit() takes the recorded components instead of running the randomised solver: everything else -
    the tf-idf fit over the training titles, the stacking, the device table - is the class's own."""
    from aaerec.lowrank import SVDRecommender

    class Recorded(SVDRecommender):
        def fit(self, X, y=None):
            assert X.shape[1] == components.shape[1], (X.shape, components.shape)
            self._dev = self._dev_of = None
            self.svd.components_ = np.array(components, dtype=np.float64)
            return self

    return Recorded


def fixture_model(fx, device, **kw):
    rec = recorded_class(fx["components"])(fx["dims"], use_title=fx["use_title"], random_state=fx["random_state"], device=None, **kw)
    rec.train(Titled(fx["train"], fx["train_titles"]))
    rec.device = device
    return rec


def fixture_features(fx, rec):
    """float64 CSR [n_test, features] as the model reads the test rows."""
    return sp.csr_matrix(rec._features(Titled(fx["test"], fx["test_titles"])), dtype=np.float64)


# ---- generated cases ------------------------------------------------------------------------------------------------
def gpu_case(dims, rows, seed):
    """V [dims, 1040] float64 with a power-law spectrum (row d scaled by (1 + d)^-1.5, as the components of a fitted
    TruncatedSVD weigh in through the singular directions the data has: a flat spectrum of 260 equal directions makes every
    score a sum of 260 cancelling terms and a quarter of the middle of the ranking ambiguous) and three zero item columns; `rows` feature rows: sparse bags of 3-30
    items plus 0-8 title weights, and where there is room row 1 empty, row 2 naming all but two items, row 3 holding 3000
    entries (every id several times: the sum of duplicates in CSR order is the row's value).  The raw arrays keep the
    duplicates; F is the summed matrix the float64 reference uses; X = F[:, :1003] names the known items; Y the held-out
    items: two from the head of the reference ranking, three others, and in row 0 one known item."""
    r = np.random.default_rng(seed)
    V = r.standard_normal((dims, N_FEATURES)) * ((1.0 + np.arange(dims)) ** -1.5)[:, None]
    V[:, list(ZERO_ITEMS)] = 0.0
    ip, idx, val = [0], [], []
    for i in range(rows):
        if i == 1 and rows > 3:
            ids, x = np.zeros(0, dtype=np.int64), np.zeros(0)
        elif i == 2 and rows > 3:
            ids = np.delete(np.arange(N_ITEMS), [11, 640])
            x = np.ones(ids.size)
        elif i == 3 and rows > 3:
            ids = r.integers(0, N_FEATURES, size=3000)
            x = r.integers(1, 4, size=3000) * 0.25
        else:
            items = r.choice(N_ITEMS, size=int(r.integers(3, 31)), replace=False)
            words = N_ITEMS + r.choice(N_FEATURES - N_ITEMS, size=int(r.integers(0, 9)), replace=False)
            ids = np.concatenate([np.sort(items), np.sort(words)])
            x = np.concatenate([np.ones(items.size), r.random(words.size)])
        idx.append(ids)
        val.append(x)
        ip.append(ip[-1] + ids.size)
    ip, idx, val = np.asarray(ip, dtype=np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float32).astype(np.float64)
    F = sp.csr_matrix((val.copy(), idx.copy(), ip.copy()), shape=(rows, N_FEATURES))       # (summed in place below: not the raw arrays)
    nnz_raw = np.diff(ip)
    F.sum_duplicates()
    F.sort_indices()
    X = sp.csr_matrix(F[:, :N_ITEMS])
    X.sort_indices()
    ref = reference(V, F, X, nnz_raw)
    truth = []
    for i in range(rows):
        order = ref["order"][i]
        ok = order[~np.isin(order, ZERO_ITEMS)]
        head = r.choice(ok[:40], size=min(2, ok.size), replace=False).tolist() if ok.size else []
        rest = [int(t) for t in r.choice(ok, size=min(5, ok.size), replace=False) if t not in head][:3] if ok.size else []
        known = X.indices[X.indptr[i]:X.indptr[i + 1]]
        extra = [int(known[0])] if i == 0 and known.size else []
        truth.append(sorted(set(int(t) for t in head + rest + extra)))
    Y = sp.csr_matrix((np.ones(sum(map(len, truth))), np.concatenate([np.asarray(t, dtype=np.int64) for t in truth]) if truth else [],
                       np.concatenate([[0], np.cumsum([len(t) for t in truth])])), shape=(rows, N_ITEMS))
    return dict(dims=dims, rows=rows, V=V, raw=(ip, idx, val.astype(np.float32)), F=F, X=X, Y=Y, ref=ref)


# ---- the float64 reference and the acceptance rule -------------------------------------------------------------------
def reference(V, F, X, nnz=None, n_items=None, c=C_ARITH):
    """Float64 scores S [n, items], tol [n, items], and per row: the rankable items best first by (-S, id) (`order`)."""
    n_items = X.shape[1] if n_items is None else n_items
    V = np.asarray(V, dtype=np.float64)
    F = sp.csr_matrix(F, dtype=np.float64)
    H = np.asarray(F @ V.T)
    S = H @ V[:, :n_items]
    nnz = np.diff(F.indptr) if nnz is None else np.asarray(nnz)
    tol = c * 2.0 ** -23 * (V.shape[0] + nnz + 8)[:, None] * (np.abs(H) @ np.abs(V[:, :n_items]))
    order = []
    for i in range(S.shape[0]):
        known = X.indices[X.indptr[i]:X.indptr[i + 1]]
        o = np.lexsort((np.arange(n_items), -S[i]))
        order.append(o[~np.isin(o, known)])
    return dict(S=S, tol=tol, order=order)


def intervals(S_row, tol_row, rankable, items):
    """(lo, hi) of `items` (rankable ids) among the rankable items of one row."""
    s, t = S_row[rankable], tol_row[rankable]
    down, up = np.sort(s - t), np.sort(s + t)
    a, b = S_row[items] + tol_row[items], S_row[items] - tol_row[items]
    lo = down.size - np.searchsorted(down, a, side="right")          # #{j : S_j - tol_j > S_t + tol_t}
    hi = up.size - np.searchsorted(up, b, side="left") - 1           # #{j : S_j + tol_j >= S_t - tol_t} - 1
    return lo, hi


def ambiguous_share(ref, k=None, truth=None, X=None, tol=True):
    """Share of checked entries whose interval is wider than one place: the reference's k best of every row, or the
    (rankable) held-out items."""
    wide = total = 0
    for i, order in enumerate(ref["order"]):
        if truth is not None:
            t = truth.indices[truth.indptr[i]:truth.indptr[i + 1]]
            items = t[np.isin(t, order)]
        else:
            items = order[:k]
        if not items.size:
            continue
        lo, hi = intervals(ref["S"][i], ref["tol"][i] if tol else np.zeros_like(ref["tol"][i]), order, items)
        wide += int(np.count_nonzero(hi > lo))
        total += items.size
    return wide / max(1, total)


def check_topk(ref, X, ids, val, k, tol=True):
    """The acceptance rule over a [n, k] list: distinct ids, no known item, no -1 while rankable items remain, every entry
    inside its interval, every scaled score within its bound."""
    n = len(ref["order"])
    assert ids.shape == val.shape == (n, k) and ids.dtype == np.int32 and val.dtype == np.float32
    for i in range(n):
        order, S, T = ref["order"][i], ref["S"][i], ref["tol"][i] if tol else np.zeros_like(ref["tol"][i])
        m = min(k, order.size)
        got = ids[i, :m].astype(np.int64)
        assert (got >= 0).all() and (ids[i, m:] == -1).all() and (val[i, m:] == 0).all(), i
        assert np.unique(got).size == m and np.isin(got, order).all(), i
        if not m:
            continue
        lo, hi = intervals(S, T, order, got)
        p = np.arange(m)
        bad = np.flatnonzero((p < lo) | (p > hi))
        assert not bad.size, (i, bad[:5], got[bad[:5]], lo[bad[:5]], hi[bad[:5]])
        jmin, jmax = int(np.argmin(S)), int(np.argmax(S))
        span = S[jmax] - S[jmin]
        if span > 0:
            want = (S[got] - S[jmin]) / span
            bound = (T[got] + T[jmin] + T[jmax]) / span + 2.0 ** -24 * np.maximum(1.0, np.abs(want))
            err = np.abs(val[i, :m].astype(np.float64) - want)
            assert (err <= bound).all(), (i, float(err.max()), float(bound[np.argmax(err - bound)]))


def check_ranks(ref, X, Y, ranks, tol=True):
    """The acceptance rule over the ranks of the held-out items (CSR order of the canonical Y)."""
    n = len(ref["order"])
    e = 0
    for i in range(n):
        order, S, T = ref["order"][i], ref["S"][i], ref["tol"][i] if tol else np.zeros_like(ref["tol"][i])
        known = X.indices[X.indptr[i]:X.indptr[i + 1]]
        for t in Y.indices[Y.indptr[i]:Y.indptr[i + 1]]:
            if t in known:
                assert ranks[e] == order.size + 1 + np.count_nonzero(known < t), (i, t, ranks[e])
            else:
                lo, hi = intervals(S, T, order, np.asarray([t]))
                assert lo[0] <= ranks[e] - 1 <= hi[0], (i, t, ranks[e], lo[0], hi[0])
            e += 1
    assert e == len(ranks)
