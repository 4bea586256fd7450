"""Shared by test_popular_cpu.py and test_popular_gpu.py: the definition of the most-popular ranking in NumPy, and the builders
of the cases both files rank.

The definition (nothing of aaerec is used for it):
    order   = lexsort((ids, -counts)): count descending, the smaller id at equal counts;
    a row's list = the order with the row's known items removed; for held-out items the known items follow, by id;
    rank    = 1 + the place of the item in that sequence;
    scaled  = (c - min) / (max - min) in float64 over ALL items, 0 where max = min.
"""
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "most_popular.npz")

N = 300                                       # not a multiple of the 64 candidates a wavefront looks at per step
KNOWN = (0, 1, 63, 64, 65, 130, 297, 300)     # known items of a row: around one and two steps of 64, nearly all, all
KS = (1, 10, 64, 65, 300)
# fl(fl(v - min) * fl(1 / span)): the difference of two counts below 2^24 is exact in fp32, the reciprocal and the product
# round once each - (1 + 2^-24)^2 - 1 < 1.0001 * 2^-23 relative to the exact quotient (the bound of tests/test_cooc_gpu.py)
SCALED_RTOL = 1.0001 * 2.0 ** -23


class Rows:
    """The slice of the Bags interface MostPopular reads: tocsr() and size()."""

    def __init__(self, X):
        self.X = sp.csr_matrix(X)

    def tocsr(self):
        return self.X.copy()

    def size(self):
        return self.X.shape


def csr_of(rows, n_cols, dtype=np.float64):
    """Canonical CSR from per-row id lists (values 1)."""
    rows = [np.sort(np.asarray(r, dtype=np.int64)) for r in rows]
    ip = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows) if len(rows) and ip[-1] else np.zeros(0, dtype=np.int64)
    return sp.csr_matrix((np.ones(idx.size, dtype=dtype), idx.astype(np.int32), ip), shape=(len(rows), n_cols))


def counts_300(seed=5):
    """int64 [N]: counts in 1..11 (many ties), a block of 40 zero-count items, five items sharing the maximum 40."""
    r = np.random.default_rng(seed)
    c = r.integers(1, 12, size=N).astype(np.int64)
    c[100:140] = 0
    c[[3, 77, 150, 298, 299]] = 40
    return c


def training_set(counts):
    """A canonical CSR [max count, items] of ones whose column sums are `counts`: item j sits in rows 0 .. counts[j] - 1."""
    rows = [np.flatnonzero(counts > d) for d in range(int(counts.max()))]
    return csr_of(rows, counts.size)


def order_of(counts):
    counts = np.asarray(counts)
    return np.lexsort((np.arange(counts.size), -counts))


def test_rows(counts, seed=6):
    """(T, Y): a row of m known items for every m of KNOWN drawn at random, then one holding exactly the first m items of the
    order (whole steps of 64 candidates are masked and the next has to be opened); truth rows that mix new items, known items
    and empty rows."""
    r = np.random.default_rng(seed)
    n = counts.size
    order = order_of(counts)
    known = [np.sort(r.choice(n, size=m, replace=False)) for m in KNOWN] + [np.sort(order[:m]) for m in KNOWN]
    truth = []
    for i, kn in enumerate(known):
        new = np.setdiff1d(np.arange(n), kn)
        if i % 5 == 2:
            truth.append([])                                                            # an empty truth row
            continue
        t = list(r.choice(new, size=min(new.size, int(r.integers(1, 12))), replace=False)) if new.size else []
        if kn.size:
            t += list(r.choice(kn, size=min(kn.size, 3), replace=False))              # held-out items that are known items
        truth.append(t)
    return csr_of(known, n), csr_of(truth, n)


def want_topk(counts, T, k, exclude_known=True):
    """ids int64 [n, k] (-1 padded) and float64 scaled scores [n, k] from the definition."""
    counts = np.asarray(counts, dtype=np.int64)
    order = order_of(counts)
    lo, span = counts.min(), counts.max() - counts.min()
    ids = np.full((T.shape[0], k), -1, dtype=np.int64)
    val = np.zeros((T.shape[0], k), dtype=np.float64)
    for r in range(T.shape[0]):
        known = T.indices[T.indptr[r]:T.indptr[r + 1]] if exclude_known else np.zeros(0, dtype=np.int64)
        best = order[~np.isin(order, known)][:k]
        ids[r, :best.size] = best
        if span:
            val[r, :best.size] = (counts[best] - lo) / span
    return ids, val


def want_ranks(counts, T, Y, exclude_known=True):
    """int64 [nnz(Y)]: the rank of every stored entry of the canonical truth Y, CSR order, from the definition."""
    counts = np.asarray(counts, dtype=np.int64)
    order = order_of(counts)
    out = np.zeros(Y.nnz, dtype=np.int64)
    for r in range(Y.shape[0]):
        known = np.sort(T.indices[T.indptr[r]:T.indptr[r + 1]]) if exclude_known else np.zeros(0, dtype=np.int64)
        seq = np.concatenate([order[~np.isin(order, known)], known])
        place = np.empty(counts.size, dtype=np.int64)
        place[seq] = np.arange(counts.size)
        for e in range(Y.indptr[r], Y.indptr[r + 1]):
            out[e] = 1 + place[Y.indices[e]]
    return out


def check_scaled(val, want_val):
    """The device's / host route's fp32 scaled scores against the exact quotient: within SCALED_RTOL, exactly 0 where it is 0."""
    val = np.asarray(val, dtype=np.float64)
    assert (val[want_val == 0] == 0).all()
    np.testing.assert_allclose(val, want_val, rtol=SCALED_RTOL, atol=0)


EVAL_ITEMS, EVAL_TEST_BAGS, EVAL_YEAR = 30, 12, 2009


def evaluation_bags(seed=8):
    """Bags for Evaluation(…, EVAL_YEAR) whose training counts are pairwise distinct: training bag d (before EVAL_YEAR) holds the
    items j >= d, so item j occurs j + 1 times.  The test bags draw 3-6 items from the items 1 .. EVAL_ITEMS - 1: the
    minimum-count item 0 is never held out, so the dense pipeline - which scales it to the 0 it masks known items with - has no
    tie to break and every tie-breaking order gives the same numbers."""
    from aaerec.datasets import Bags
    r = np.random.RandomState(seed)
    data = [["i%d" % j for j in range(d, EVAL_ITEMS)] for d in range(EVAL_ITEMS)]
    years = [2000 + d % 9 for d in range(EVAL_ITEMS)]
    for _ in range(EVAL_TEST_BAGS):
        data.append(["i%d" % j for j in r.choice(np.arange(1, EVAL_ITEMS), size=r.randint(3, 7), replace=False)])
        years.append(EVAL_YEAR)
    owners = ["d%d" % i for i in range(len(data))]
    return Bags(data, owners, {"year": dict(zip(owners, years))})


def evaluation_setup(metrics, topk):
    """Evaluation over evaluation_bags(), set up, with what the docstring above promises checked on the split itself."""
    from aaerec import evaluation as E
    ev = E.Evaluation(evaluation_bags(), EVAL_YEAR, metrics=metrics, logfile=None, topk=topk).setup(min_elements=1, drop=1)
    counts = np.asarray(ev.train_set.tocsr().sum(0)).ravel()
    assert counts.size == EVAL_ITEMS and np.unique(counts).size == counts.size
    assert ev.y_test.shape[0] == EVAL_TEST_BAGS and ev.y_test.nnz == EVAL_TEST_BAGS
    assert int(np.argmin(counts)) not in set(ev.y_test.indices.tolist())
    return ev


def counting(rec):
    """rec with predict / predict_topk / predict_ranks wrapped to record their calls; returns the list of names called."""
    asked = []
    for name in ("predict", "predict_topk", "predict_ranks"):
        real = getattr(rec, name)
        setattr(rec, name, (lambda real, name: lambda *a, **kw: (asked.append(name), real(*a, **kw))[1])(real, name))
    return asked
