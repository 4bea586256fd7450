"""Shared by test_random_cpu.py and test_random_gpu.py: the definition of the random baseline's draws and of its ranking in NumPy,
built from tests/device_rng.py (nothing of aaerec is used for it), and the builders of the cases both files rank.

The definition:
    key     = rng_key(seed, draw, 0) ^ 15 * STREAM_MUL;  s(r, j) = hash_cell(key, r, j) >> (32 - bits);  score = s * 2^-bits
    order   = lexsort((ids, -s)): s descending, the smaller id at equal s;
    a row's list = the order with the row's known items removed; for held-out items the known items follow, by id;
    rank    = 1 + the place of the item in that sequence; 0 for an id outside [0, items);
    scaled  = (score - min) * inv in float32, span = max - min, inv = 1 / span where span > 0, else 1: min / max over ALL items.
"""
import functools

import numpy as np
import scipy.sparse as sp

import device_rng as D
from popular_cases import Rows, counting, csr_of                                      # noqa: F401  (re-exported)

STREAM = 15
SEED = 20261019
GRID_ITEMS = (1, 63, 64, 65, 4097, 70001)
GRID_KS = (1, 10, 32, 33, 500, 1024)
# (seed, row) of the test set whose 1024th and 1025th largest draws over 70 001 items are EQUAL at bits = 24 (the first row of
# seed 77 for which that holds: scan_tie_row below found it; test_random_cpu.py holds the record to the scan's condition)
TIE_SEED, TIE_ROW, TIE_ITEMS, TIE_K = 77, 27, 70001, 1024


def values(seed, draw, row0, n_rows, n_items, bits=24):
    """uint32 [n_rows, n_items]: s(r, j) for rows [row0, row0 + n_rows)."""
    key = D.rng_key(seed, draw, 0) ^ ((STREAM * D.STREAM_MUL) & D.M64)
    w = D.hash_cell(key, np.arange(n_rows, dtype=np.int64) + row0, np.arange(n_items, dtype=np.int64))
    return w >> np.uint32(32 - bits)


def scores(seed, draw, row0, n_rows, n_items, bits=24):
    return values(seed, draw, row0, n_rows, n_items, bits).astype(np.float32) * np.float32(2.0 ** -bits)


def boundary_ties(v, known, k):
    """True when the k-th and the (k + 1)-th best unknown items of a row of values v share a value."""
    u = np.sort(np.delete(np.asarray(v, dtype=np.int64), known))[::-1]
    return u.size > k and u[k - 1] == u[k]


def scan_tie_row(seed, n_items, k, rows=400, bits=24):
    """The first row r < rows of the test set, no item known, whose k-th and (k + 1)-th largest draws are equal (None: none)."""
    for r in range(rows):
        if boundary_ties(values(seed, 0, r, 1, n_items, bits)[0], np.zeros(0, dtype=np.int64), k):
            return r
    return None


def grid_rows(n_items, k, seed=4):
    """Canonical CSR of the row kinds every size is ranked over: an empty row, a row that knows all but k - 1 items (its list
    ends in the tail), a row that knows every item, three rows of ~20 random ids."""
    r = np.random.default_rng(seed + 31 * n_items + k)
    every = np.arange(n_items)
    rows = [[], np.sort(r.permutation(n_items)[:n_items - (k - 1)]), every]
    rows += [np.sort(r.choice(n_items, size=min(20, n_items), replace=False)) for _ in range(3)]
    return csr_of(rows, n_items)


def truth_rows(T, n_items, sizes=(0, 1, 64, 65, 4096, 65), seed=9):
    """Canonical CSR over max(n_items + 2000, 5000) columns: sizes[i] held-out ids for row i - up to three quarters of them inside
    [0, n_items) (known items of the row among them, three forced where the row has that many), the rest beyond n_items."""
    r = np.random.default_rng(seed + n_items)
    cols = max(n_items + 2000, 5000)
    out = []
    for i in range(T.shape[0]):
        size = sizes[i % len(sizes)]
        known = T.indices[T.indptr[i]:T.indptr[i + 1]]
        inside = r.choice(n_items, size=min((3 * size + 3) // 4, n_items), replace=False)
        if size >= 4 and known.size >= 3:
            inside = np.union1d(inside[:max(0, inside.size - 3)], known[:3])
        beyond = n_items + r.choice(cols - n_items, size=size - inside.size, replace=False)
        out.append(np.concatenate([inside, beyond]))
    return csr_of(out, cols)


@functools.lru_cache(maxsize=64)
def _full_order(seed, draw, row0, n_rows, n_items, bits):
    v = values(seed, draw, row0, n_rows, n_items, bits).astype(np.int64)
    order = np.stack([np.lexsort((np.arange(n_items), -v[i])) for i in range(n_rows)])
    v.setflags(write=False)
    order.setflags(write=False)
    return v, order


def want_topk(seed, draw, row0, T, k, exclude_known=True, bits=24):
    """ids int32 [n, k] (-1 padded) and float32 scaled scores [n, k] from the definition."""
    n, n_items = T.shape
    v, order = _full_order(seed, draw, row0, n, n_items, bits)
    ids = np.full((n, k), -1, dtype=np.int32)
    val = np.zeros((n, k), dtype=np.float32)
    unit = np.float32(2.0 ** -bits)
    for i in range(n):
        known = T.indices[T.indptr[i]:T.indptr[i + 1]] if exclude_known else np.zeros(0, dtype=np.int64)
        best = order[i][~np.isin(order[i], known)][:k] if known.size else order[i][:k]
        ids[i, :best.size] = best
        lo, hi = np.float32(v[i].min()) * unit, np.float32(v[i].max()) * unit
        span = np.float32(hi - lo)
        inv = np.float32(1) / span if span > 0 else np.float32(1)
        val[i, :best.size] = (v[i][best].astype(np.float32) * unit - lo) * inv
    return ids, val


def want_ranks(seed, draw, row0, T, Y, exclude_known=True, bits=24):
    """int32 [nnz(Y)]: the rank of every stored entry of the canonical truth Y, CSR order, from the definition."""
    n, n_items = T.shape
    _, order = _full_order(seed, draw, row0, n, n_items, bits)
    out = np.zeros(Y.nnz, dtype=np.int32)
    for i in range(n):
        if Y.indptr[i] == Y.indptr[i + 1]:
            continue
        known = np.sort(T.indices[T.indptr[i]:T.indptr[i + 1]]) if exclude_known else np.zeros(0, dtype=np.int64)
        seq = np.concatenate([order[i][~np.isin(order[i], known)], known])
        place = np.empty(n_items, dtype=np.int64)
        place[seq] = np.arange(n_items)
        for e in range(Y.indptr[i], Y.indptr[i + 1]):
            t = Y.indices[e]
            out[e] = 1 + place[t] if 0 <= t < n_items else 0
    return out


# ---- the class under Evaluation: 300 test rows over 5000 items ------------------------------------------------------------------
EVAL_ITEMS, EVAL_TEST_BAGS, EVAL_YEAR = 5000, 300, 2009


def evaluation_bags(seed=8):
    """Bags for Evaluation(..., EVAL_YEAR): 500 training bags of ten items cover the EVAL_ITEMS items once each; the test bags
    draw 5-12 of them."""
    from aaerec.datasets import Bags
    r = np.random.RandomState(seed)
    data = [["i%d" % j for j in range(10 * d, 10 * d + 10)] for d in range(EVAL_ITEMS // 10)]
    years = [2000 + d % 9 for d in range(len(data))]
    for _ in range(EVAL_TEST_BAGS):
        data.append(["i%d" % j for j in r.choice(EVAL_ITEMS, size=r.randint(5, 13), replace=False)])
        years.append(EVAL_YEAR)
    owners = ["d%d" % i for i in range(len(data))]
    return Bags(data, owners, {"year": dict(zip(owners, years))})


def evaluation_setup(metrics, metrics_on="host"):
    from aaerec import evaluation as E
    ev = E.Evaluation(evaluation_bags(), EVAL_YEAR, metrics=metrics, logfile=None, topk=True, metrics_on=metrics_on)
    ev.setup(min_elements=1, drop=1)
    assert ev.x_test.shape == (EVAL_TEST_BAGS, EVAL_ITEMS) and ev.y_test.nnz == EVAL_TEST_BAGS
    return ev


def forced_tie_case():
    """(T, Y, bits): 9 rows over 300 items at bits = 3 - eight values over 300 items, so every boundary of every list is a tie."""
    T = grid_rows(300, 10)
    T = sp.vstack([T, csr_of([[5, 6, 7], [], np.arange(0, 300, 2)], 300)]).tocsr()
    r = np.random.default_rng(12)
    Y = csr_of([np.sort(r.choice(300, size=s, replace=False)) for s in (3, 0, 5, 7, 1, 2, 4, 300, 6)], 300)
    return T, Y, 3
