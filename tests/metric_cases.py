"""Shared by test_metrics_cpu.py and test_metrics_gpu.py: the definitions of the rank-based metrics in exact arithmetic
(`fractions.Fraction`) and NumPy, and the builders of the cases both files score.  Nothing of aaerec is used here.

With a row's stored ranks ordered by (rank, position in the row) - r_1 <= ... <= r_m, j the 1-based place - and the cap k
(None: unbounded), h = #{r_j <= k}; a stored ABSENT counts towards m and is never <= k:

    mrr      1 / r_1 if r_1 <= k, else 0                        p        h / k
    map      (sum_{j <= h} j / r_j) / h, 0 if h = 0             r-prec   #{r_j <= min(m, k)} / m
    ndcg     (sum_{j <= h} d[r_j]) / (sum_{i <= min(k, m)} d[i])   clicks   (r_1 - 1) // 10 if r_1 <= k, else k / 10 + 1

d[i] is the DOUBLE 1 / log2(1 + i) of the table the code under test reads, taken exactly.  A row without entries scores 0,
clicks k / 10 + 1 - in doubles, `k / 10.0 + 1`, the reference's own expression (mpd_metrics.py:144), where there is no hit.

Error bounds (u = 2^-53, every term positive):
  * mrr, p, r-prec, clicks are one correctly rounded division of two integers: the result is the double nearest the exact
    value, `float(Fraction)`.
  * map sums h terms fl(j / r_j), each within u of its exact value, with h - 1 additions and one division: at most
    (h + 1) roundings, (1 + u)^(h + 1) - 1 <= (h + 2) u for h <= 2^20.
  * ndcg sums h table entries, then min(k, m) table entries, and divides: (h - 1) + (min(k, m) - 1) + 1 roundings.
  With t the number of summed terms (h; h + min(k, m) for ndcg) a computed value lies within (t + 2) u of the exact one,
  relatively - in ANY summation order, NumPy's pairwise sum included - and two computed values within 2 (t + 2) u of each other.
"""
import functools
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "challenge_metrics.npz")
OLD_GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics.npz")

ABSENT = 2 ** 31 - 1
U = 2.0 ** -53
KINDS = ("mrr", "map", "p", "ndcg", "r-prec", "clicks")
KIND_CODE = {kind: i for i, kind in enumerate(KINDS)}
EXACT_KINDS = ("mrr", "p", "r-prec", "clicks")
KS = (1, 5, 10, 64, 65, 500, 1024)
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096)
ROW_MAX = 4096


def name_of(kind, k):
    return kind if k is None else "{}@{}".format(kind, k)


def table(K):
    """The reference's discounts (eval/mpd/mpd_metrics.py:80) as doubles: d[i] at index i - 1."""
    return 1.0 / np.log2(1 + np.arange(1, int(K) + 1))


def all_specs():
    """Every kind at every k of KS, and the two unbounded ones: 44 (kind, k)."""
    return [(kind, k) for kind in KINDS for k in KS] + [("mrr", None), ("map", None)]


def specs_32():
    """32 of them for one full call: each kind at five of the seven caps - the window of five moves by one from kind to kind, so
    every cap meets at least four kinds - and the two unbounded ones."""
    out = []
    for i, kind in enumerate(KINDS):
        out += [(kind, KS[(i + s) % len(KS)]) for s in range(5)]
    return out + [("mrr", None), ("map", None)]


def exact(kind, k, ranks, d):
    """(the exact value as a Fraction, t = the number of summed terms) of one row; ranks in stored order, d the table doubles."""
    ranks = [int(r) for r in ranks]
    m = len(ranks)
    if m == 0:
        return (Fraction(k / 10.0 + 1.0) if kind == "clicks" else Fraction(0)), 0
    srt = sorted(ranks)                                     # (equal ranks: their j differ, their values do not)
    inside = lambda r, cap: r != ABSENT and (cap is None or r <= cap)      # noqa: E731
    h = sum(1 for r in srt if inside(r, k))
    if kind == "mrr":
        return (Fraction(1, srt[0]) if inside(srt[0], k) else Fraction(0)), 0
    if kind == "p":
        return Fraction(h, k), 0
    if kind == "r-prec":
        return Fraction(sum(1 for r in srt if inside(r, min(m, k))), m), 0
    if kind == "clicks":
        return (Fraction((srt[0] - 1) // 10) if inside(srt[0], k) else Fraction(k / 10.0 + 1.0)), 0
    if kind == "map":
        return (sum(Fraction(j + 1, srt[j]) for j in range(h)) / h if h else Fraction(0)), h
    ideal = min(k, m)
    if not h:
        return Fraction(0), 0
    return sum(Fraction(float(d[srt[j] - 1])) for j in range(h)) / sum(Fraction(float(d[i])) for i in range(ideal)), h + ideal


def check_value(got, want, t, kind, what=""):
    """One computed value against the exact one: the nearest double for the one-division kinds, (t + 2) u relative otherwise."""
    got = float(got)
    if kind in EXACT_KINDS:
        assert got == float(want), (what, kind, got, float(want))
    else:
        err = abs(Fraction(got) - want)
        assert err <= Fraction((t + 2) * U) * want, (what, kind, got, float(want), float(err / want) if want else None, t)


# ---- the rows of the one device call ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_rows():
    """(indptr int64, ranks int32): one row per length of LENGTHS, then five more.  Ranks are drawn without repetition from
    1 .. 6000 (small denominators keep the exact sums quick), a few of every row of 63 to 257 entries replaced by large ones up
    to 2^31 - 2, and stored in random order.  Rows of 2, 65, 257 and 4096 entries also carry ABSENT (twice where they can).  The
    extra rows: two pairs of equal ranks (both of a pair are counted, at consecutive places j - which of the two comes first shows
    in no value, so the position half of the ordering is not observable here), ABSENT alone, a first rank beyond every cap, all
    of 1 .. 64 in descending order, and a row of 64 with its hits at the caps themselves."""
    r = np.random.RandomState(4096)
    rows = []
    for m in LENGTHS:
        x = r.choice(6000, size=m, replace=False).astype(np.int64) + 1
        if 63 <= m <= 257:
            x[r.choice(m, size=5, replace=False)] = [2 ** 31 - 2, 2 ** 31 - 3, 2 ** 30 + 1, 70001, 1025]
        if m in (2, 65, 257, 4096):
            x[r.choice(m, size=min(2, m - 1), replace=False)] = ABSENT
        rows.append(x)
    rows.append(np.array([7, 3, 7, 12, 3], dtype=np.int64))
    rows.append(np.array([ABSENT], dtype=np.int64))
    rows.append(np.array([2000, 1500, 2 ** 31 - 2], dtype=np.int64))
    rows.append(np.arange(64, 0, -1, dtype=np.int64))
    rows.append(np.concatenate([np.array([1, 5, 10, 64, 65, 500, 1024, 2, 6, 11, 66, 501, 1025]), 3000 + np.arange(51)]).astype(np.int64))
    indptr = np.concatenate([[0], np.cumsum([x.size for x in rows])]).astype(np.int64)
    ranks = np.concatenate(rows).astype(np.int32)
    ranks.setflags(write=False)
    indptr.setflags(write=False)
    return indptr, ranks


@functools.lru_cache(maxsize=None)
def device_rows_exact():
    """{(kind, k): [(Fraction, t) per row]} of device_rows() for every spec of all_specs(), against table(max KS)."""
    indptr, ranks = device_rows()
    d = table(max(KS))
    return {(kind, k): [exact(kind, k, ranks[indptr[i]:indptr[i + 1]], d) for i in range(indptr.size - 1)] for kind, k in all_specs()}


# ---- mean and variance -----------------------------------------------------------------------------------------------------
FINISH_SIZES = (1, 2, 63, 257, 1000)


def finish_values(n, seed=0):
    """n non-negative doubles as a metric's per-row values are: some zeros, some ones, the rest spread over ten decades."""
    r = np.random.RandomState(100 + seed + n)
    x = r.rand(n) * 10.0 ** r.randint(-8, 2, size=n)
    x[r.rand(n) < 0.2] = 0.0
    x[r.rand(n) < 0.1] = 1.0
    return x


def exact_mean_var(x):
    fx = [Fraction(float(v)) for v in x]
    mean = sum(fx) / len(fx)
    return mean, sum((v - mean) ** 2 for v in fx) / len(fx)


def check_mean_std(mean, std, x, extra_rel=0.0):
    """(mean, std) of the doubles x against their exact mean and variance: the mean within (n + 1) u relative - n - 1 additions
    of non-negative terms and one division - and std^2 within (n + 8) 2^-52 max x^2 absolute: the mean's error e shifts every
    deviation by e, its cross term sum_i (x_i - mean) e vanishes and e^2 is second order; each squared deviation rounds twice
    (the difference, the square), the n - 1 additions and the division once each, all relative to terms of at most max x^2,
    and sqrt then squaring add three more roundings.  extra_rel: what the x themselves may be off by (relative), for values
    that were computed rather than given."""
    n = len(x)
    want_mean, want_var = exact_mean_var(x)
    top = Fraction(float(np.max(np.abs(x)))) if n else Fraction(0)
    assert abs(Fraction(float(mean)) - want_mean) <= Fraction((n + 1) * U + extra_rel) * abs(want_mean), (n, float(mean), float(want_mean))
    var = Fraction(float(std)) ** 2
    assert abs(var - want_var) <= Fraction((n + 8) * 2.0 ** -52 + 4 * extra_rel) * top * top, (n, float(var), float(want_var))


# ---- lists to ranks --------------------------------------------------------------------------------------------------------
LIST_KS = (1, 10, 64, 65, 1024)


def list_case(K, seed=0):
    """(ids int32 [n, K] with -1 padding and one id listed twice where K allows, truth indptr, truth indices - ascending per
    row, two rows empty) over 3000 items."""
    r = np.random.RandomState(50 + K + seed)
    n, items = 9, 3000
    ids = np.full((n, K), -1, dtype=np.int32)
    truth = []
    for i in range(n):
        fill = K if i % 3 else K - (K + 2) // 3                         # (every third row ends in padding: all of it at K = 1)
        ids[i, :fill] = r.choice(items, size=fill, replace=False)
        if fill >= 4:
            ids[i, fill - 1] = ids[i, 1]                                # (a duplicated id: its smaller position counts)
        if i in (2, 7):
            truth.append(np.zeros(0, dtype=np.int64))
            continue
        inside = r.choice(ids[i, :fill], size=min(fill, 1 + r.randint(6)), replace=False) if fill else np.zeros(0, dtype=np.int64)
        if fill >= 4:
            inside = np.append(inside, ids[i, 1])
        outside = r.choice(items, size=1 + r.randint(70), replace=False)
        truth.append(np.unique(np.concatenate([inside, outside])))
    indptr = np.concatenate([[0], np.cumsum([t.size for t in truth])]).astype(np.int64)
    return ids, indptr, np.concatenate(truth).astype(np.int32)


def want_ranks_from_lists(ids, indptr, indices):
    """int32 [nnz]: position + 1 of every truth entry among its row's ids (the first one of a repeated id), ABSENT otherwise."""
    out = np.full(indices.size, ABSENT, dtype=np.int32)
    for i in range(indptr.size - 1):
        for e in range(indptr[i], indptr[i + 1]):
            at = np.flatnonzero(ids[i] == indices[e])
            if at.size:
                out[e] = at[0] + 1
    return out


# ---- the fixture -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    """challenge_metrics.npz with the ranks of its targets in its rankings: (z, indptr, ranks int32 in CSR order)."""
    z = np.load(GOLDEN)
    perms, indptr, indices = z["rankings"], z["indptr"], z["indices"]
    ranks = np.zeros(indices.size, dtype=np.int32)
    for i in range(indptr.size - 1):
        place = np.empty(perms.shape[1], dtype=np.int64)
        place[perms[i]] = np.arange(perms.shape[1])
        ranks[indptr[i]:indptr[i + 1]] = place[indices[indptr[i]:indptr[i + 1]]] + 1
    return z, indptr, ranks


def fixture_names():
    """[(name, row of reference values [n], kind, k)] of the fixture: the challenge's three at its five caps, then METRICS."""
    z, _, _ = fixture()
    out = []
    for kind in ("r-prec", "ndcg", "clicks"):
        for i, k in enumerate(z["ks"].tolist()):
            out.append((name_of(kind, k), z[kind][i], kind, k))
    for name, vals in zip(z["metric_names"].tolist(), z["metric_values"]):
        kind, _, k = name.partition("@")
        out.append((name, vals, kind.lower(), int(k) if k else None))
    return out


def summed_terms(kind, k, indptr, ranks):
    """float64 [n]: t of every row - h = #{r_j <= k, r_j != ABSENT} for map (k None: unbounded), h + min(k, m) for ndcg."""
    indptr, ranks = np.asarray(indptr), np.asarray(ranks)
    m = np.diff(indptr)
    rows = np.repeat(np.arange(m.size), m)
    inside = (ranks != ABSENT) & (True if k is None else ranks <= k)
    h = np.bincount(rows[inside], minlength=m.size).astype(np.float64)
    return h + (np.where(h > 0, np.minimum(m, k), 0) if kind == "ndcg" else 0)


def check_against_fixture(got, want, kind, k, indptr, ranks):
    """Per-row values against the reference's: equal for the one-division kinds, within 2 (t + 2) u relative for map and ndcg,
    t the number of terms the row sums (summed_terms)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if kind in EXACT_KINDS:
        np.testing.assert_array_equal(got, want)
        return
    t = summed_terms(kind, k, indptr, ranks)
    rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print(name_of(kind, k), "largest difference in units of (t + 2) u:", float((rel / ((t + 2) * U)).max()))
    assert (np.abs(got - want) <= 2 * (t + 2) * U * np.abs(want)).all(), (kind, k, float((rel / ((t + 2) * U)).max()))
