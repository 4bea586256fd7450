"""What the rank-based metrics (aaerec/evaluation.py, aaerec/ranking.py, csrc/rank_metrics.h, csrc/abi_metrics.h) need no device
for: the library's surface and its argument checks, the metric names, the host forms against the reference's recorded values
(tests/golden/challenge_metrics.npz) and against the function they replace, lists against ranks, and the guards of the device
route.  Definitions and bounds: tests/metric_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import metric_cases as MC


# ---- the library's surface -----------------------------------------------------------------------------------------------
CALLS = ("aae_metric_rows", "aae_metric_finish", "aae_ranks_from_lists")


def test_library_header_and_prototypes_agree_and_the_abi_version_stands():
    from aaerec import _hip
    lib = _hip.load_library()
    for name in CALLS:
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    with open(os.path.join(MC.ROOT, "include", "aaerec_hip.h")) as fh:
        text = fh.read()
    assert "#define AAE_ABI_VERSION 4" in text
    for piece in [name + "(" for name in CALLS] + ["typedef struct aae_metric_spec {", "typedef struct aae_rank_rows {",
                                                  "typedef enum aae_metric_kind {", "#define AAE_METRIC_MAX 32",
                                                  "#define AAE_METRIC_ROW_MAX 4096", "#define AAE_RANK_ABSENT 2147483647",
                                                  "evaluation.py:94-164", "rank_metrics_with_std.py", "eval/mpd/mpd_metrics.py:43-144"]:
        assert piece in text, piece
    for i, kind in enumerate(("MRR", "MAP", "P", "NDCG", "RPREC", "CLICKS")):
        assert "AAE_METRIC_{} = {}".format(kind, i) in text
    assert (_hip.METRIC_MAX, _hip.METRIC_ROW_MAX, _hip.RANK_ABSENT) == (32, 4096, 2 ** 31 - 1)
    assert _hip.METRIC_KINDS == MC.KIND_CODE
    # the argument lists of the prototypes are those of the header: one ctypes argument per C parameter
    for name in CALLS:
        decl = text[text.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_hip._PROTOS[name][1]), name
    for name in ("rank_metrics", "ranks_from_lists", "discount_table"):
        assert callable(getattr(_hip, name)), name
    assert hasattr(_hip.DeviceDiscounts, "get")
    np.testing.assert_array_equal(_hip.discount_table(7), MC.table(7))
    assert C.sizeof(_hip.AaeMetricSpec) == 8


def _args(**over):
    """Well-formed calls over pointers nothing may dereference, one argument replaced."""
    from aaerec import _hip
    p = 0x1000
    rows, truth = _hip.AaeRankRows(), _hip.AaeBatch()
    rows.indptr_dev = rows.ranks_dev = p
    rows.n_rows = 5
    truth.indptr_dev = truth.indices_dev = truth.values_dev = p
    truth.n_rows = 4
    a = dict(rows=rows, specs=[(0, 0), (1, 10), (2, 5), (3, 20), (4, 7), (5, 500)], n_metrics=None, disc=p, n_disc=20, per_row=p, ld=5,
             vals=p, fin_ld=9, fin_n=9, fin_metrics=3, out=p, ids=p, ids_ld=10, k=10, truth=truth, ranks=p)
    a.update(over)
    return a


def _call(lib, which, a):
    from aaerec import _hip
    ref = lambda s: None if s is None else C.byref(s)      # noqa: E731
    if which == "rows":
        specs = a["specs"]
        arr = None if specs is None else (_hip.AaeMetricSpec * max(1, len(specs)))(*[_hip.AaeMetricSpec(kind, k) for kind, k in specs])
        n = a["n_metrics"] if a["n_metrics"] is not None else len(specs)
        return lib.aae_metric_rows(ref(a["rows"]), arr, n, a["disc"], a["n_disc"], a["per_row"], a["ld"], None)
    if which == "finish":
        return lib.aae_metric_finish(a["vals"], a["fin_ld"], a["fin_n"], a["fin_metrics"], a["out"], None)
    return lib.aae_ranks_from_lists(a["ids"], a["ids_ld"], a["k"], ref(a["truth"]), a["ranks"], None)


def _with(kind, field, value):
    def make():
        a = _args()
        setattr(a[kind], field, value)
        return a
    return make


_BAD = [
    ("rows", lambda: _args(rows=None)),
    ("rows", _with("rows", "indptr_dev", None)),
    ("rows", _with("rows", "ranks_dev", None)),
    ("rows", _with("rows", "n_rows", -1)),
    ("rows", lambda: _args(specs=None, n_metrics=2)),
    ("rows", lambda: _args(n_metrics=0)),
    ("rows", lambda: _args(n_metrics=-3)),
    ("rows", lambda: _args(specs=[(0, 5)] * 33)),                # more than AAE_METRIC_MAX
    ("rows", lambda: _args(specs=[(6, 5)])),                     # no such kind
    ("rows", lambda: _args(specs=[(-1, 5)])),
    ("rows", lambda: _args(specs=[(0, -1)])),
    ("rows", lambda: _args(specs=[(1, 2 ** 31 - 1)])),           # a cap that is AAE_RANK_ABSENT itself
    ("rows", lambda: _args(specs=[(2, 0)])),                     # unbounded p, ndcg, r-prec, clicks: not defined
    ("rows", lambda: _args(specs=[(3, 0)])),
    ("rows", lambda: _args(specs=[(4, 0)])),
    ("rows", lambda: _args(specs=[(0, 0), (5, 0)])),
    ("rows", lambda: _args(specs=[(3, 21)])),                    # ndcg beyond the table's 20 entries
    ("rows", lambda: _args(specs=[(3, 5)], disc=None)),
    ("rows", lambda: _args(n_disc=-1)),
    ("rows", lambda: _args(per_row=None)),
    ("rows", lambda: _args(ld=4)),                               # ld < n_rows
    ("finish", lambda: _args(vals=None)),
    ("finish", lambda: _args(out=None)),
    ("finish", lambda: _args(fin_n=-1)),
    ("finish", lambda: _args(fin_metrics=0)),
    ("finish", lambda: _args(fin_metrics=33)),
    ("finish", lambda: _args(fin_ld=8)),
    ("lists", lambda: _args(ids=None)),
    ("lists", lambda: _args(k=0)),
    ("lists", lambda: _args(k=-2)),
    ("lists", lambda: _args(ids_ld=9)),                          # ld < k
    ("lists", lambda: _args(truth=None)),
    ("lists", _with("truth", "indptr_dev", None)),
    ("lists", _with("truth", "indices_dev", None)),
    ("lists", _with("truth", "n_rows", -1)),
    ("lists", _with("truth", "row_start", -1)),                  # (without rows_dev the window starts at row_start)
    ("lists", lambda: _args(ranks=None)),
]
_ENTRY = {"rows": "aae_metric_rows", "finish": "aae_metric_finish", "lists": "aae_ranks_from_lists"}


@pytest.mark.parametrize("case", range(len(_BAD)))
def test_invalid_arguments_are_refused_before_the_device(case):
    from aaerec import _hip
    lib = _hip.load_library()
    which, make = _BAD[case]
    assert _call(lib, which, make()) == -1                     # AAE_EINVAL
    msg = lib.aae_last_error().decode()
    assert msg.startswith(_ENTRY[which] + ": ") and len(msg) > len(_ENTRY[which]) + 6, msg


def test_calls_without_rows_launch_nothing():
    from aaerec import _hip
    lib = _hip.load_library()
    a = _args(ld=0)
    a["rows"].n_rows = 0
    assert _call(lib, "rows", a) == 0
    a = _args()
    a["truth"].n_rows = 0
    assert _call(lib, "lists", a) == 0
    a = _args(specs=[(0, 0), (1, 0)], disc=None, n_disc=0, ld=0)                # no ndcg spec: no table needed
    a["rows"].n_rows = 0
    assert _call(lib, "rows", a) == 0


# ---- names ---------------------------------------------------------------------------------------------------------------
def test_metric_spec_round_trips_names_and_refuses_the_rest():
    from aaerec import evaluation as E
    for kind, k in MC.all_specs() + [("ndcg", 2 ** 20 + 1), ("clicks", 3)]:
        name = MC.name_of(kind, k)
        assert E.metric_spec(name) == (kind, k) and E.metric_name(kind, k) == name
        assert E.metric_name(*E.metric_spec(name)) == name
    assert E.metric_spec("P@1") == ("p", 1) and E.metric_spec("P@20") == E.metric_spec("p@20")
    for name in E.METRICS:
        assert E.metric_spec(name)[1] == E.METRICS[name].k
    for bad in ("", "mrr@", "mrr@0", "map@-1", "p", "ndcg", "r-prec", "clicks", "auc@5", "mrr@1.5", "mrr@ 5", "MRR@5", "p@5@5", 5, None):
        with pytest.raises(ValueError):
            E.metric_spec(bad)
    with pytest.raises(ValueError):
        E.metric_name("p")


def test_metrics_keeps_its_keys_and_the_challenge_metrics_are_a_dict_of_their_own():
    from aaerec import evaluation as E
    assert sorted(E.METRICS) == sorted(["mrr@5", "mrr@10", "mrr@20", "map@5", "map@10", "map@20", "p@5", "p@10", "p@20", "P@1", "mrr", "map"])
    assert sorted(E.CHALLENGE_METRICS) == sorted(MC.name_of(kind, k) for kind in ("r-prec", "ndcg", "clicks") for k in (5, 10, 20, 500))
    assert not set(E.CHALLENGE_METRICS) & set(E.METRICS)
    for name, spec in E.CHALLENGE_METRICS.items():
        assert E.metric_spec(name) == spec
    assert E.Evaluation(None, None).metrics is E.METRICS and E.Evaluation(None, None).metrics_on == "host"
    with pytest.raises(ValueError):
        E.Evaluation(None, None, metrics_on="gpu")


# ---- the function evaluate_ranks replaces ----------------------------------------------------------------------------------
def _parent_evaluate_ranks(ranks_csr, metrics):
    """evaluate_ranks as it stood before the new kinds, statement for statement."""
    from aaerec.evaluation import METRICS, MAP, MRR
    R = sp.csr_matrix(ranks_csr)
    n = R.shape[0]
    rows = np.repeat(np.arange(n), np.diff(R.indptr))
    order = np.lexsort((R.data, rows))
    r = np.asarray(R.data)[order].astype(np.float64)
    j = (np.arange(r.size) - np.asarray(R.indptr, dtype=np.int64)[rows] + 1).astype(np.float64)
    has = np.diff(R.indptr) > 0
    first = np.zeros(n, dtype=np.float64)
    first[has] = r[np.asarray(R.indptr[:-1])[has]]
    out = []
    for name in metrics:
        metric = METRICS[name]
        k = metric.k
        inside = np.ones(r.size, dtype=bool) if k is None else r <= k
        if isinstance(metric, MRR):
            ok = has & (first <= k) if k is not None else has
            per_row = np.where(ok, 1.0 / np.where(ok, first, 1.0), 0.0)
        elif isinstance(metric, MAP):
            hits = np.bincount(rows[inside], minlength=n).astype(np.float64)
            total = np.bincount(rows[inside], weights=(j / r)[inside], minlength=n)
            per_row = np.where(hits > 0, total / np.where(hits > 0, hits, 1.0), 0.0)
        else:
            per_row = np.bincount(rows[inside], minlength=n).astype(np.float64) / k
        out.append((per_row.mean(), per_row.std()))
    return out


def _ranks_of(y_true, scores):
    """CSR of the 1-based ranks of the entries of y_true in `scores` (better first, the smaller id at equal scores)."""
    Y = sp.csr_matrix(y_true)
    Y.sort_indices()
    data = np.zeros(Y.nnz, dtype=np.int32)
    ids = np.arange(Y.shape[1])
    for r in range(Y.shape[0]):
        s = scores[r]
        for e in range(Y.indptr[r], Y.indptr[r + 1]):
            t = Y.indices[e]
            data[e] = 1 + np.count_nonzero((s > s[t]) | ((s == s[t]) & (ids < t)))
    return sp.csr_matrix((data, Y.indices.copy(), Y.indptr.copy()), shape=Y.shape)


def test_old_names_are_bit_identical_to_the_function_they_had():
    from aaerec import evaluation as E
    z = np.load(MC.OLD_GOLDEN)
    R = _ranks_of(z["y_true"], z["removed"])
    assert R.nnz > 100
    names = list(E.METRICS)
    got, want = E.evaluate_ranks(R, names), _parent_evaluate_ranks(R, names)
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes()
    got_none = E.evaluate_ranks(R, names, device=None)
    assert np.asarray(got_none).tobytes() == np.asarray(want).tobytes()
    # and per_row=True holds the values those pairs are the mean and std of
    per = E.evaluate_ranks(R, names, per_row=True)
    assert per.shape == (len(names), R.shape[0]) and per.dtype == np.float64
    assert np.asarray([(v.mean(), v.std()) for v in per]).tobytes() == np.asarray(want).tobytes()
    # the fixture's rows as well, with an empty row put in
    _, indptr, ranks = MC.fixture()
    indptr2 = np.concatenate([indptr[:3], indptr[2:]])
    R2 = sp.csr_matrix((ranks, np.zeros(ranks.size, dtype=np.int32), indptr2), shape=(indptr2.size - 1, 700))
    R2.indices = np.concatenate([np.arange(a, dtype=np.int32) for a in np.diff(indptr2)])
    assert np.asarray(E.evaluate_ranks(R2, names)).tobytes() == np.asarray(_parent_evaluate_ranks(R2, names)).tobytes()


# ---- the host forms against the reference's recorded values ------------------------------------------------------------------
def _fixture_csr():
    z, indptr, ranks = MC.fixture()
    return z, sp.csr_matrix((ranks, z["indices"], indptr), shape=(indptr.size - 1, int(z["n_items"])))


def test_the_fixture_is_what_the_issue_describes():
    z, indptr, ranks = MC.fixture()
    lengths = np.diff(indptr)
    assert int(z["n_items"]) == 700 and z["ks"].tolist() == [1, 10, 64, 65, 500]
    assert lengths.min() == 1 and lengths.max() == 200 and {1, 2, 3, 63, 64, 65, 200} <= set(lengths.tolist())
    assert z["rankings"].shape == (lengths.size, 700) and (np.sort(z["rankings"], axis=1) == np.arange(700)).all()
    assert ranks.min() >= 1 and ranks.max() <= 700
    for kind in ("r-prec", "ndcg", "clicks"):
        assert z[kind].shape == (5, lengths.size)
    assert (z["r-prec"] > 0).any() and (z["ndcg"][1] > 0).any() and (z["clicks"][4] < 51).any() and (z["clicks"][0] == 1.1).any()
    assert sorted(z["metric_names"].tolist()) == sorted(["mrr@5", "mrr@10", "mrr@20", "map@5", "map@10", "map@20", "p@5", "p@10",
                                                        "p@20", "P@1", "mrr", "map"])


def test_host_forms_equal_the_references_values():
    from aaerec import evaluation as E
    z, R = _fixture_csr()
    cases = MC.fixture_names()
    names = [c[0] for c in cases]
    got = E.evaluate_ranks(R, names, per_row=True)
    for (name, want, kind, k), row in zip(cases, got):
        MC.check_against_fixture(row, want, kind, k, R.indptr, R.data)
    pairs = E.evaluate_ranks(R, names)
    for (m, s), row in zip(pairs, got):
        assert m == row.mean() and s == row.std()


def test_host_forms_equal_the_exact_definition_on_the_device_rows():
    from aaerec import evaluation as E
    indptr, ranks = MC.device_rows()
    R = sp.csr_matrix((ranks, np.concatenate([np.arange(a, dtype=np.int32) for a in np.diff(indptr)]), indptr),
                      shape=(indptr.size - 1, ROW_ITEMS))
    specs = MC.all_specs()
    got = E.evaluate_ranks(R, [MC.name_of(kind, k) for kind, k in specs], per_row=True)
    want = MC.device_rows_exact()
    for (kind, k), row in zip(specs, got):
        for i, (v, (w, t)) in enumerate(zip(row, want[(kind, k)])):
            MC.check_value(v, w, t, kind, (kind, k, i))


ROW_ITEMS = 5000


# ---- lists against ranks ---------------------------------------------------------------------------------------------------
def test_evaluate_topk_from_lists_equals_evaluate_ranks_from_the_full_ranks():
    from aaerec import evaluation as E
    z, R = _fixture_csr()
    n = R.shape[0]
    truth = sp.csr_matrix((np.ones(R.nnz), R.indices, R.indptr), shape=R.shape)
    bounded = [c for c in MC.fixture_names() if c[3] is not None]
    for K in (20, 500, 700):
        ids = z["rankings"][:, :K].copy()
        names = [c[0] for c in bounded if c[3] <= K]
        assert len(names) >= 10
        per_lists = E.evaluate_topk(truth, ids, names, per_row=True)
        per_ranks = E.evaluate_ranks(R, names, per_row=True)
        np.testing.assert_array_equal(per_lists, per_ranks)
        new = [nm for nm in names if nm not in E.METRICS]
        assert np.asarray(E.evaluate_topk(truth, ids, new)).tobytes() == np.asarray(E.evaluate_ranks(R, new)).tobytes()
        # the names of METRICS keep the relevance-matrix form they had (rank_metrics_with_std): the same values within the
        # bounds of tests/metric_cases.py - a row's value within 2 (t + 2) u, t <= 20, the mean of n of them (n + 1) u more
        old = [nm for nm in names if nm in E.METRICS]
        rel = (2 * 22 + n + 1) * MC.U
        for (m1, s1), (m2, s2), row in zip(E.evaluate_topk(truth, ids, old), E.evaluate_ranks(R, old), E.evaluate_ranks(R, old, per_row=True)):
            assert abs(m1 - m2) <= 2 * rel * abs(m2)
            assert abs(s1 * s1 - s2 * s2) <= 2 * ((n + 8) * 2.0 ** -52 + 4 * 2 * 22 * MC.U) * float(row.max()) ** 2
    for name in ("mrr", "map", "ndcg@21", "clicks@500"):
        with pytest.raises(ValueError):
            E.evaluate_topk(truth, z["rankings"][:, :20], [name])


def test_host_ranks_from_lists_equals_the_restatement():
    from aaerec import evaluation as E
    for K in MC.LIST_KS:
        ids, indptr, indices = MC.list_case(K)
        gt = sp.csr_matrix((np.ones(indices.size), indices, indptr), shape=(indptr.size - 1, 3000))
        got = E._host_ranks_from_lists(gt, ids)
        np.testing.assert_array_equal(got.data, MC.want_ranks_from_lists(ids, indptr, indices))
        assert got.dtype == np.int32 and (got.data == MC.ABSENT).any() and (got.data != MC.ABSENT).any()


# ---- the guards of the device route ----------------------------------------------------------------------------------------
def _long_row_case(m):
    r = np.random.RandomState(m)
    lengths = [3, m, 0, 2]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ranks = np.concatenate([r.permutation(6000)[:a] + 1 for a in lengths]).astype(np.int32)
    cols = np.concatenate([np.arange(a, dtype=np.int32) for a in lengths])
    return sp.csr_matrix((ranks, cols, indptr), shape=(4, 6000))


def test_the_wrapper_sends_an_over_long_row_to_the_host_route(monkeypatch):
    import torch
    from aaerec import _hip, evaluation as E, ranking
    called = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)      # (a device is "present": only the guards are looked at)
    monkeypatch.setattr(_hip, "rank_metrics", lambda indptr, ranks, specs, **kw: called.append(1) or np.zeros((len(specs), 2)))
    monkeypatch.setattr(_hip, "upload", lambda x, *a, **kw: x)
    names = ["map", "ndcg@10", "r-prec@500", "clicks@5", "mrr@20"]
    R = _long_row_case(MC.ROW_MAX + 1)
    assert not E.device_metrics_ok(np.diff(R.indptr), E._specs(names), "cuda:0")
    got = E.evaluate_ranks(R, names, device="cuda:0")
    assert not called
    assert np.asarray(got).tobytes() == np.asarray(E.evaluate_ranks(R, names)).tobytes()
    d = MC.table(500)
    per = E.evaluate_ranks(R, names, device="cuda:0", per_row=True)
    for name, row in zip(names, per):
        kind, k = E.metric_spec(name)
        w, t = MC.exact(kind, k, R.data[R.indptr[1]:R.indptr[2]], d)
        MC.check_value(row[1], w, t, kind, name)
    # a row of exactly AAE_METRIC_ROW_MAX entries is the device's; an ndcg cap beyond 2^20 and no device are not
    ok = _long_row_case(MC.ROW_MAX)
    assert E.device_metrics_ok(np.diff(ok.indptr), E._specs(names), "cuda:0")
    E.evaluate_ranks(ok, names, device="cuda:0")
    assert called == [1]
    assert E.device_metrics_ok(np.diff(ok.indptr), [("ndcg", 2 ** 20)], "cuda:0")
    assert not E.device_metrics_ok(np.diff(ok.indptr), [("ndcg", 2 ** 20 + 1)], "cuda:0")
    assert E.device_metrics_ok(np.diff(ok.indptr), [("map", 2 ** 20 + 1), ("mrr", None)], "cuda:0")
    assert not E.device_metrics_ok(np.diff(ok.indptr), E._specs(names), None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert not E.device_metrics_ok(np.diff(ok.indptr), E._specs(names), "cuda:0")
    # ndcg beyond 2^20 on the host: the same definition (the table only reaches as far as the ranks do)
    big = E.evaluate_ranks(ok, ["ndcg@{}".format(2 ** 20 + 1), "ndcg@6000"], device="cuda:0", per_row=True)
    np.testing.assert_array_equal(big[0], big[1])
    assert called == [1] and ranking.rank_metrics is not None


def test_a_rank_below_one_raises_on_both_routes(monkeypatch):
    import torch
    from aaerec import evaluation as E
    R = _long_row_case(5)
    R.data[4] = 0
    with pytest.raises(ValueError):
        E.evaluate_ranks(R, ["mrr"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(ValueError):
        E.evaluate_ranks(R, ["mrr"], device="cuda:0")
    R.data[4] = -3
    with pytest.raises(ValueError):
        E.evaluate_ranks(R, ["clicks@5"])


# ---- recommenders and Evaluation on the host route ---------------------------------------------------------------------------
def test_host_routes_of_a_recommender_answer_metrics_and_evaluation_asks_for_them():
    import popular_cases as PC
    from aaerec import evaluation as E
    from aaerec.popular import MostPopular
    counts = PC.counts_300()
    T, Y = PC.test_rows(counts)
    rec = MostPopular(device=None)
    rec.train(PC.Rows(PC.training_set(counts)))
    names = ["mrr", "map@10", "ndcg@10", "r-prec@65", "clicks@65", "p@5"]
    ranks = rec.predict_ranks(PC.Rows(T), Y)
    assert np.asarray(rec.predict_ranks(PC.Rows(T), Y, metrics=names)).tobytes() == np.asarray(E.evaluate_ranks(ranks, names)).tobytes()
    bounded = names[1:]
    ids, _ = rec.predict_topk(PC.Rows(T), k=65)
    got = rec.predict_topk(PC.Rows(T), k=65, y_true=Y, metrics=bounded)
    assert np.asarray(got).tobytes() == np.asarray(E.evaluate_topk(Y, ids, bounded)).tobytes()
    with pytest.raises(ValueError):
        rec.predict_topk(PC.Rows(T), k=65, metrics=bounded)                   # no ground truth
    with pytest.raises(ValueError):
        rec.predict_topk(PC.Rows(T), k=65, y_true=Y, metrics=["mrr"])         # unbounded from lists
    for metrics, method in ((["mrr@5", "ndcg@5", "clicks@5"], "predict_topk"), (["mrr", "r-prec@5"], "predict_ranks")):
        on_host, on_dev = MostPopular(device=None), MostPopular(device=None)
        asked = PC.counting(on_dev)
        ev = PC.evaluation_setup(metrics, topk=True)
        want = ev([on_host])[0]
        ev.metrics_on = "device"
        got = ev([on_dev])[0]
        assert asked == [method]
        assert np.asarray(got, dtype=np.float64).tobytes() == np.asarray(want, dtype=np.float64).tobytes()
