"""The rank-based metrics on the device (csrc/rank_metrics.h through aaerec._hip, aaerec.evaluation, aaerec.ranking): per-row
values against exact arithmetic over the same ranks and the same table doubles, the guard of over-long rows, the (mean, std)
reduction, lists to ranks, the reference's recorded values, and Evaluation(metrics_on="device") against "host".  Definitions,
cases and every bound: tests/metric_cases.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import metric_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _codes(specs):
    return [(MC.KIND_CODE[kind], 0 if k is None else k) for kind, k in specs]


def _per_row(indptr, ranks, specs):
    from aaerec import _hip
    return _hip.rank_metrics(_hip.upload(np.array(indptr), DEV), _hip.upload(np.array(ranks), DEV), _codes(specs), per_row=True)


def _check_rows(got, specs, want, rows=None, what=""):
    assert got.shape[0] == len(specs) and got.dtype == np.float64
    for (kind, k), vals in zip(specs, got):
        for i in (range(vals.size) if rows is None else rows):
            w, t = want[(kind, k)][i]
            print(what, MC.name_of(kind, k), "row", i, "got", repr(float(vals[i])), "exact", float(w), "t", t)
            MC.check_value(vals[i], w, t, kind, (what, kind, k, i))


@pytest.fixture(scope="module")
def full_call():
    """The one call with all 32 specs over the rows of MC.device_rows(), and its exact counterpart."""
    indptr, ranks = MC.device_rows()
    assert np.diff(indptr)[:len(MC.LENGTHS)].tolist() == list(MC.LENGTHS) and ranks.max() == MC.ABSENT
    assert np.sort(ranks[ranks != MC.ABSENT])[-1] == 2 ** 31 - 2
    specs = MC.specs_32()
    assert len(specs) == 32 and {k for _, k in specs} == set(MC.KS) | {None} and {kind for kind, _ in specs} == set(MC.KINDS)
    got = _per_row(indptr, ranks, specs)
    got.setflags(write=False)
    return indptr, ranks, specs, got, MC.device_rows_exact()


def test_all_32_specs_in_one_call_equal_the_exact_definition(full_call):
    indptr, ranks, specs, got, want = full_call
    assert got.shape == (32, indptr.size - 1) and np.isfinite(got).all()
    _check_rows(got, specs, want, what="32")


def test_every_spec_alone_equals_the_exact_definition_and_the_full_call(full_call):
    indptr, ranks, specs, full, want = full_call
    for spec in MC.all_specs():                                    # (every kind at every cap of MC.KS, and the unbounded two)
        got = _per_row(indptr, ranks, [spec])
        _check_rows(got, [spec], want, what="single")
        if spec in specs:
            assert got[0].tobytes() == full[specs.index(spec)].tobytes(), spec


def test_a_second_run_returns_the_same_bits(full_call):
    indptr, ranks, specs, got, _ = full_call
    assert _per_row(indptr, ranks, specs).tobytes() == got.tobytes()


def test_more_than_32_names_go_in_parts_and_the_pairs_are_the_mean_and_std_of_the_rows(full_call):
    from aaerec import _hip
    indptr, ranks, _, _, want = full_call
    specs = MC.all_specs()
    d_indptr, d_ranks = _hip.upload(np.array(indptr), DEV), _hip.upload(np.array(ranks), DEV)
    per = _hip.rank_metrics(d_indptr, d_ranks, _codes(specs), per_row=True)
    _check_rows(per, specs, want, rows=(0, 3, 9, 11), what="44")
    pairs = _hip.rank_metrics(d_indptr, d_ranks, _codes(specs))
    assert pairs.shape == (44, 2)
    for (mean, std), vals in zip(pairs, per):
        MC.check_mean_std(mean, std, vals)


def test_a_row_beyond_the_cap_is_nan_and_its_neighbours_stand():
    """A row of 4097 entries through the library call itself (the Python guards are not in the way): the length is compared with
    the cap before LDS is indexed, the row's values are NaN, every other row's are right."""
    r = np.random.RandomState(7)
    lengths = [10, MC.ROW_MAX + 1, 70, 0, 300, 5000, 1]
    rows = [r.choice(6000, size=m, replace=False).astype(np.int32) + 1 for m in lengths]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    specs = [("map", None), ("ndcg", 500), ("r-prec", 64), ("clicks", 10), ("mrr", 5), ("p", 1024)]
    got = _per_row(indptr, np.concatenate(rows), specs)
    d = MC.table(500)
    assert np.isnan(got[:, [1, 5]]).all()
    for q, (kind, k) in enumerate(specs):
        for i in (0, 2, 3, 4, 6):
            w, t = MC.exact(kind, k, rows[i], d)
            MC.check_value(got[q, i], w, t, kind, (kind, k, i))


def test_a_rank_below_one_is_nan_through_the_library_and_a_value_error_through_the_package():
    from aaerec import evaluation as E
    indptr = np.array([0, 2, 5, 105], dtype=np.int64)
    ranks = np.concatenate([[3, 1], [4, 0, 9], np.arange(100, 0, -1)]).astype(np.int32)
    ranks[50] = -7
    got = _per_row(indptr, ranks, [("mrr", None), ("clicks", 10)])
    assert np.isnan(got[:, 1:]).all() and got[0, 0] == 1.0 and got[1, 0] == 0.0
    R = sp.csr_matrix((ranks, np.concatenate([np.arange(2), np.arange(3), np.arange(100)]).astype(np.int32), indptr), shape=(3, 100))
    with pytest.raises(ValueError):
        E.evaluate_ranks(R, ["mrr"], device=DEV)


@pytest.mark.parametrize("n", MC.FINISH_SIZES)
def test_finish_gives_the_mean_and_population_std_of_given_doubles(n):
    from aaerec import _hip
    x = np.stack([MC.finish_values(n, seed) for seed in range(3)] + [np.full(n, 0.3)])
    vals = torch.as_tensor(x).to(DEV)
    out = torch.full((x.shape[0], 2), -1.0, dtype=torch.float64, device=DEV)
    _hip._check(_hip.load_library().aae_metric_finish(_hip._ptr(vals), int(vals.stride(0)), n, x.shape[0], _hip._ptr(out),
                                                      _hip._stream_of(vals.device)))
    got = out.cpu().numpy()
    for (mean, std), row in zip(got, x):
        print("n", n, "mean", repr(float(mean)), "std", repr(float(std)), "numpy", repr(float(row.mean())), repr(float(row.std())))
        MC.check_mean_std(mean, std, row)
    out2 = torch.empty_like(out)
    _hip._check(_hip.load_library().aae_metric_finish(_hip._ptr(vals), int(vals.stride(0)), n, x.shape[0], _hip._ptr(out2),
                                                      _hip._stream_of(vals.device)))
    assert out2.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize("K", MC.LIST_KS)
def test_ranks_from_lists_equal_the_restatement(K):
    from aaerec import _hip
    ids, indptr, indices = MC.list_case(K)
    n = indptr.size - 1
    want = MC.want_ranks_from_lists(ids, indptr, indices)
    assert (ids == -1).any() and (np.diff(indptr) == 0).sum() == 2 and (want == MC.ABSENT).any() and (want != MC.ABSENT).any()
    truth = _hip.DeviceCSR.from_arrays(indptr, indices, np.ones(indices.size, dtype=np.float32), 3000, DEV)
    d_ids = _hip.upload(ids, DEV)
    got = _hip.ranks_from_lists(d_ids, truth, 0, n, indices.size)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # a window of rows, and a shorter list out of the same matrix (its row stride stays K)
    lo, hi = 3, 8
    part = _hip.ranks_from_lists(d_ids[lo:hi], truth, lo, hi - lo, int(indptr[hi] - indptr[lo]))
    np.testing.assert_array_equal(part.cpu().numpy(), want[indptr[lo]:indptr[hi]])
    if K > 1:
        short = _hip.ranks_from_lists(d_ids, truth, 0, n, indices.size, k=K // 2)
        np.testing.assert_array_equal(short.cpu().numpy(), MC.want_ranks_from_lists(ids[:, :K // 2], indptr, indices))


# ---- the reference's recorded values -----------------------------------------------------------------------------------------
def test_device_values_equal_the_references_from_ranks_and_from_lists():
    from aaerec import evaluation as E
    z, indptr, ranks = MC.fixture()
    R = sp.csr_matrix((ranks, z["indices"], indptr), shape=(indptr.size - 1, int(z["n_items"])))
    cases = MC.fixture_names()
    names = [c[0] for c in cases]
    got = E.evaluate_ranks(R, names, device=DEV, per_row=True)
    for (name, want, kind, k), row in zip(cases, got):
        MC.check_against_fixture(row, want, kind, k, indptr, ranks)
    truth = sp.csr_matrix((np.ones(R.nnz), R.indices, R.indptr), shape=R.shape)
    bounded = [c for c in cases if c[3] is not None]
    from_lists = E.evaluate_topk(truth, z["rankings"][:, :500], [c[0] for c in bounded], device=DEV, per_row=True)
    for (name, want, kind, k), row in zip(bounded, from_lists):
        MC.check_against_fixture(row, want, kind, k, indptr, ranks)
    # (mean, std) of the same call: the device's pairs against the exact mean and variance of the device's own rows
    for (mean, std), row in zip(E.evaluate_ranks(R, names, device=DEV), got):
        MC.check_mean_std(mean, std, row)
    with pytest.raises(ValueError):
        E.evaluate_topk(truth, z["rankings"][:, :500], ["mrr"], device=DEV)


# ---- Evaluation: metrics_on="device" against "host" --------------------------------------------------------------------------
N_ITEMS, N_PROTO, N_DOCS = 1000, 100, 2000          # the sizes of config C1 (tools/gen_golden.py gen_e2e_c1)


@pytest.fixture(scope="module")
def c1_bags():
    from aaerec.datasets import Bags
    rng = np.random.RandomState(42)
    protos = [rng.choice(N_ITEMS, size=10, replace=False) for _ in range(N_PROTO)]
    data, owners, years = [], [], {}
    for i in range(N_DOCS):
        p = protos[rng.randint(N_PROTO)]
        data.append(["i%d" % t for t in rng.choice(p, size=rng.randint(6, 10), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // N_DOCS
    return Bags(data, owners, {"year": years})


def _recommender(kind):
    if kind == "popular":
        from aaerec.popular import MostPopular
        return MostPopular(device=DEV)
    from aaerec.aae import AAERecommender
    return AAERecommender(n_hidden=50, n_code=50, n_epochs=3, batch_size=100, gen_lr=0.01, verbose=False, seed=11)


TOPK_NAMES = ["mrr@10", "map@10", "p@5", "P@1", "ndcg@10", "r-prec@10", "clicks@10", "clicks@500", "ndcg@500"]
RANK_NAMES = ["mrr", "map", "mrr@10", "ndcg@500", "r-prec@20", "clicks@500", "p@20"]


@pytest.mark.parametrize("kind", ["popular", "aae"])
@pytest.mark.parametrize("names,method", [(TOPK_NAMES, "predict_topk"), (RANK_NAMES, "predict_ranks")])
def test_evaluation_with_metrics_on_the_device_gives_the_hosts_numbers(c1_bags, kind, names, method):
    """One trained recommender under Evaluation(metrics_on="host") and under "device": the same lists / ranks both times, so the
    numbers differ by rounding alone.  A row holds one held-out item (drop=1): a per-row value sums t <= 2 terms on either side,
    2 (t + 2) u apart at most; the mean of n of them (n + 1) u more on either side; the std through its variance, whose bound
    (MC.check_mean_std) holds on either side, over values of at most 1 - clicks@k: k / 10 + 1."""
    from aaerec.evaluation import Evaluation
    np.random.seed(3)
    torch.manual_seed(3)
    ev = Evaluation(c1_bags, 2009, metrics=names, logfile=None, topk=True).setup(min_elements=2, drop=1)
    n = ev.y_test.shape[0]
    # (C1's generator: 100 prototypes of 10 out of 1000 items reach some 650 distinct items)
    assert 600 < ev.train_set.size(1) <= N_ITEMS and n >= 150 and ev.y_test.nnz == n
    rec = _recommender(kind)
    asked = []
    real = getattr(rec, method)
    setattr(rec, method, lambda *a, **kw: asked.append(kw.get("metrics")) or real(*a, **kw))
    host = ev([rec])[0]
    rec.train = lambda training_set: None                     # (the same trained model answers the second run)
    ev.metrics_on = "device"
    dev = ev([rec])[0]
    assert asked == [None, names]
    row_eps = 2 * (2 + 2) * MC.U
    for name, (m_h, s_h), (m_d, s_d) in zip(names, host, dev):
        top = float(name.split("@")[1]) / 10 + 1 if name.startswith("clicks") else 1.0
        print(kind, name, "host", repr(float(m_h)), repr(float(s_h)), "device", repr(float(m_d)), repr(float(s_d)))
        assert abs(m_d - m_h) <= (row_eps + 2 * (n + 1) * MC.U) * abs(m_h), name
        assert abs(s_d * s_d - s_h * s_h) <= 2 * ((n + 8) * 2.0 ** -52 + 4 * row_eps) * top * top, name
    assert all(np.isfinite(v) for pair in dev for v in pair) and dev[0][0] > 0
