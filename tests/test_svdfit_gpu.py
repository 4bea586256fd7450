"""SVDRecommender(fit="device") against scikit-learn's float64 fit with the same random_state (tests/svdfit_cases.py).

Per case and quantity the device may deviate by at most 8 * d32, d32 the deviation of the float32 host emulation of the same
algorithm.  Each test prints d32 and the device's figure before it asserts (DESIGN 3.4e records them)."""
import numpy as np
import pytest

import svdfit_cases as S
from lowrank_cases import Titled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_FITS = {}


def _fit(name):
    """The device fit of a case, run once: (recommender, components_ of a second fit with the same random_state)."""
    if name not in _FITS:
        from aaerec.lowrank import SVDRecommender
        c = S.case(name)
        recs = []
        for _ in range(2):
            rec = SVDRecommender(c["dims"], use_title=c["titles"] is not None, fit="device", device=DEV, random_state=c["seed"])
            rec.train(Titled(c["X"], c["titles"]))
            assert rec.fitted_on == "device" and not rec.qr_on_host
            recs.append(rec)
        _FITS[name] = recs[0], recs[1].svd.components_
    return _FITS[name]


@pytest.mark.parametrize("name", S.CASES)
def test_device_fit_within_8_d32_of_sklearn(name):
    c = S.case(name)
    rec, _ = _fit(name)
    svd = rec.svd
    assert svd.components_.shape == c["sk"].components_.shape and svd.components_.dtype == np.float64
    assert svd.n_features_in_ == c["A"].shape[1]
    got, resid = S.deviations(c, svd.components_, svd.singular_values_)
    for q in ("sigma", "resid", "orth"):
        print("{} {}: d32 {:.3e}  device {:.3e}  bound {:.3e}".format(name, q, c["d32"][q], got[q], c["bound"][q]))
    print("{} residual: device {!r} sklearn {!r} optimum {!r}".format(name, resid, c["sk_resid"], c["optimum"]))
    for q in ("sigma", "resid", "orth"):
        assert got[q] <= c["bound"][q], (q, got[q], c["bound"][q])
    assert resid >= c["optimum"] - c["bound"]["resid"] * c["sk_resid"]         # no rank-dims V goes below the optimum
    # what TruncatedSVD.fit leaves beside the components (fp32 products: a loose look, the three quantities above judge the fit)
    np.testing.assert_allclose(svd.explained_variance_, c["sk"].explained_variance_, rtol=1e-3, atol=1e-6 * c["sk"].explained_variance_[0])
    np.testing.assert_allclose(svd.explained_variance_ratio_.sum(), c["sk"].explained_variance_ratio_.sum(), rtol=1e-4)


@pytest.mark.parametrize("name", S.CASES)
def test_same_random_state_same_bits(name):
    rec, again = _fit(name)
    assert np.array_equal(rec.svd.components_.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize("name", ["wide_300x500", S.TITLE_CASE])
def test_fitted_model_serves_every_route(name):
    """transform / inverse_transform / predict_topk / predict_ranks after fit="device": the shapes fit="host" returns."""
    from aaerec.lowrank import SVDRecommender
    c = S.case(name)
    rec, _ = _fit(name)
    host = SVDRecommender(c["dims"], use_title=c["titles"] is not None, device=DEV, random_state=c["seed"])
    bags = Titled(c["X"], c["titles"])
    host.train(bags)
    test = Titled(c["X"][:50], None if c["titles"] is None else c["titles"][:50])
    F = rec._features(test)
    assert rec.transform(F).shape == host.transform(F).shape == (50, c["dims"])
    assert rec.inverse_transform(rec.transform(F)).shape == host.inverse_transform(host.transform(F)).shape
    assert rec.predict(test).shape == host.predict(test).shape
    assert str(rec) == str(host) and rec.on_device(10)
    ids, val = rec.predict_topk(test, 10)
    hids, hval = host.predict_topk(test, 10)
    assert ids.shape == hids.shape == (50, 10) and val.shape == hval.shape and ids.dtype == hids.dtype
    Y = c["X"][50:100]
    ranks, hranks = rec.predict_ranks(test, Y), host.predict_ranks(test, Y)
    assert ranks.shape == hranks.shape and np.array_equal(ranks.indptr, hranks.indptr) and ranks.nnz == hranks.nnz
    assert ranks.data.min() >= 1
