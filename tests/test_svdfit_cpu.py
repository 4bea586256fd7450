"""SVDRecommender(fit=...) without a device: the emulation that pins the algorithm equals scikit-learn's fit, the default is the
host fit as it was, and every case the device fit hands back to the host warns and gives exactly the host fit."""
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import svdfit_cases as S
from aaerec.lowrank import SVDRecommender


@pytest.mark.parametrize("name", list(S.BAG_CASES))
def test_float64_emulation_is_sklearn(name):
    c = S.case(name)
    V, s = c["emu64"]
    assert np.abs(s - c["sk"].singular_values_).max() == 0.0
    assert np.abs(V - c["sk"].components_).max() == 0.0


@pytest.mark.parametrize("name", S.CASES)
def test_float32_emulation_is_a_fit_in_fp32(name):
    """d32 is the size of fp32 rounding, not of a different algorithm: far below the gap to the exact optimum."""
    c = S.case(name)
    assert 0 < c["d32"]["sigma"] < 2e-6 and 0 < c["d32"]["orth"] < 2e-5 and c["d32"]["resid"] < 2e-6
    assert c["sk_resid"] >= c["optimum"]


def _host(A, dims, seed, **kw):
    return SVDRecommender(dims, device=None, random_state=seed, **kw).fit(A).svd.components_


def test_default_is_the_host_fit_and_bad_arguments_raise():
    c = S.case("wide_300x500")
    rec = SVDRecommender(c["dims"], device=None, random_state=c["seed"])
    assert rec.fit_on == "host"
    rec.fit(c["A"])
    assert rec.fitted_on == "host"
    assert np.array_equal(rec.svd.components_, c["sk"].components_)
    with pytest.raises(ValueError):
        SVDRecommender(8, fit="device", device=None)
    with pytest.raises(ValueError):
        SVDRecommender(8, fit="gpu")


def _not_finite_in_fp32(A):
    A = A.copy()
    A.data[5] = 1e39          # finite in float64, infinite as fp32
    return A


@pytest.mark.parametrize("why, kw, change", [
    ("dims + n_oversamples", dict(n_oversamples=4090), None),
    ("arpack", dict(algorithm="arpack"), None),
    ("not finite", dict(), _not_finite_in_fp32),
    ("fit_bytes", dict(fit_bytes=1024), None),
])
def test_fallbacks_warn_and_give_the_host_fit(why, kw, change):
    c = S.case("wide_300x500")
    A = change(c["A"]) if change else c["A"]
    dims = 8
    rec = SVDRecommender(dims, fit="device", device="cuda:0", random_state=c["seed"], **kw)
    with pytest.warns(UserWarning, match=re.escape(why)) as seen:
        rec.fit(A)
    assert sum("fitting on the host" in str(w.message) for w in seen) == 1
    assert rec.fitted_on == "host"
    host_kw = {k: v for k, v in kw.items() if k != "fit_bytes"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = _host(A, dims, c["seed"], **host_kw)
    assert np.array_equal(rec.svd.components_, want)


def test_more_components_than_features_raises_as_sklearn_does():
    A = sp.csr_matrix(np.eye(6))
    with pytest.raises(ValueError, match="n_components"):
        SVDRecommender(7, fit="device", device="cuda:0").fit(A)
