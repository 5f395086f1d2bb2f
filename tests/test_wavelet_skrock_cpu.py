"""CPU: the SK-ROCK coefficient table (tests/wavelet_skrock_restatement.py and the library's host functions
sbtv_skrock_coefficients / sbtv_skrock_max_step) and the restated chain of tests/wavelet_skrock_cases.py.

On the scalar linear drift D(v) = -a v one step is X_new = A X + Bq (q Z) with A = T_s(w0 - w1 a delta) / T_s(w0) (the
stability polynomial); A and Bq are read off the restated step with (X, Z) = (1, 0) and (0, 1 / q)."""
import math

import numpy as np
import pytest

import wavelet_posterior_cases as wpc
import wavelet_skrock_cases as wkc
import wavelet_skrock_restatement as wkr

STAGES = (2, 3, 5, 10, 15)
ETA = 0.05


def _cheb_T(s, x):
    return wkr.chebyshev(s, x)[0][s]


def _responses(c, adelta):
    """(A, Bq) of one step on D(v) = -a v at delta = 1, a = adelta: X_new = A X + Bq q Z."""
    drift = lambda v: -adelta * v
    q = math.sqrt(2.0)
    return wkr.step(1.0, 0.0, drift, c, 1.0), wkr.step(0.0, 1.0 / q, drift, c, 1.0)


@pytest.mark.parametrize("s", STAGES)
def test_table_identities(s):
    c = wkr.coefficients(s, ETA)
    T = c["T"]
    # nu_j + kappa_j = 1 and kappa_j = -T_{j-2} / T_j, j >= 2
    np.testing.assert_allclose(c["nu"][1:] + c["kappa"][1:], 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(c["kappa"][1:], -T[:-2] / T[2:], rtol=1e-12, atol=0)
    # the stability polynomial, and |A| < 1 on (0, l_s]
    for ad in np.linspace(1e-6, 1.0, 41) * c["ls"]:
        A, _ = _responses(c, float(ad))
        want = _cheb_T(s, c["omega0"] - c["omega1"] * float(ad)) / T[s]
        assert abs(A - want) <= 1e-12, (s, ad, A, want)
        assert abs(A) < 1.0, (s, ad, A)
    # the stationary variance of a dX = -a X dt + sqrt 2 dW is 1 / a: 2 delta Bq^2 / (1 - A^2) a -> 1 as a delta -> 0
    ad = 1e-3 * c["ls"]
    A, Bq = _responses(c, ad)
    ratio = 2.0 * Bq * Bq / (1.0 - A * A) * ad
    assert abs(ratio - 1.0) <= 0.01, (s, ratio)


@pytest.mark.parametrize("s", STAGES)
def test_library_table_is_the_restatement(s):
    """Host functions of the library: no GPU."""
    import sbtv
    got, want = sbtv.skrock_coefficients(s, ETA), wkr.coefficients(s, ETA)
    for k in ("mu", "nu", "kappa"):
        assert got[k].shape == (s,)
        np.testing.assert_allclose(got[k], want[k], rtol=1e-14, atol=0, err_msg=k)
    for k in ("omega0", "omega1", "ls"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-14, atol=0, err_msg=k)
    for s2, lam, nB2 in ((0.37, 1.85, 1.0), (2.5, 0.5, 0.8), (1e-2, 5e-2, 0.0)):
        np.testing.assert_allclose(sbtv.skrock_max_step(s, ETA, s2, lam, nB2), want["ls"] / (nB2 / s2 + 1.0 / lam), rtol=1e-14)
    assert sbtv.skrock_max_step(s, ETA, 0.37, 1.85) == sbtv.skrock_max_step(s, ETA, 0.37, 1.85, 1.0) == wkr.max_step(s, ETA, 0.37, 1.85)


def test_library_table_refusals():
    import sbtv
    for s, eta in ((1, ETA), (0, ETA), (3, 0.0), (3, -1.0), (3, float("nan")), (3, float("inf"))):
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.skrock_coefficients(s, eta)
        assert e.value.code == -1, (s, eta)
    for args in ((1, ETA, 1.0, 1.0), (3, 0.0, 1.0, 1.0), (3, ETA, 0.0, 1.0), (3, ETA, 1.0, 0.0), (3, ETA, float("nan"), 1.0),
                 (3, ETA, 1.0, float("inf")), (3, ETA, 1.0, 1.0, -1.0), (3, ETA, 1.0, 1.0, float("nan"))):
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.skrock_max_step(*args)
        assert e.value.code == -1, args


@pytest.mark.parametrize("name", ["a", "c", "d"])
@pytest.mark.parametrize("s", [2, 3, 10])
def test_restated_chain_stays_finite_at_the_steps_of_the_gpu_tests(name, s):
    r = wkc.chain(name, 0, s, 6, wkc.noise(name, 6)[:, 0])
    assert r["samples"].shape[0] == 6
    assert np.all(np.isfinite(r["samples"])) and np.all(np.isfinite(r["gx"])) and np.all(np.isfinite(r["logpi"]))
    peak = float(np.max(np.abs(r["samples"])))
    print(f"case {name} s = {s}: max|X| = {peak:.4g}, gx = {r['gx'][0]:.6g} .. {r['gx'][-1]:.6g}")
    assert peak < 1e4                                                      # the data are 0..255 images


def test_cases_use_four_fifths_of_the_stability_bound():
    p = wpc.problem("b")
    op = wkc.options("b", 3, 4)
    want = 0.8 * wkr.coefficients(3, ETA)["ls"] / (1.0 / float(min(p["sigma2"])) + 1.0 / op["lambda"])
    assert op["delta"] == pytest.approx(want, rel=1e-15)
