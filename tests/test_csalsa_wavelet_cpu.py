"""CPU: the two NumPy restatements of C-SALSA with the wavelet analysis prior (tests/csalsa_wavelet_restatement.py) on the cases of
tests/csalsa_wavelet_cases.py, and what the GPU tests rely on.

- The literal CSALSA_v2 iteration with identity P / PT, the TV prox as psi and phi = TVnorm is sbtv_oracle.CSALSA_v2 bit for bit.
- Every case stops where its table entry says.  Where the rule fires inside the loop, its value is at least 1 % away from tolA
  and criterion / epsilon at least 1e-3 away from 1 at the stopping iteration and at the one before; at no earlier iteration are
  both conditions of the stop within those margins of holding; and ||ve|| / epsilon is at least 1e-3 away from 1 at every
  iteration of every case, so no rounding within the bars below can move a stop or flip the projection.
- The literal iteration and the state form the library runs stop at the same iteration and agree within the bars of the GPU test
  (objective rtol 1e-9, criterion 1e-8, distance1 rtol 1e-6 with atol 1e-9, distance2 and mses 1e-9, max|x - ref| < 1e-7).
  Measured here, worst over the ten cases: objective 6.7e-16, criterion 2.2e-14, distance1 1.6e-13, distance2 2.1e-14,
  mses 1.1e-14 (all relative), max|dx| 1.3e-12.
- The x returned by a case that stops inside the loop is feasible: ||B x - y|| <= epsilon, recomputed from x alone."""
import os
import re

import numpy as np
import pytest

import csalsa_wavelet_cases as cc
import csalsa_wavelet_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_literal_restatement_with_identity_handles_and_the_tv_prox_is_the_oracle_bit_for_bit():
    import sbtv_oracle as o
    import wavelet_cases as wc
    x = wc.synth_image(32, 32, 4)                             # square: the oracle splits [pux puy] down the middle
    st = wc.setup(x)
    p = dict(x=x, y=st["y"], sigma=st["sigma"], H=st["model"].H_FFT(*st["p_true"]))
    A = lambda v: np.real(np.fft.ifft2(p["H"] * np.fft.fft2(v)))
    AT = lambda v: np.real(np.fft.ifft2(np.conj(p["H"]) * np.fft.fft2(v)))
    invLS = lambda r, mu: np.real(np.fft.ifft2(np.fft.fft2(r) / (np.abs(p["H"]) ** 2 + mu)))
    ident = lambda v: v
    for stop, init in ((3, 0), (1, 2), (2, 2)):
        kw = dict(true_x=p["x"], stopcriterion=stop, tolA=1e-3, maxiter=25, initialization=init, epsilon=0.0)
        ref = o.CSALSA_v2(p["y"], A, 1.0, 1.0, p["sigma"], AT=AT, invLS=invLS, TViters=5, **kw)
        got = cr.csalsa_wavelet_literal(p["y"], A, AT, invLS, ident, ident, cr.TVProx(p["y"].shape, 5), o.TVnorm, 1.0, 1.0,
                                        p["sigma"], **kw)
        assert got["n_outer"] == ref["n_outer"] > 2
        assert (got["numA"], got["numAt"], got["epsilon"]) == (ref["numA"], ref["numAt"], ref["epsilon"])
        for k in ("x", "u", "v", "objective", "distance1", "distance2", "criterion", "mses"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases_stop_where_the_table_says_with_margins(name):
    p, ref = cc.problem(name), cc.reference(name)
    n, tolA = ref["n_outer"], p["tolA"]
    assert n == p["stops_at"], (name, n)
    assert p["form"] == cc.library_form(p["y"].shape, p["delta"])
    assert ref["epsilon"] == pytest.approx(p["eps"], rel=1e-15)
    for k in ("objective", "distance1", "distance2", "criterion", "times", "mses"):
        assert len(ref[k]) == n, k
    assert len(ref["stopvalue"]) == len(ref["n_ve"]) == n - 1
    assert (ref["numA"], ref["numAt"]) == (2 + (n - 1), 1 + (1 if isinstance(p["init"], int) and p["init"] == 2 else 0) + (n - 1))
    ball = ref["n_ve"] / ref["epsilon"]
    print(f"{name}: ||ve|| / epsilon closest to 1: {ball[np.argmin(np.abs(ball - 1))]:.5f}; inside the ball in "
          f"{int(np.sum(ball <= 1))} of {n - 1} iterations")
    assert np.min(np.abs(ball - 1)) >= 1e-3
    if name == "i":
        assert 0 < np.sum(ball <= 1) < n - 1                  # both branches of the projection
    if name not in cc.INSIDE:
        assert n == p["maxiter"]
        return
    assert 2 < n < p["maxiter"]
    sv, ce = ref["stopvalue"], ref["criterion"][1:] / ref["epsilon"]      # entry outer - 2 of both
    print(f"{name}: rule value {sv[-2]:.4e} at {n - 1}, {sv[-1]:.4e} at {n}, tolA {tolA:.1e}; criterion / epsilon {ce[-2]:.5f}, "
          f"{ce[-1]:.5f}")
    assert sv[-1] < tolA and ce[-1] <= 1
    for j in (-1, -2):
        assert abs(sv[j] / tolA - 1) >= 0.01 and abs(ce[j] - 1) >= 1e-3
    # no earlier iteration comes within the margins of stopping
    assert np.all((sv[:-1] >= 1.01 * tolA) | (ce[:-1] >= 1 + 1e-3))


def test_the_constraint_decides_case_g():
    ref, p = cc.reference("g"), cc.problem("g")
    sv, ce = ref["stopvalue"], ref["criterion"][1:] / ref["epsilon"]
    assert sv[-2] < p["tolA"] and ce[-2] > 1 >= ce[-1]


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_literal_iteration_and_state_form_agree_within_the_gpu_bars(name):
    ref, got = cc.reference(name), cc.state_form(name)
    rel = lambda k: float(np.max(np.abs(got[k][ref[k] != 0] / ref[k][ref[k] != 0] - 1)))
    print(f"{name} ({cc.problem(name)['form']}): stopped at {ref['n_outer']} / {got['n_outer']}; relative: objective "
          f"{rel('objective'):.1e}, criterion {rel('criterion'):.1e}, distance1 {rel('distance1'):.1e}, distance2 "
          f"{rel('distance2'):.1e}, mses {rel('mses'):.1e}; max|dx| {np.max(np.abs(got['x'] - ref['x'])):.1e}")
    assert got["n_outer"] == ref["n_outer"]
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"])
    np.testing.assert_allclose(got["objective"], ref["objective"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["criterion"], ref["criterion"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(got["distance1"], ref["distance1"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got["distance2"], ref["distance2"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["mses"], ref["mses"], rtol=1e-9, atol=0)
    assert np.max(np.abs(got["x"] - ref["x"])) < 1e-7


@pytest.mark.parametrize("name", cc.INSIDE)
def test_the_returned_x_is_feasible(name):
    p, ref = cc.problem(name), cc.reference(name)
    f = cc.feasible(p, ref["x"])
    print(f"{name}: ||B x - y|| / epsilon = {f:.5f}")
    assert f <= 1


def test_the_threshold_acts():
    for name in ("a", "g"):
        zero = float(np.mean(cc.reference(name)["u"] == 0.0))
        print(f"{name}: {100 * zero:.1f} % of u is zero")
        assert zero > 0


def test_entry_point_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    name, nargs = "sbtv_CSALSA_wavelet", 29
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == nargs
    assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(sbtv.csalsa_wavelet) and "csalsa_wavelet" in sbtv.__all__
