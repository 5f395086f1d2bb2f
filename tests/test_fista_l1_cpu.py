"""CPU: the wavelet-l1 FISTA (sbtv_fista_l1) before any GPU is involved.

(i) the one-synthesis form the library runs (tests/fista_l1_restatement.py, fista_l1_operator) against my_fista_l1.m line for
line (fista_l1_literal): max|dxw| <= 1e-8 and objective rtol 1e-10, a tenth of the GPU bars of tests/test_gpu_fista_l1.py (the
two differ by roundings only: measured 4e-12 on max|xw| ~ 300 and 7e-16); (ii) the cases whose stop rule is meant to fire
inside the loop do so with a margin that the GPU's rounding cannot cross; (iii) (iv) what the zero start and a threshold above
every coefficient must give; (v) the export, its binding and the one refusal that needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fista_l1_cases as fc
import fista_l1_restatement as fr
import wavelet_restatement as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["a", "b", "d", "f", "g"])
def test_operator_form_equals_the_literal_iteration(name):
    lit, op = fc.reference(name), fc.operator_form(name)
    assert lit["n_iter"] == op["n_iter"]
    dx = float(np.max(np.abs(lit["xw"] - op["xw"])))
    do = float(np.max(np.abs(op["objective"] / lit["objective"] - 1.0)))
    print(f"case {name}: n_iter {lit['n_iter']}, max|dxw| = {dx:.1e} on max|xw| = {np.max(np.abs(lit['xw'])):.3g}, objective rel {do:.1e}")
    assert dx <= 1e-8
    np.testing.assert_allclose(op["objective"], lit["objective"], rtol=1e-10)
    np.testing.assert_allclose(op["mses"], lit["mses"], rtol=1e-10)
    assert np.max(np.abs(lit["x"] - op["x"])) <= 1e-8
    assert lit["calls"] == op["calls"] == 2 + 3 * (lit["n_iter"] - 1)


@pytest.mark.parametrize("name,k_stop", [("a", 55), ("b", 28), ("c", 9), ("f", 25)])
def test_stop_rule_fires_inside_the_loop_with_a_margin(name, k_stop):
    """Rule 1 is a difference of nearly equal objectives: a 1e-9 relative error of the objective moves a criterion of 1e-4 by
    about 2e-5 relative, so 1 % is a wide margin; rules 2 and 3 carry the relative error of their sums, 1e-3 is."""
    p, ref = fc.problem(name), fc.reference(name)
    n, crit = ref["n_iter"], ref["criteria"]
    print(f"case {name}: stops at k = {n}, criterion {crit[-2]:.6g} -> {crit[-1]:.6g}, tolerance {p['tol']:.6g}")
    assert n == k_stop
    assert 2 < n < p["maxiters"]
    margin = 1e-2 if p["stop"] == 1 else 1e-3
    assert crit[-1] < p["tol"] * (1 - margin)
    assert crit[-2] > p["tol"] * (1 + margin)
    assert np.all(crit[:-1] >= p["tol"])


def test_zero_start_objective_and_first_iterate():
    p = fc.problem("a")
    r = fr.fista_l1_literal(p["y"], p["H"], p["h"], p["levels"], p["tau"], 1, 0.0, 2, true_xw=p["true_xw"])
    assert r["objective"][0] == 0.5 * wr._sq(p["y"])
    ATb = wr.mrdwt_TI2D(np.real(np.fft.ifft2(np.conj(p["H"]) * np.fft.fft2(p["y"]))), p["h"], p["levels"])
    np.testing.assert_array_equal(r["xw"], wr.soft(ATb, p["tau"]))
    assert r["n_iter"] == 2 and r["mses"][0] == wr._sq(p["true_xw"]) / p["true_xw"].size


@pytest.mark.parametrize("fn", [fr.fista_l1_literal, fr.fista_l1_operator], ids=["literal", "operator"])
def test_a_threshold_above_every_coefficient_keeps_x_at_zero(fn):
    p = fc.problem("f")
    tau = fc.huge_tau(p)
    r2 = fn(p["y"], p["H"], p["h"], p["levels"], tau, 2, 1e300, 6)
    assert r2["n_iter"] == 6 and not np.any(r2["xw"]) and np.all(np.isnan(r2["criteria"]))
    assert np.all(r2["objective"] == r2["objective"][0])
    r1 = fn(p["y"], p["H"], p["h"], p["levels"], tau, 1, 1e-6, 6)
    assert r1["n_iter"] == 2 and not np.any(r1["xw"])


def test_export_binding_and_null_context():
    """Fails before the entry point exists."""
    import sbtv
    from sbtv import _lib
    hdr = open(os.path.join(ROOT, "include", "sbtv.h")).read()
    m = re.search(r"\bint\s+sbtv_fista_l1\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "include/sbtv.h does not declare sbtv_fista_l1"
    nparams = len(m.group(1).split(","))
    assert re.search(r"#define\s+SBTV_FISTA_L1_NOLAG\s+2\b", hdr) and _lib.FISTA_L1_NOLAG == 2
    assert re.search(r"#define\s+SBTV_VERSION\s+100\b", hdr)
    assert "sbtv_fista_l1" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sbtv_fista_l1"][1]) == nparams == 24
    assert callable(sbtv.my_fista_l1) and "my_fista_l1" in sbtv.__all__
    lib = sbtv.load_library()
    assert hasattr(lib, "sbtv_fista_l1")
    z = np.zeros(4)
    n = (C.c_int * 1)()
    rc = lib.sbtv_fista_l1(None, _lib.vptr(z), 2, 2, 1, _lib.vptr(z), 1, _lib.vptr(z), 2, 2, _lib.vptr(z), 1.0, 1, 0.0, 1,
                           None, None, _lib.vptr(z), None, None, None, None, n, 0)
    assert rc == -1                                                      # SBTV_ERR_BADARG
