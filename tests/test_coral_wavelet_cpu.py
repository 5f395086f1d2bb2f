"""CPU: the NumPy restatements of CoRAL with the TV + wavelet-l1 regulariser (tests/coral_wavelet_restatement.py) on the cases of
tests/coral_wavelet_cases.py, and what the GPU tests rely on:

* the literal form with P1 = P2 = identity and TV on both terms IS sbtv_oracle.CoRAL_v2, bit for bit;
* the literal form and the state form the library runs stop at the same iteration and agree at the bars
  tests/test_analysis_cpu.py uses for its two forms (1e-10 relative in objective / distance / mses, 1e-8 absolute in x);
* every case stops where its table entry says, and where the rule fires inside the loop the criterion at the stopping iteration
  and at the one before are each at least 1 % away from tolA, so no rounding within the bars of the GPU tests can move the stop;
* every Chambolle step's err is at least 1 % away from the inner tolerance (the first prox of a run has a zero input and stops
  at k = 1 with err = 0, every later one runs all TViters steps), so the optimistic launches and the exact rule cannot differ;
* the compound solution has a lower compound objective than the solutions of either single-regulariser problem."""
import os
import re

import numpy as np
import pytest

import analysis_restatement as ar
import coral_wavelet_cases as cc
import coral_wavelet_restatement as cr
import sbtv_oracle as o
import wavelet_restatement as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("start", [0, 2])
def test_literal_form_with_two_tv_terms_is_the_oracle_coral(start):
    p = cc.problem("1")
    mu1, mu2 = 0.05, 0.08
    A, AT, invLS = cr.blur_handles(p["H"], mu1 + mu2)
    kw = dict(true_x=p["x"], stopcriterion=1, tolA=1e-3, maxiter=12, initialization=start)
    ref = o.CoRAL_v2(p["y"], A, p["tau1"], 0.7 * p["tau2"], mu1=mu1, mu2=mu2, AT=AT, invLS=invLS, TViters1=5, TViters2=3, **kw)
    got = cr.coral_literal(p["y"], A, AT, invLS, p["tau1"], 0.7 * p["tau2"], mu1, mu2, ("tv", 5), ("tv", 3), **kw)
    assert got["n_outer"] == ref["n_outer"] > 2
    for k in ("x", "u", "v", "objective", "distance", "mses", "criterion"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_literal_iteration_and_operator_form_agree(name):
    ref, got = cc.reference(name), cc.operator_form(name)
    print(f"{name}: stopped at {ref['n_outer']} / {got['n_outer']}, objective "
          f"{np.max(np.abs(got['objective'] / ref['objective'] - 1)):.1e}, distance "
          f"{np.max(np.abs(got['distance'] / ref['distance'] - 1)):.1e}, mses {np.max(np.abs(got['mses'] / ref['mses'] - 1)):.1e} "
          f"apart (relative), x {np.max(np.abs(got['x'] - ref['x'])):.1e}")
    assert got["n_outer"] == ref["n_outer"]
    for k in ("objective", "distance", "mses"):
        assert got[k].shape == ref[k].shape
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-10, atol=0, err_msg=k)
    assert np.max(np.abs(got["x"] - ref["x"])) < 1e-8
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"]) == (1 + ref["n_outer"], 2)
    assert [k for k, _ in got["prox1"]] == [k for k, _ in ref["prox1"]]


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases_stop_where_the_table_says_with_a_margin(name):
    p, ref = cc.problem(name), cc.reference(name)
    n = ref["n_outer"]
    assert n == p["stops_at"], (name, n)
    assert len(ref["objective"]) == len(ref["mses"]) == len(ref["times"]) == n + 1 and ref["distance"].shape == (n, 2)
    if name not in cc.INSIDE:
        assert n == p["maxiter"]
        return
    assert 2 < n < p["maxiter"]
    crit = ref["criterion"]                                   # entry outer - 1; entry 0 is the reference's criterion(1) = 1
    assert len(crit) == n
    last, before = crit[n - 1], crit[n - 2]
    print(f"{name}: criterion {before:.4e} at {n - 1}, {last:.4e} at {n}, tolA {p['tolA']:.4e}")
    assert last < p["tolA"] <= before
    assert abs(last / p["tolA"] - 1) >= 0.01 and abs(before / p["tolA"] - 1) >= 0.01
    assert np.all(crit[1:n - 1] >= p["tolA"])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_every_chambolle_step_is_clear_of_the_inner_tolerance(name):
    p, ref = cc.problem(name), cc.reference(name)
    tol = cr.CHAMBOLLE_TOL
    ks = [k for k, _ in ref["prox1"]]
    errs = np.array([e for steps in ref["steps1"] for e in steps])
    print(f"{name}: iterations per prox {ks}, err nearest to the tolerance {errs[np.argmin(np.abs(errs - tol))]:.3e}")
    assert len(ks) == ref["n_outer"] and errs.size == sum(ks)
    assert ks[0] == 1 and ref["steps1"][0] == [0.0]           # the first input x - bu is exactly zero
    assert ks[1:] == [p["TViters"]] * (ref["n_outer"] - 1)
    assert np.all(np.abs(errs / tol - 1) >= 0.01)


def test_a_flat_observation_stops_every_prox_at_its_first_step():
    p, ref = cc.flat_problem(), cc.flat_reference()
    assert ref["n_outer"] == 6
    assert [k for k, _ in ref["prox1"]] == [1] * 6
    errs = [e for steps in ref["steps1"] for e in steps]
    print("flat: err of each prox", errs)
    assert max(errs) < 0.01 * cr.CHAMBOLLE_TOL
    # every trace entry is of ordinary size (coral_wavelet_cases.flat_problem says why the PSF has a gain)
    assert np.all(ref["objective"] > 1.0) and np.all(ref["distance"] > 1e-6) and np.all(ref["mses"] > 1.0)
    got = cc.run(cr.coral_wavelet_operator, p)
    np.testing.assert_allclose(got["objective"], ref["objective"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got["distance"], ref["distance"], rtol=1e-8, atol=0)


def test_compound_solution_beats_both_single_regulariser_solutions():
    """Case 1 with tau1 = sigma^2, tau2 = 0.5 sigma^2, rule 1 at 1e-6.  (With the case's own tau1 = tau2 = 0.5 sigma^2 the gap to
    the wavelet-only solution is 106 of 3.06e5, 0.03 %, too close to what the tolerance leaves open; with these it is 364 of 3.15e5
    while the compound run at 1e-9 lowers F by 22.)"""
    p = cc.problem("1")
    tau1, tau2 = p["sigma"] ** 2, 0.5 * p["sigma"] ** 2
    A, AT, invLS1 = cr.blur_handles(p["H"], p["mu1"])
    kw = dict(stopcriterion=1, tolA=1e-6, maxiter=5000, initialization=2)

    def F(x):
        return 0.5 * wr._sq(p["y"] - A(x)) + tau1 * o.TVnorm(x) + tau2 * float(np.sum(np.abs(wr.mrdwt_TI2D(x, p["h"], p["levels"]))))

    both = cr.coral_wavelet(p["y"], p["H"], p["h"], p["levels"], tau1, tau2, p["mu1"], p["mu2"], TViters=p["TViters"], **kw)
    tv = o.SALSA_v2(p["y"], A, tau1, mu=p["mu1"], AT=AT, invLS=invLS1, TViters=p["TViters"], **kw)
    l1 = ar.salsa_analysis_literal(p["y"], p["H"], p["h"], p["levels"], tau2, p["mu2"], **kw)
    for r in (both, tv, l1):
        assert 2 < r["n_outer"] < 5000
    Fb, Ftv, Fl1 = F(both["x"]), F(tv["x"]), F(l1["x"])
    print(f"F(compound) = {Fb:.6e} after {both['n_outer']} iterations; F(TV only) - F = {Ftv - Fb:.4e}, "
          f"F(wavelet-l1 only) - F = {Fl1 - Fb:.4e}")
    assert Fb < Ftv
    assert Fb < Fl1


def test_a_threshold_above_every_coefficient_keeps_v_at_zero():
    """huge_tau2 on the literal form: v is zero throughout, the l1 term of every objective entry is zero, and the bound of its
    docstring holds with room."""
    p = cc.problem("2")
    n = 6
    tau2 = cc.huge_tau2(p, n)
    r = cc.run(cr.coral_wavelet, dict(p, tau2=tau2), stopcriterion=2, tolA=0.0, maxiter=n, initialization=0)
    assert r["n_outer"] == n and not np.any(r["v"])
    np.testing.assert_allclose(r["distance"][:, 1], 1.0, rtol=1e-12)
    A = cr.blur_handles(p["H"], 1.0)[0]
    assert r["objective"][-1] == pytest.approx(0.5 * wr._sq(p["y"] - A(r["x"])) + p["tau1"] * o.TVnorm(r["u"]), rel=1e-12)
    # bv_n = -W'S_n: the largest soft argument the run could still meet is below max|bv| + max|W'x| <= 2 t_n
    assert np.max(np.abs(r["bv"])) < (tau2 / p["mu2"]) / 3.0


def test_coral_wavelet_entry_point_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    name, nargs = "sbtv_CoRAL_wavelet", 26
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == nargs
    assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(sbtv.CoRAL_wavelet) and "CoRAL_wavelet" in sbtv.__all__



def test_a_group_context_is_refused_before_anything_else():
    import sbtv

    class FakeGroup:
        is_group = True

    with pytest.raises(NotImplementedError, match="no sharded variant"):
        sbtv.CoRAL_wavelet(np.zeros((8, 8)), None, 1.0, 1.0, "MU1", 0.1, "MU2", 0.1, ctx=FakeGroup())
