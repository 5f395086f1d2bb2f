"""CPU: the two NumPy restatements of the analysis-prior wavelet SALSA (tests/analysis_restatement.py) on the cases of
tests/analysis_cases.py, and what the GPU tests rely on: the literal SALSA_v2 iteration and the (s, bu) form the library runs
stop at the same iteration and agree to 1e-10 relative in objective / distance / mses and 1e-8 absolute in x; every case
stops where its table entry says; and where the rule fires inside the loop, the criterion at the stopping iteration and at
the one before are each at least 1 % away from tolA, so no rounding within the bars of the GPU tests (1e-9 relative) can
move the stop."""
import os
import re

import numpy as np
import pytest

import analysis_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_literal_iteration_and_operator_form_agree(name):
    ref, got = ac.reference(name), ac.operator_form(name)
    print(f"{name}: stopped at {ref['n_outer']} / {got['n_outer']}, objective "
          f"{np.max(np.abs(got['objective'] / ref['objective'] - 1)):.1e}, distance "
          f"{np.max(np.abs(got['distance'] / ref['distance'] - 1)):.1e}, mses {np.max(np.abs(got['mses'] / ref['mses'] - 1)):.1e} "
          f"apart (relative), x {np.max(np.abs(got['x'] - ref['x'])):.1e}")
    assert got["n_outer"] == ref["n_outer"]
    for k in ("objective", "distance", "mses"):
        assert got[k].shape == ref[k].shape
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-10, atol=0, err_msg=k)
    assert np.max(np.abs(got["x"] - ref["x"])) < 1e-8
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"]) == (1 + ref["n_outer"], 1)


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_cases_stop_where_the_table_says_with_a_margin(name):
    p, ref = ac.problem(name), ac.reference(name)
    n = ref["n_outer"]
    assert n == p["stops_at"], (name, n)
    assert len(ref["objective"]) == len(ref["mses"]) == len(ref["times"]) == n + 1 and len(ref["distance"]) == n
    if name not in ac.INSIDE:
        assert n == p["maxiter"]
        return
    assert 2 < n < p["maxiter"]
    crit = ref["criterion"]                                   # entry outer - 2
    assert len(crit) == n - 1
    last, before = crit[n - 2], crit[n - 3]
    print(f"{name}: criterion {before:.4e} at {n - 1}, {last:.4e} at {n}, tolA {p['tolA']:.4e}")
    assert last < p["tolA"] <= before
    assert abs(last / p["tolA"] - 1) >= 0.01 and abs(before / p["tolA"] - 1) >= 0.01
    assert np.all(crit[:n - 2] >= p["tolA"])


def test_the_threshold_acts():
    """u of the literal form is sparse."""
    for name in ("a", "g"):
        u = ac.reference(name)["u"]
        zero = float(np.mean(u == 0.0))
        print(f"{name}: {100 * zero:.1f} % of u is zero")
        assert zero > 0


def test_a_threshold_above_every_coefficient_keeps_u_at_zero():
    """huge_tau on the literal form: u is zero throughout and the bound of its docstring holds with room."""
    import analysis_restatement as ar
    p = ac.problem("f")
    r = ar.salsa_analysis_literal(p["y"], p["H"], p["h"], p["levels"], ac.huge_tau(p), p["mu"], stopcriterion=2, tolA=0.0, maxiter=6,
                                  initialization=0)
    assert r["n_outer"] == 6 and not np.any(r["u"])
    np.testing.assert_allclose(r["distance"], 1.0, rtol=1e-12)
    assert np.max(np.abs(r["bu"])) < 0.2 * ac.huge_tau(p) / p["mu"]


def test_analysis_entry_point_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    name, nargs = "sbtv_SALSA_analysis", 24
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == nargs
    assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(sbtv.SALSA_analysis) and "SALSA_analysis" in sbtv.__all__
