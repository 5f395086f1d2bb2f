"""CPU: the NumPy restatements of the masked-observation wavelet SALSA (tests/masked_analysis_restatement.py) on the cases of
tests/masked_analysis_cases.py, and what the GPU tests (tests/test_gpu_masked_analysis.py) rely on.

Anchor (i): with identity handles, the oracle's chambolle_prox_TV_stop (warm duals) as psi and TVnorm as phi the literal iteration
is masked_restatement.salsa_masked bit for bit.
Anchor (ii): with m = 1 the literal iteration reaches the fixed point of analysis_restatement.salsa_analysis_literal (64 x 64, Haar,
levels 4, rule 1 with tolA 1e-12, at most 3000 iterations).  Measured here: objective 5.1e-10 relative and PSNR 4.0e-6 dB apart
at mu2 = 1 (both run their 3000 iterations), 6.5e-7 and 5.2e-5 dB at mu2 = 0.1 (the masked form stops at 2081); the bars are
1e-5 and 5e-3 dB.
Literal against state form: both stop at the same iteration on every case; the worst relative difference measured over the
seven cases is 1.1e-15 in objective, 1.5e-14 in distance, 3.7e-15 in mses, and 5.0e-13 absolute in x (pixel values in 0..255).
The assertions stand at 100 times those: 1.1e-13, 1.5e-12, 3.7e-13 and 5.0e-11, each far below a tenth of the GPU bars
(1e-9, 1e-7, 1e-9, 1e-7).
The cases whose rule fires inside the loop do so where the table says, with the criterion at the stopping iteration and at the one
before each at least 1 % away from tolA.
The property: on the `man` problem of masked_analysis_cases.property_problem the literal iteration scores 25.06 dB over the
observed pixels in 87 iterations, salsa_analysis_literal on the 250 x 250 observation 21.02 dB in 81 (both with peak 255 over the
same 250 x 250 pixels): +4.0 dB; the bar is +2 dB."""
import os
import re

import numpy as np
import pytest

import analysis_restatement as ar
import masked_analysis_cases as mc
import masked_analysis_restatement as mar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 100 times the worst difference measured between the literal and the state form (module docstring)
STATE_RTOL = dict(objective=1.1e-13, distance=1.5e-12, mses=3.7e-13)
STATE_X_ATOL = 5.0e-11
GPU_RTOL = dict(objective=1e-9, distance=1e-7, mses=1e-9)
GPU_X_ATOL = 1e-7


@pytest.mark.parametrize("stop,init,mu2", [(1, 0, 0.1), (2, 2, 1.0), (3, "array", 0.3)])
def test_identity_handles_and_the_tv_prox_give_the_masked_restatement_bit_for_bit(stop, init, mu2):
    import masked_restatement as mr
    import sbtv_oracle as o
    p = mc.problem("b")                                       # 128 x 128, frame mask with holes
    if init == "array":
        init = np.random.default_rng(5).uniform(0, 255, size=p["x"].shape)
    tau, mu1, K = 0.03 * p["tau"], 0.003, 5
    kw = dict(true_x=p["x"], stopcriterion=stop, tolA={1: 1e-3, 2: 1e-2, 3: 0.0}[stop], maxiter=12, initialization=init)
    ref = mr.salsa_masked(p["y"], p["m"], p["H"], tau, mu1, mu2, TViters=K, **kw)
    ident = lambda a: a
    got = mar.salsa_masked_literal(p["y"], p["m"], p["H"], tau, mu1, mu2, ident, ident, mar.WarmChambolle(p["x"].shape, K),
                                   o.TVnorm, **kw)
    assert got["n_outer"] == ref["n_outer"] and (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"])
    for k in ("x", "objective", "distance", "mses", "u", "v", "bu", "bv"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("mu2", [1.0, 0.1])
def test_full_mask_reaches_the_fixed_point_of_the_analysis_restatement(mu2):
    import sbtv_oracle as o
    p = mc.problem("a")                                       # 64 x 64, Haar, levels 4
    y = mc.wc.setup(p["x"])["y"]                              # the whole observation: m = 1
    kw = dict(stopcriterion=1, tolA=1e-12, maxiter=3000, initialization=0)
    ref = ar.salsa_analysis_literal(y, p["H"], p["h"], p["levels"], p["tau"], p["mu1"], **kw)
    got = mar.salsa_masked_analysis_literal(y, np.ones_like(y), p["H"], p["h"], p["levels"], p["tau"], p["mu1"], mu2, **kw)
    dobj = abs(got["objective"][-1] / ref["objective"][-1] - 1)
    dpsnr = abs(o.PSNR(p["x"], got["x"]) - o.PSNR(p["x"], ref["x"]))
    print(f"mu2 = {mu2}: {got['n_outer']} / {ref['n_outer']} iterations, objective {dobj:.2e} relative, PSNR {dpsnr:.2e} dB apart")
    assert dobj <= 1e-5 and dpsnr <= 5e-3


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_literal_iteration_and_state_form_agree(name):
    ref, got = mc.reference(name), mc.state_form(name)
    rel = {k: float(np.max(np.abs(got[k] / ref[k] - 1))) for k in STATE_RTOL}
    dx = float(np.max(np.abs(got["x"] - ref["x"])))
    print(f"{name}: stopped at {ref['n_outer']} / {got['n_outer']}, relative: " + ", ".join(f"{k} {v:.1e}" for k, v in rel.items()) +
          f", x {dx:.1e} absolute")
    assert got["n_outer"] == ref["n_outer"]
    for k, bar in STATE_RTOL.items():
        assert bar <= 0.1 * GPU_RTOL[k]
        assert got[k].shape == ref[k].shape
        np.testing.assert_allclose(got[k], ref[k], rtol=bar, atol=0, err_msg=k)
    assert STATE_X_ATOL <= 0.1 * GPU_X_ATOL and dx < STATE_X_ATOL
    p = mc.problem(name)
    start2 = not isinstance(p["init"], np.ndarray) and p["init"] == 2
    n = ref["n_outer"]
    assert (got["numA"], got["numAt"]) == (ref["numA"], ref["numAt"]) == (1 + n, n + (1 if start2 else 0))
    assert mc.calls(p, n) == 1 + (1 if start2 else 0) + 2 * n


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_cases_stop_where_the_table_says_with_a_margin(name):
    p, ref = mc.problem(name), mc.reference(name)
    n = ref["n_outer"]
    assert n == p["stops_at"], (name, n)
    assert len(ref["objective"]) == len(ref["mses"]) == len(ref["times"]) == n + 1 and ref["distance"].shape == (n, 2)
    if name not in mc.INSIDE:
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


def test_the_objective_falls_and_inpainting_lowers_the_error():
    a, g = mc.reference("a"), mc.reference("g")
    assert a["objective"][-1] < a["objective"][0]
    assert g["mses"][-1] < g["mses"][0]
    assert float(np.mean(a["u"] == 0.0)) > 0                  # the threshold acts


def test_the_masked_form_beats_the_periodic_form_on_an_observation_without_wrapped_pixels():
    """The bar of the GPU test on the reference alone."""
    q = mc.property_problem()
    kw = dict(stopcriterion=q["stop"], tolA=q["tolA"], maxiter=q["maxiter"], initialization=0)
    per = ar.salsa_analysis_literal(q["y_obs"], q["H_obs"], q["h"], q["levels"], q["tau"], q["mu1"], **kw)
    msk = mar.salsa_masked_analysis_literal(q["y"], q["m"], q["H"], q["h"], q["levels"], q["tau"], q["mu1"], q["mu2"], **kw)
    t = mc.TAILLE
    obs = q["scene"][t - 1:, t - 1:]
    p_per = mc.psnr_over(np.ones_like(obs), obs, per["x"])
    p_msk = mc.psnr_over(q["m"], q["scene"], msk["x"])
    print(f"periodic {p_per:.2f} dB ({per['n_outer']} iterations), masked {p_msk:.2f} dB ({msk['n_outer']} iterations)")
    assert p_msk >= p_per + 2.0


def test_masked_analysis_entry_point_declared_exported_and_bound():
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    lib = sbtv.load_library()
    name, nargs = "sbtv_SALSA_masked_analysis", 26
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == nargs
    assert hasattr(lib, name), f"{name} is not exported by libsbtv.so"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(sbtv.SALSA_masked_analysis) and "SALSA_masked_analysis" in sbtv.__all__
    shim = os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd", "matlab", "sbtv_salsa_masked_analysis.m")
    assert f"'{name}'" in open(shim).read()
