"""CPU: the restated masked-observation MYULA chain and SAPG loop (tests/masked_sapg_restatement.py) on the cases of
tests/masked_sapg_cases.py, and the presence of the feature in the built library.

The restatement is anchored three ways: with m = 1 it is the oracle's SAPG_algorithm / myula; central differences of the
masked negative log-likelihood  n_obs/2 log s2 + R/(2 s2)  give its gradF, its G_p and (with the sign of the ascent the loop
takes in sigma2) its G_sigma, which pins n_obs and the mask's place in every sum; and y under m = 0 moves no output.  No prox
call of a case sits on the edge of the Chambolle stop rule, so a last-bit difference between two correct implementations
cannot change an iteration count: that is what makes the bars of tests/test_gpu_sapg_masked.py meaningful."""

import numpy as np
import pytest

import masked_sapg_cases as msc
import masked_sapg_restatement as msr
import sbtv_oracle as o

TRACES = ("thetas", "sigmas", "ps", "logpi", "logpi_wu", "gx", "grads")


# ---- the feature is there --------------------------------------------------------------------------------------------
def test_library_exports_the_masked_entries():
    import sbtv
    from sbtv import _lib
    lib = sbtv.load_library()
    for name in ("sbtv_myula_masked", "sbtv_SAPG_masked"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 23


def test_python_entries_exist():
    import sbtv
    for name in ("SAPG_masked", "myula_masked"):
        assert callable(getattr(sbtv, name)) and name in sbtv.__all__


# ---- m = 1: the oracle ------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz = b != 0
    return float(np.max(np.abs(a[nz] / b[nz] - 1))) if np.any(nz) else 0.0


@pytest.mark.parametrize("name", ["gauss-valid", "moffat-holes", "laplace-weights"])
def test_with_a_mask_of_ones_the_sapg_restatement_is_the_oracle(name):
    q = msc.problem(name)
    st, kw = q["setup"], q["kw"]
    nz = iter(q["noise"])
    ref = o.SAPG_algorithm(st, kw["samples"], kw["warmup"], kw["burnIn"], lambda shape: next(nz), chambolleit=kw["chambolleit"],
                           fix=kw["fix"], c=kw["c"])
    got = msc.chain(name, mask=np.ones_like(q["mask"]))
    pairs = [("thetas", got["thetas"], ref["thetas"]), ("sigmas", got["sigmas"], ref["sigmas"]), ("ps", got["ps"], ref["ps"]),
             ("logpi", got["logpi"], ref["logPiTraceX"]), ("logpi_wu", got["logpi_wu"], ref["logPiTrace_WU"]),
             ("gx", got["gx"], ref["gXTrace"]), ("grads", got["grads"], ref["grads"]),
             ("theta_EB", got["theta_EB"], ref["theta_EB"]), ("p_EB", got["p_EB"], ref["p_EB"]),
             ("sigma_EB", got["sigma_EB"], ref["sigma_EB"]), ("last sample", got["samples"][-1], ref["Xlast_sample"])]
    print(f"{name}, m = 1: " + ", ".join(f"{k} {_rel(a, b):.1e}" for k, a, b in pairs))
    for k, a, b in pairs:
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=k)


@pytest.mark.parametrize("name", ["moffat-holes", "tiny"])
def test_with_a_mask_of_ones_the_myula_restatement_is_the_oracle(name):
    q = msc.myula_problem(name)
    model, y, p, s2 = q["model"], q["y"], q["p"], q["s2"]
    op = {"y": y, "lambda": q["lam"], "gamma": q["gam"], "theta_op": q["theta"], "tau_op": p, "samples": q["samples"],
          "gradF": lambda x, tau: np.real(model.AT(model.A(x, *tau) - y, *tau)) / s2,
          "proxG": lambda x, lam, theta: o.chambolle_prox_TV_stop(x, lam=lam * theta, maxiter=msc.CHAMBOLLEIT)[0]}
    nz = iter(q["noise"])
    ref = o.myula(op, y, lambda shape: next(nz))
    got = msc.myula_chain(name, mask=np.ones_like(q["mask"]))
    print(f"{name}, m = 1: myula last sample {_rel(got['x'], ref):.1e}")
    np.testing.assert_allclose(got["x"], ref, rtol=1e-12, atol=0)
    assert got["samples"].shape == (q["samples"] - 1,) + y.shape


# ---- the gradients are those of the stated likelihood --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["laplace-weights", "gauss-valid"])
def test_central_differences_of_the_negative_log_likelihood_give_the_gradients(name):
    """d/dx = gradF, d/dp_q = G_p(q), d/ds2 = -G_sigma (the loop ascends in sigma2), each to 1e-5 relative.  The likelihood is
    quadratic in x, so a pixel's central difference is exact up to rounding / |gradF|: the pixels are drawn among those whose
    gradient is at least a tenth of the largest."""
    q = msc.problem(name)
    st, model, m = q["setup"], q["model"], q["mask"]
    y = st["y"]
    rng = np.random.default_rng(5)
    x = np.abs(y + 3.0 * rng.standard_normal(y.shape))
    p = tuple(o.DEMO[q["kind"]]["init"])
    s2 = st["sigma_init"]
    nll = lambda xx, pp, ss: msr.neg_log_likelihood(model, xx, pp, ss, y, m)
    assert msr.n_obs(m) < m.size and (name != "laplace-weights" or msr.n_obs(m) != np.sum(m))
    g = msr.gradF(model, x, p, s2, y, m)
    big = np.argwhere(np.abs(g) >= 0.1 * np.max(np.abs(g)))
    figs = []
    for i, j in big[rng.choice(len(big), size=4, replace=False)]:
        h = 1e-2
        e = np.zeros_like(x)
        e[i, j] = h
        fd = (nll(x + e, p, s2) - nll(x - e, p, s2)) / (2 * h)
        figs.append(abs(fd / g[i, j] - 1))
        assert fd == pytest.approx(g[i, j], rel=1e-5), (i, j)
    for k in range(len(p)):
        h = 1e-5 * p[k]
        up, dn = list(p), list(p)
        up[k] += h
        dn[k] -= h
        fd = (nll(x, tuple(up), s2) - nll(x, tuple(dn), s2)) / (2 * h)
        G = msr.G_p(model, k, x, p, s2, y, m)
        figs.append(abs(fd / G - 1))
        assert fd == pytest.approx(G, rel=1e-5), k
    h = 1e-5 * s2
    fd = (nll(x, p, s2 + h) - nll(x, p, s2 - h)) / (2 * h)
    Gs = msr.G_sigma(model, x, p, s2, y, m)
    figs.append(abs(-fd / Gs - 1))
    print(f"{name}: n_obs = {msr.n_obs(m)}, sum(m) = {np.sum(m):g}; relative differences (4 pixels, G_p, G_sigma): "
          + ", ".join(f"{v:.1e}" for v in figs))
    assert -fd == pytest.approx(Gs, rel=1e-5)


# ---- y under m = 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss-valid", "laplace-weights"])
def test_y_under_a_zero_of_the_mask_moves_nothing(name):
    q = msc.problem(name)
    y, m = q["setup"]["y"], q["mask"]
    x0 = 0.5 * y + 20.0
    a = msc.chain(name, x0=x0)
    b = msc.chain(name, x0=x0, y=np.where(m > 0, y, 1e6))
    for k in TRACES + ("samples", "k"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    mq = msc.myula_problem(name)
    c = msc.myula_chain(name)
    d = msc.myula_chain(name, y=np.where(m > 0, mq["y"], 0.0))
    assert np.any(c["samples"][0] != d["samples"][0])                    # the one exception: the chain starts from y as given
    np.testing.assert_array_equal(msr.gradF(mq["model"], c["x"], mq["p"], mq["s2"], mq["y"], m),
                                  msr.gradF(mq["model"], c["x"], mq["p"], mq["s2"], np.where(m > 0, mq["y"], 1e6), m))


# ---- the stop rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", msc.NAMES)
def test_no_prox_call_sits_on_the_edge_of_the_stop_rule(name):
    """Every prox call gives the same iteration count at tol (1 - 1e-6), tol and tol (1 + 1e-6)."""
    r = msc.chain(name, alt_tols=(msr.TOL * (1 - 1e-6), msr.TOL * (1 + 1e-6)))
    calls = 1 + (msc.WARMUP - 1) + 1 + (msc.SAMPLES - 1)
    assert r["k"].shape == (calls,) and r["k_alt"].shape == (calls, 2)
    fired = r["err"] <= msr.TOL
    margin = np.min(np.abs(r["err"][fired] / msr.TOL - 1)) if np.any(fired) else float("nan")
    print(f"{name}: k = {r['k'].min()} .. {r['k'].max()}, the rule fired in {int(np.sum(fired))} of {calls} calls, "
          f"closest final err to tol: {margin:.2%}")
    np.testing.assert_array_equal(r["k_alt"][:, 0], r["k"])
    np.testing.assert_array_equal(r["k_alt"][:, 1], r["k"])
    assert np.all(r["k"] >= 1) and np.all(r["k"] <= msc.CHAMBOLLEIT)
    np.testing.assert_array_equal(r["samples"], msc.reference(name)["samples"])     # the extra runs change nothing


@pytest.mark.parametrize("name", msc.NAMES)
def test_restated_loop_is_finite_and_keeps_the_layout_of_the_myula_loop(name):
    q, r = msc.problem(name), msc.reference(name)
    S = msc.SAMPLES
    assert r["samples"].shape == (S,) + q["setup"]["y"].shape
    for k in TRACES + ("samples",):
        assert np.all(np.isfinite(r[k])), k
    assert r["gx"][-1] == 0.0 and r["logpi_wu"][0] == 0.0 and not np.any(r["grads"][:, 0])      # the index quirks, kept
    assert r["thetas"][0] == q["op"]["th_init"] and r["sigmas"][0] == q["op"]["sigma_init"]
    assert np.all(r["samples"][1:] >= 0)                                 # the reflecting abs()
    assert float(np.max(np.abs(r["samples"]))) < 1e4                     # the data are 0..255 images
    # the parameters may sit on their clamps (sigma2 and Laplace's b do, as in the demo at this size); every gradient is live
    assert np.all(r["grads"][:, 1:] != 0) and len(set(r["thetas"].tolist())) > 2
