"""CPU: the semi-blind wavelet-l1 loop without a GPU (tests/wavelet_sb_restatement.py on the cases of
tests/wavelet_sb_cases.py).  The fused form the library runs against the literal loop; the literal loop with every parameter
fixed against the theta-only restatement; the PSF-parameter gradient against a finite difference of the data term; the
behaviour the GPU cases rely on (b visits its lower bound and leaves it, sigma2 visits its upper bound and leaves it); the
sensitivity of every GPU parity case to a 1e-12 perturbation of its start; the boundary; the compiler's resource report."""
import os
import re

import numpy as np
import pytest

from test_kernel_resources import HIPCC, _find, _report

import wavelet_restatement as wr
import wavelet_sapg_restatement as wsr
import wavelet_sb_cases as wbc
import wavelet_sb_restatement as wsb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = ("thetas", "ps", "sigmas", "grads", "gXTrace", "logPiTraceX", "logPiTrace_WU", "mean_thetas", "tol_thetas",
          "mean_ps", "tol_ps")


def worst(got, ref, keys=TRACES, by_scale=()):
    """Largest relative difference over the traces, the EB estimates and the last sample of all chains: entry by entry,
    except for the traces named in `by_scale`, which are measured row by row against the row's largest magnitude."""
    w = 0.0
    for (eb, r), (eb_ref, rr) in zip(got, ref):
        for k in keys:
            assert (k in r) == (k in rr), k
            if k not in rr:
                continue
            a, c = np.asarray(r[k], dtype=np.float64), np.asarray(rr[k], dtype=np.float64)
            assert a.shape == c.shape, (k, a.shape, c.shape)
            np.testing.assert_array_equal(np.isnan(a), np.isnan(c), err_msg=k)
            fin = np.isfinite(c)
            if k in by_scale:
                a2, c2 = np.atleast_2d(a), np.atleast_2d(c)
                for q in range(c2.shape[0]):
                    if np.max(np.abs(c2[q])) > 0:
                        w = max(w, float(np.max(np.abs(a2[q] - c2[q])) / np.max(np.abs(c2[q]))))
                continue
            if k.startswith("tol_"):                          # a difference of two nearly equal means: absolute below 1e-9
                small = fin & (np.abs(c) < 1e-9)
                assert np.all(np.abs(a[small] - c[small]) <= 1e-12), k
                fin = fin & ~small
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(c[fin] != 0, np.abs(a[fin] / c[fin] - 1), np.abs(a[fin]))
            w = max(w, float(rel.max()) if rel.size else 0.0)
        for k in ("theta", "sigma2"):
            w = max(w, abs(eb[k] / eb_ref[k] - 1))
        w = max(w, float(np.max(np.abs(eb["p"] / eb_ref["p"] - 1))))
        w = max(w, float(np.max(np.abs(r["Xlast_sample"] - rr["Xlast_sample"])) / np.max(np.abs(rr["Xlast_sample"]))))
    return w


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_fused_form_equals_the_literal_loop(name):
    p = wbc.problem(name)
    w = worst(wbc.run(wsb.fused, p, wbc.noise(name)), wbc.reference(name))
    print(f"case {name}: fused against literal, worst relative difference {w:.1e}")
    assert w <= 1e-12


@pytest.mark.parametrize("name", ["A", "B"])
def test_all_fixed_is_the_theta_only_loop(name):
    """Every parameter fixed and p_init = p_true: the theta traces and the last sample of the theta-only literal loop on the
    same H and noise, as identical arrays."""
    p = wbc.problem(name)
    nz = wbc.noise(name)
    npar = wsb.NPAR[p["kind"]]
    for b in range(p["batch"]):
        op = dict(p["ops"][b], fix_p=(True,) * npar, p_init=p["ops"][b]["p_true"], fix_sigma=True)
        eb, r = wsb.literal(p["y"][b], p["model"], p["h"], p["levels"], op, nz[:, b])
        H = p["model"].H_FFT(*op["p_true"])
        eb0, r0 = wsr.sapg_wavelet_literal(p["y"][b], H, p["h"], p["levels"], op, nz[:, b])
        for k in ("thetas", "gXTrace", "logPiTraceX", "mean_thetas", "tol_thetas"):
            np.testing.assert_array_equal(r[k], r0[k], err_msg=k)
        if op["warmup"] > 0:
            np.testing.assert_array_equal(r["logPiTrace_WU"], r0["logPiTrace_WU"])
        np.testing.assert_array_equal(r["Xlast_sample"], r0["Xlast_sample"])
        assert eb["theta"] == eb0 and np.all(r["ps"][:npar] == np.array(op["p_true"])[:, None])
        assert np.all(r["sigmas"] == op["sigma2"]) and eb["sigma2"] == pytest.approx(op["sigma2"], rel=1e-14)


@pytest.mark.parametrize("kind,p", [("gaussian", (0.7, 0.6)), ("moffat", (0.6, 3.5)), ("laplace", (0.2,))])
def test_parameter_gradient_against_a_central_difference(kind, p):
    """G_p = <dB/dp W X, B_p W X - y> / sigma2 is the derivative of f(X; p) = ||y - B_p W X||^2 / (2 sigma2) at a fixed X."""
    import sbtv_oracle as o
    x = wbc.image((64, 64))
    st = o.demo_setup(kind, x, np.random.default_rng(5).standard_normal(x.shape), evMax=1.0, BSNR=30.0)
    h, levels, s2, y, model = wbc.wc.daub(2), 3, st["sigma"] ** 2, st["y"], st["model"]
    X = wr.mrdwt_TI2D(y, h, levels) + np.random.default_rng(6).standard_normal((64, 7 * 64))
    WX = wr.mirdwt_TI2D(X, h, levels)
    f = lambda q: wr._sq(y - model.A(WX, *q)) / (2 * s2)
    for q in range(len(p)):
        hq = 1e-6
        up, dn = list(p), list(p)
        up[q] += hq
        dn[q] -= hq
        fd = (f(up) - f(dn)) / (2 * hq)
        G = wsb.grad_p(model, y, WX, p, q, s2)
        print(f"{kind} parameter {q}: G = {G:.9g}, central difference {fd:.9g}, relative error {abs(G / fd - 1):.1e}")
        assert abs(G - fd) <= 1e-6 * abs(fd)


def test_case_A_visits_the_lower_bound_and_leaves_it():
    p = wbc.problem("A")
    (eb, r), = wbc.reference("A")
    b, lo = r["ps"][0], p["ops"][0]["p_min"][0]
    at = np.flatnonzero(b == lo)
    print(f"b: on p_min at samples {at[0] + 1}..{at[-1] + 1} ({at.size} of them), b(101) = {b[100]:.4g}, b(160) = {b[-1]:.4g}, "
          f"b_EB = {eb['p'][0]:.4g}, theta_EB = {eb['theta']:.4g}")
    assert at.size and np.any(b[at[-1] + 1:] > lo)
    assert r["ps"][1].tolist() == [0.0] * 160 and np.all(r["grads"][1] == 0) and np.all(r["sigmas"] == p["ops"][0]["sigma2"])
    assert np.all(np.isnan(r["tol_ps"][0, 1:19])) and np.all(np.isfinite(r["tol_ps"][0, 20:]))


def test_case_C_visits_the_upper_sigma2_bound_and_leaves_it():
    p = wbc.problem("C")
    (eb, r), = wbc.reference("C")
    s, hi = r["sigmas"], p["ops"][0]["sigma2_max"]
    at = np.flatnonzero(s == hi)
    print(f"sigma2: start {s[0]:.4g}, on sigma2_max = {hi:.4g} at samples {at[0] + 1}..{at[-1] + 1}, sigma2(80) = {s[-1]:.4g}, "
          f"true {p['sigma_true2']:.4g}")
    assert at.size and s[-1] < hi and at[-1] < 79


@pytest.mark.parametrize("name", sorted(wbc.CASES))
def test_gpu_parity_cases_are_not_sensitive_to_their_start(name):
    """A 1e-12 relative perturbation of the start state changes no trace by more than 1e-10 relative over the compared
    length: the rtol 1e-9 of the GPU parity test is then a statement about the arithmetic, not about chaos.  (A longer
    free-sigma2 chain does not meet this, which is why case C stops at 80 samples.)  Every trace is measured entry by entry,
    except `grads`: G_p and G_sigma2 are sums with cancellation that change sign along the chain, and the relative
    condition of an entry next to a zero crossing is unbounded whatever the chain does (entry by entry, cases B and C reach
    1.4e-10 .. 3.2e-10 in single entries of grads while every other trace stays below 2e-11).  Their change is measured
    against the largest |G| of the same row, which is what a perturbation that grows along the chain would also move."""
    p = wbc.problem(name)
    nz = wbc.noise(name)
    x0 = [wr.mrdwt_TI2D(p["y"][b], p["h"], p["levels"]) for b in range(p["batch"])]
    x1 = [x * (1 + 1e-12 * np.random.default_rng(50 + b).standard_normal(x.shape)) for b, x in enumerate(x0)]
    w = worst(wbc.run(wsb.fused, p, nz, xw0=x1), wbc.run(wsb.fused, p, nz, xw0=x0), by_scale=("grads",))
    print(f"case {name}: worst relative change after a 1e-12 perturbation of the start {w:.1e}")
    assert w <= 1e-10


def test_entry_point_declared_exported_bound_and_shimmed():
    import ctypes as C
    import sbtv
    from sbtv import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbtv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+sbtv_SAPG_wavelet_semiblind\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "sbtv_SAPG_wavelet_semiblind is not declared in include/sbtv.h"
    assert len(m.group(1).split(",")) == 26 == len(_lib.SIGNATURES["sbtv_SAPG_wavelet_semiblind"][1])
    assert hasattr(sbtv.load_library(), "sbtv_SAPG_wavelet_semiblind")
    assert callable(sbtv.SAPG_wavelet_semiblind) and "SAPG_wavelet_semiblind" in sbtv.__all__
    s = re.search(r"typedef\s+struct\s+sbtv_sapg_wavelet_sb_opts\s*\{(.*?)\}", text, flags=re.S).group(1)
    names = [re.sub(r"\[\d+\]|\W", "", n) for d in s.split(";") if d.strip()
             for n in re.sub(r"^\s*(unsigned long long|\w+)\s", "", d.strip()).split(",")]
    assert names == [n.rstrip("_") for n, _ in _lib.sbtv_sapg_wavelet_sb_opts._fields_]
    assert C.sizeof(_lib.sbtv_sapg_wavelet_sb_opts) == 224
    shim = open(os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd", "matlab",
                             "sbtv_sapg_wavelet_semiblind.m")).read()
    assert "'sbtv_SAPG_wavelet_semiblind'" in shim and "libstruct('sbtv_sapg_wavelet_sb_opts')" in shim


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chain_kernels_use_no_scratch():
    """wav_sb_update_kernel, and the kernels the three chain drivers share (csrc/wavelet_chain.hip): the step kernel this
    entry launches is the instantiation without moments."""
    rep, chain = _report("wavelet_sapg_sb.hip"), _report("wavelet_chain.hip")
    for r, parts in ((chain, ("wav_step_kernel", "ILb0E")), (rep, ("wav_sb_update_kernel",)), (chain, ("wav_abs_sum_kernel",))):
        k = _find(r, *parts)
        print(parts, k)
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (parts, k)
    assert _find(chain, "wav_step_kernel", "ILb0E")["Occupancy"] >= 4   # a streaming pass: enough waves to hide the loads
