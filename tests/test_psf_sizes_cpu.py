"""CPU: the PSF builders at every mask size 1..15 and with a rotated Gaussian, and the proof that the cases of
tests/psf_size_cases.py (run on the GPU by tests/test_gpu_psf_sizes.py) are good cases: their PSF parameters move at every
iteration, never touch a bound, and their traces do not amplify a last-bit perturbation of the data to anywhere near the bars
they are compared at.  No GPU: sbtv_psf_taps and sbtv_err_psf are host arithmetic."""
import numpy as np
import pytest

import psf_size_cases as pc

KINDS = ("gaussian", "moffat", "laplace")
PARAMS = {"gaussian": [(0.4, 0.3), (0.7, 0.2), (0.55, 0.45)], "moffat": [(0.4, 3.5), (0.6, 5.0)], "laplace": [(0.3,), (0.2,)]}
PHIS = (0.0, 0.3, 0.6, -1.1)


@pytest.mark.parametrize("t", range(1, 16))
def test_host_builder_matches_the_oracle_at_every_size(t):
    """sbtv.psf_family against sbtv_oracle.PSF_TAPS at the bars of tests/test_abi.py::test_psf_taps_match_oracle."""
    import sbtv
    import sbtv_oracle as o
    for kind in KINDS:
        for p in PARAMS[kind]:
            for phi in (PHIS if kind == "gaussian" else (None,)):
                pp = p if phi is None else p + (phi,)
                taps, d = sbtv.psf_family(kind, t, pp)
                ref, dref = o.PSF_TAPS[kind]
                assert taps.shape == (t, t)
                np.testing.assert_allclose(taps, ref(t, pp), rtol=1e-14, atol=1e-17, err_msg=f"{kind} {t} {pp}")
                assert len(d) == len(dref)
                for q, (a, fn) in enumerate(zip(d, dref)):
                    np.testing.assert_allclose(a, fn(t, pp), rtol=1e-12, atol=1e-16, err_msg=f"{kind} {t} {pp} d{q}")


def test_blur_model_hands_phi_to_the_gaussian_only():
    import sbtv_oracle as o
    m = o.BlurModel("gaussian", (16, 12), psf_size=5, phi=0.6)
    np.testing.assert_array_equal(m.taps(0.7, 0.2), o.Gaussian_psf(5, 0.7, 0.2, 0.6))
    np.testing.assert_array_equal(m.dtaps(0, 0.7, 0.2), o.diff_gaus_w1_taps(5, 0.7, 0.2, 0.6))
    np.testing.assert_array_equal(m.dtaps(1, 0.7, 0.2), o.diff_gaus_w2_taps(5, 0.7, 0.2, 0.6))
    assert np.max(np.abs(m.taps(0.7, 0.2) - o.Gaussian_psf(5, 0.7, 0.2))) > 1e-3        # the rotation is not a no-op
    np.testing.assert_array_equal(o.BlurModel("gaussian", (16, 12), 5).taps(0.7, 0.2), o.Gaussian_psf(5, 0.7, 0.2))
    for kind, p in (("moffat", (0.4, 3.5)), ("laplace", (0.3,))):
        np.testing.assert_array_equal(o.BlurModel(kind, (16, 12), 5, phi=0.6).taps(*p), o.BlurModel(kind, (16, 12), 5).taps(*p))


@pytest.mark.parametrize("kind,t,phi", [("gaussian", 3, 0.0), ("gaussian", 8, 0.6), ("gaussian", 15, 0.6), ("moffat", 3, 0.0),
                                        ("moffat", 8, 0.0), ("moffat", 15, 0.0), ("laplace", 3, 0.0), ("laplace", 8, 0.0),
                                        ("laplace", 15, 0.0)])
def test_host_err_psf_at_other_sizes_matches_the_oracle(kind, t, phi):
    """sbtv.sapg._err_psf against sbtv_oracle.err_psf_trace at the bars of
    tests/test_abi.py::test_err_psf_host_entry_matches_oracle."""
    import sbtv_oracle as o
    from sbtv.sapg import _err_psf
    rng = np.random.default_rng(3)
    n = 24
    lo, hi = {"gaussian": (0.1, 1.0), "moffat": (0.05, 8.0), "laplace": (0.05, 1.0)}[kind]
    npar = 1 if kind == "laplace" else 2
    ps = rng.uniform(lo, hi, (npar, n))
    ps[:, 5] = ps[:, 4]
    p_true = o.DEMO[kind]["true"]
    got = _err_psf(kind, t, ps, p_true, phi)
    ref = o.err_psf_trace(kind, ps, p_true, t, phi)
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-20)
    assert np.all(ref[1:] > 0)
    if kind == "moffat":
        assert got[0] == 0.0
    if phi:
        assert not np.allclose(ref, o.err_psf_trace(kind, ps, p_true, t), rtol=1e-3)      # phi reaches both PSFs


@pytest.mark.parametrize("t", [3, 8, 9, 15])
@pytest.mark.parametrize("kind,q,p", [("gaussian", 0, (0.55, 0.45, 0.6)), ("gaussian", 1, (0.55, 0.45, 0.6)),
                                      ("gaussian", 0, (0.4, 0.3, 0.6)), ("gaussian", 1, (0.4, 0.3, 0.6)),
                                      ("laplace", 0, (0.2,)), ("laplace", 0, (0.3,)), ("moffat", 1, (0.6, 5.0)),
                                      ("moffat", 1, (0.4, 3.5)), ("moffat", 0, (0.6, 5.0)), ("moffat", 0, (0.4, 3.5))])
def test_oracle_derivative_taps_are_the_derivatives_of_its_taps(kind, q, p, t):
    """Central difference of the normalised taps, step h = 1e-6 p, against the oracle's derivative taps to 1e-7 max|d|: the
    truncation term h^2 f''' / 6 is 1e-12 p^2 f''', the rounding term 1.1e-16 max(f) / h at most 1e-9 of the taps.  Moffat
    alpha: utils/diff_moffat_alpha.m is HALF the derivative of psf_moffat.m (csrc/wavelet_sapg_sb.hip, `g0_scale`), in
    every tap and in the sum, so also after the quotient rule: the difference quotient is twice the oracle's taps."""
    import sbtv_oracle as o
    taps, dtaps = o.PSF_TAPS[kind]
    h = 1e-6 * p[q]
    up, dn = list(p), list(p)
    up[q] += h
    dn[q] -= h
    fd = (taps(t, tuple(up)) - taps(t, tuple(dn))) / (up[q] - dn[q])
    d = dtaps[q](t, p) * (2.0 if (kind == "moffat" and q == 0) else 1.0)
    assert np.max(np.abs(d)) > 1e-6
    assert np.max(np.abs(fd - d)) <= 1e-7 * np.max(np.abs(d))


def _strictly_inside_and_moving(ps, pmin, pmax, label):
    for q in range(len(pmin)):
        tr = np.asarray(ps[q], dtype=np.float64)
        assert np.all((tr > pmin[q]) & (tr < pmax[q])), f"{label}: parameter {q} touches a bound: {tr}"
        move = np.abs(np.diff(tr)) / np.abs(tr[:-1])
        assert np.all(move >= 1e-4), f"{label}: parameter {q} moves by {move.min():.1e} relative in one iteration"


@pytest.mark.parametrize("name", sorted(pc.TV_CASES))
def test_tv_case_is_a_good_case(name):
    """(1) every free PSF parameter strictly inside (pmin, pmax) at every iteration, (2) moving by 1e-4 relative or more at
    every iteration, (3) every trace finite, (4) the reference on y (1 + 1e-15 r) agrees with the reference on y 100 times
    more tightly than the GPU bar of every compared trace."""
    import sbtv_oracle as o
    p, ref = pc.tv_problem(name), pc.tv_reference(name)
    d = o.DEMO[p["kind"]]
    assert len(ref) == p["chains"]
    for b, r in enumerate(ref):
        _strictly_inside_and_moving(r["ps"], d["pmin"], d["pmax"], f"{name} chain {b}")
        for key, _, _ in pc.TV_BARS:
            if key in r:
                assert np.all(np.isfinite(np.asarray(r[key], dtype=np.float64)[..., 1:] if key == "logPiTrace_WU" else r[key])), key
    for b, (g, r) in enumerate(zip(pc.tv_reference(name, True), ref)):
        worst = pc.tv_compare(g, r, tighten=100.0, label=f"{name} chain {b} perturbed", shared=p["shared"])
        print(f"{name} chain {b}: worst fraction of bar / 100: " + ", ".join(f"{k} {f:.1e}" for k, (_, f) in worst.items()))
    if p["chains"] > 1 and not p["shared"]:
        last = [tuple(r["ps"][:, -1]) for r in ref]
        assert len(set(last)) == p["chains"]                  # every chain has its own parameters, hence its own taps


WAV_KEYS = ("thetas", "ps", "sigmas", "grads", "gXTrace", "logPiTraceX", "mean_thetas", "tol_thetas", "mean_ps", "tol_ps")


def wav_compare(got, ref, rtol):
    """The numerical bars of tests/test_gpu_wavelet_sb.py::_check at `rtol`."""
    for (eb, r), (eb_ref, rr) in zip(got, ref):
        for k in WAV_KEYS:
            a, c = np.asarray(r[k], dtype=np.float64), np.asarray(rr[k], dtype=np.float64)
            fin = np.isfinite(c)
            np.testing.assert_array_equal(np.isnan(a), np.isnan(c), err_msg=k)
            if k.startswith("tol_"):
                small = fin & (np.abs(c) < 1e-9)
                assert np.all(np.abs(a[small] - c[small]) <= 1e-12 * (rtol / pc.WAV_RTOL)), k
                fin = fin & ~small
            np.testing.assert_allclose(a[fin], c[fin], rtol=rtol, atol=0, err_msg=k)
        assert abs(eb["theta"] - eb_ref["theta"]) <= rtol * eb_ref["theta"]
        assert abs(eb["sigma2"] - eb_ref["sigma2"]) <= rtol * eb_ref["sigma2"]
        np.testing.assert_allclose(eb["p"], eb_ref["p"], rtol=rtol, atol=0)
        xs = float(np.max(np.abs(rr["Xlast_sample"])))
        assert float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - rr["Xlast_sample"]))) <= rtol * xs


@pytest.mark.parametrize("name", sorted(pc.WAV_CASES))
def test_wavelet_case_is_a_good_case(name):
    """The four conditions of test_tv_case_is_a_good_case for the semi-blind wavelet cases (bar: rtol 1e-9 on every trace)."""
    p, ref = pc.wav_problem(name), pc.wav_reference(name)
    op = p["ops"][0]
    npar = len(op["p_min"])
    for b, (eb, r) in enumerate(ref):
        _strictly_inside_and_moving(r["ps"][:npar], op["p_min"], op["p_max"], f"{name} chain {b}")
        for k in ("thetas", "ps", "sigmas", "grads", "gXTrace", "logPiTraceX", "mean_thetas", "mean_ps", "Xlast_sample"):
            assert np.all(np.isfinite(r[k])), k
        assert np.all(np.isfinite(r["tol_thetas"][p["ops"][b]["burnIn"]:]))      # NaN while the window is empty, as specified
    wav_compare(pc.wav_reference(name, True), ref, pc.WAV_RTOL / 100.0)
    if p["batch"] > 1:
        assert ref[0][1]["ps"][0, -1] != ref[1][1]["ps"][0, -1]
