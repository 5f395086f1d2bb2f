"""The masked-observation wavelet SALSA problems shared by tests/test_masked_analysis_cpu.py and
tests/test_gpu_masked_analysis.py, built as tests/analysis_cases.py builds its own: synth_image(M, N, 4), wavelet_cases.setup
(BSNR 30, 7 x 7 Gaussian taps), tau = sigma^2, mu1 = 0.05.  Each reference (the literal restatement,
tests/masked_analysis_restatement.py) is computed once per session and never modified."""
import functools

import numpy as np

from conftest import synth_image

import masked_analysis_restatement as mar
import wavelet_cases as wc

TAILLE = 7
# name: (M, N), filter length, levels, mask kind, stop rule, tolA, start (0, 2 or "random"), mu2, MAXITERA, and the outer iteration at
# which the literal restatement stops on the CPU (tests/test_masked_analysis_cpu.py asserts it, and that the criterion at that
# iteration and at the one before are each at least 1 % away from tolA)
CASES = {
    "a": ((64, 64), 2, 4, "frame", 1, 1e-4, 2, 0.1, 60, 18),        # rule 1 inside the loop: the stop the host sees one iteration late
    "b": ((128, 128), 4, 4, "frame_holes", 2, 1.46e-2, 0, 1.0, 40, 15),   # D4, rule 2 on the image, zero start
    # rule 3: objective(2) is already below tolA, but the rule is not evaluated before outer = 2, where the objective is above
    "c": ((128, 128), 2, 3, "weights", 3, 3.1294e6, "random", 0.3, 30, 3),     # weighted pixels, y unscaled, a given start image
    "d": ((100, 90), 2, 3, "frame", 1, 0.0, 2, 0.1, 10, 10),         # chirp-z FFT path, runs to MAXITERA
    # 1 048 576 pixels: beyond what one grid of the pixel pass covers (1024 workgroups x 256 lanes x 2)
    "e": ((1024, 1024), 2, 3, "frame", 1, 0.0, 2, 0.1, 3, 3),
    "f": ((16, 18), 2, 3, "frame", 1, 1e-2, 2, 0.1, 40, 15),         # partly filled last workgroup
    "g": ((48, 40), 4, 3, "inpaint", 2, 2e-2, 0, 0.1, 40, 18),       # D4, rectangular; a single unit tap: B = identity, 30 % missing
}
INSIDE = "abcfg"                                            # the cases whose rule fires inside the loop
INPAINT_SIGMA = 2.0                                         # noise of the inpainting case (pixel values in 0..255)


def frame_mask(shape, taille=TAILLE):
    """Ones where the circular blur uses no wrapped pixel (sbtv.valid_mask, restated)."""
    m = np.zeros(shape)
    m[taille - 1:, taille - 1:] = 1.0
    return m


def _mask(kind, shape):
    if kind == "frame":
        return frame_mask(shape)
    if kind == "frame_holes":
        return frame_mask(shape) * (np.random.default_rng(8).random(shape) > 0.3)
    if kind == "weights":
        return np.random.default_rng(7).uniform(0.0, 2.0, shape)
    assert kind == "inpaint"
    return (np.random.default_rng(12).random(shape) > 0.3).astype(np.float64)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, m, H, taps, h, levels, tau, mu1, mu2, init, stop, tolA, maxiter, stops_at, p_true) of a case.  taps: None for
    the 7 x 7 Gaussian of p_true (the library's psf_family builds it), else the array."""
    shape, K, levels, kind, stop, tolA, init, mu2, maxiter, stops_at = CASES[name]
    x = synth_image(shape[0], shape[1], 4)
    m = _mask(kind, shape)
    if kind == "inpaint":
        y = (x + INPAINT_SIGMA * np.random.default_rng(13).standard_normal(shape)) * m
        H, taps, p_true, tau = np.ones(shape, dtype=np.complex128), np.ones((1, 1)), None, INPAINT_SIGMA ** 2
    else:
        st = wc.setup(x)
        # what lies under m = 0 is zeroed (it must not matter); weighted data stay as they are: the solver forms m .* y itself
        y = st["y"] if kind == "weights" else st["y"] * m
        H, taps, p_true, tau = st["model"].H_FFT(*st["p_true"]), None, st["p_true"], st["sigma"] ** 2
    if init == "random":
        init = np.random.default_rng(23).uniform(0, 255, size=shape)
    return dict(x=x, y=y, m=m, H=H, taps=taps, h=wc.daub(K), levels=levels, tau=tau, mu1=0.05, mu2=mu2, init=init, stop=stop,
                tolA=tolA, maxiter=maxiter, stops_at=stops_at, p_true=p_true)


def run(fn, p, **kw):
    args = dict(true_x=p["x"], stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"], initialization=p["init"])
    args.update(kw)
    return fn(p["y"], p["m"], p["H"], p["h"], p["levels"], p["tau"], p["mu1"], p["mu2"], **args)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The literal iteration on the case (read-only for its users)."""
    return run(mar.salsa_masked_analysis_literal, problem(name))


@functools.lru_cache(maxsize=None)
def state_form(name):
    """The (s, bu) / (v, bv) form on the case (read-only for its users)."""
    return run(mar.salsa_masked_analysis_state, problem(name))


def calls(p, n_outer):
    return mar.calls(p, n_outer)


@functools.lru_cache(maxsize=None)
def property_problem():
    """The problem of the property the entry exists for: the `man` crop man512[100:356, 60:316] blurred circularly (7 x 7 Gaussian
    PSF w = (0.4, 0.3), BSNR 30 dB, noise default_rng(3)), observed on the 250 x 250 part without wrapped pixels.  y_obs: that
    observation, (y, m): it embedded in the 256 x 256 domain (sbtv.embed_observation, restated), H / H_obs: the spectra of the
    taps at the two sizes.  Haar, levels 4, tau = 0.3 sigma^2, mu1 = 0.05, mu2 = 0.1, rule 1 with tolA 1e-5, at most 300
    iterations, zero start."""
    import os

    import sbtv_oracle as o
    from conftest import GOLDEN
    scene = np.load(os.path.join(GOLDEN, "man_512.npy")).astype(np.float64)[100:356, 60:316]
    st = wc.setup(scene, seed=3)
    t = TAILLE
    y_obs = st["y"][t - 1:, t - 1:]
    y, m = np.zeros(scene.shape), frame_mask(scene.shape)
    y[t - 1:, t - 1:] = y_obs
    taps = o.Gaussian_psf(t, *st["p_true"])
    return dict(scene=scene, y_obs=y_obs, y=y, m=m, H=st["model"].H_FFT(*st["p_true"]), H_obs=o.resize(taps, y_obs.shape),
                h=wc.daub(2), levels=4, tau=0.3 * st["sigma"] ** 2, mu1=0.05, mu2=0.1, stop=1, tolA=1e-5, maxiter=300,
                p_true=st["p_true"])


def psnr_over(mask, x_true, x):
    """PSNR (peak 255) over the pixels where mask is non-zero (tests/masked_restatement.py)."""
    sel = np.asarray(mask) > 0
    return 10.0 * np.log10(255.0 ** 2 / float(np.mean((x_true[sel] - x[sel]) ** 2)))
