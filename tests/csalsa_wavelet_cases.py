"""The problems of C-SALSA with the wavelet analysis prior shared by tests/test_csalsa_wavelet_cpu.py and
tests/test_gpu_csalsa_wavelet.py, built as tests/analysis_cases.py builds its own: synth_image(M, N, 4), wavelet_cases.setup
(sbtv_oracle.demo_setup("gaussian", ...), BSNR 30), 7 x 7 Gaussian taps, sigma from the set-up.  Each reference (the literal
restatement, tests/csalsa_wavelet_restatement.py, with phi = ||W' .||_1) is computed once per session and never modified."""
import functools

import numpy as np

from conftest import synth_image

import csalsa_wavelet_restatement as cr
import wavelet_cases as wc

# name: (M, N), filter length, levels, mu1, mu2, stop rule, tolA, start (0, 2 or "random"), MAXITERA, EPSILON as a multiple of the
# default sqrt(n + 8 sqrt n) sigma (1: the default itself, passed as 0), CONTINUATIONFACTOR, the form the library runs
# ("spectral" or "image"), and the outer iteration at which the literal restatement stops on the CPU.
# tests/test_csalsa_wavelet_cpu.py asserts that iteration and the margins: for the cases of INSIDE the rule's value is at least
# 1 % away from tolA and criterion / epsilon at least 1e-3 away from 1, both at the stopping iteration and at the one before; for
# every iteration of every case ||ve|| / epsilon is at least 1e-3 away from 1, so the projection cannot change its branch.
CASES = {
    # the lagged stop inside the loop: criterion / epsilon 0.9924 at 23; rule value 5.3e-4, 4.0e-3 the iteration before
    "a": ((64, 64), 2, 4, 1.0, 1.0, 3, 1e-3, 0, 60, 1.0, 1.0, "spectral", 23),
    "b": ((128, 128), 4, 4, 2.0, 1.0, 1, 1e-3, 0, 60, 1.0, 1.0, "spectral", 27),      # rule 1 on the objective ||W'x||_1
    "c": ((128, 128), 2, 3, 1.0, 1.0, 2, 2e-3, "random", 60, 1.0, 1.0, "spectral", 17),   # rule 2 on the image, given start
    "d": ((100, 90), 2, 3, 1.0, 1.0, 3, 0.0, 2, 10, 1.0, 1.0, "image", 10),           # chirp-z plan: the image form
    "e": ((512, 512), 2, 4, 1.0, 1.0, 3, 0.0, 2, 4, 1.0, 1.0, "spectral", 4),         # 2.6 M coefficients: the grid-stride loop
    "f": ((16, 18), 2, 3, 1.0, 1.0, 3, 0.0, 2, 12, 1.0, 1.0, "image", 12),            # partly filled last workgroup
    # the CONSTRAINT decides: the rule's value is below tolA from 36 on, criterion / epsilon 1.0015 at 36 and 0.9980 at 37
    "g": ((48, 40), 4, 3, 2.0, 1.0, 2, 2e-3, 0, 80, 1.0, 1.0, "image", 37),
    "h": ((64, 64), 2, 4, 0.4, 0.7, 3, 0.0, 2, 12, 1.0, 1.0, "spectral", 12),         # mu2 != 1
    # a wide ball: ||ve|| <= epsilon in many iterations, both branches of the projection
    "i": ((64, 64), 2, 4, 1.0, 1.0, 3, 1e-3, 2, 60, 30.0, 1.0, "spectral", 29),
    "j": ((64, 64), 2, 4, 0.7, 0.7, 3, 0.0, 0, 12, 1.0, 1.03, "image", 12),           # continuation: the threshold changes
}
INSIDE = "abcgi"                                            # the cases whose rule fires inside the loop


def library_form(shape, delta):
    """The form sbtv_CSALSA_wavelet runs by default: the spectral one needs fixed mu1 / mu2 and the power-of-two FFT plan (both
    sizes powers of two, at least 16); every other size takes the chirp-z plan, which has no OP_CSALSA row pass."""
    pow2 = all(n >= 16 and n & (n - 1) == 0 for n in shape)
    return "spectral" if pow2 and delta == 1.0 else "image"


def default_epsilon(n, sigma):
    return float(np.sqrt(n + 8 * np.sqrt(n)) * sigma)                    # CSALSA_v2.m:413


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, H, h, levels, mu1, mu2, sigma, stop, tolA, init, maxiter, epsilon (0: the default), eps (its value), delta,
    form, stops_at, p_true) of a case."""
    shape, K, levels, mu1, mu2, stop, tolA, init, maxiter, epsf, delta, form, stops_at = CASES[name]
    x = synth_image(shape[0], shape[1], 4)
    st = wc.setup(x)
    if init == "random":
        init = np.random.default_rng(21).uniform(0, 255, size=shape)
    eps0 = default_epsilon(x.size, st["sigma"])
    return dict(x=x, y=st["y"], H=st["model"].H_FFT(*st["p_true"]), h=wc.daub(K), levels=levels, mu1=mu1, mu2=mu2,
                sigma=st["sigma"], stop=stop, tolA=tolA, init=init, maxiter=maxiter, epsilon=0.0 if epsf == 1.0 else epsf * eps0,
                eps=epsf * eps0, delta=delta, form=form, stops_at=stops_at, p_true=st["p_true"])


def _args(p, **kw):
    args = dict(true_x=p["x"], stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"], initialization=p["init"],
                continuationfactor=p["delta"], epsilon=p["epsilon"])
    args.update(kw)
    return args


@functools.lru_cache(maxsize=None)
def reference(name):
    """CSALSA_v2.m line for line on the case, with the wavelet handles (read-only for its users)."""
    p = problem(name)
    return cr.csalsa_wavelet_literal(p["y"], **cr.wavelet_handles(p["H"], p["h"], p["levels"]), mu1=p["mu1"], mu2=p["mu2"],
                                     sigma=p["sigma"], **_args(p))


@functools.lru_cache(maxsize=None)
def state_form(name):
    """The (s, bu, E, s_) form, or the image form where the library runs that, on the case (read-only for its users)."""
    p = problem(name)
    return cr.csalsa_wavelet_state(p["y"], p["H"], p["h"], p["levels"], p["mu1"], p["mu2"], p["sigma"], form=p["form"], **_args(p))


def calls(p, n_outer):
    """What the call counter advances by, as csalsa_one counts: AT(y), the invLS probe, AT(zeros) for the zero start, A twice
    before the loop, then AT, invLS and A per iteration outer = 2..n_outer (P and PT are not counted by the reference)."""
    zero_start = not isinstance(p["init"], np.ndarray) and p["init"] == 0
    return 4 + (1 if zero_start else 0) + 3 * (n_outer - 1)


def feasible(p, x):
    """||B x - y|| / epsilon of an image x, from x alone."""
    Bx = np.real(np.fft.ifft2(p["H"] * np.fft.fft2(np.asarray(x, dtype=np.float64))))
    return float(np.linalg.norm((Bx - p["y"]).ravel())) / p["eps"]
