"""The analysis-prior wavelet SALSA problems shared by tests/test_analysis_cpu.py and tests/test_gpu_analysis.py, built as
tests/wavelet_cases.py builds its own: synth_image(M, N, 4), sbtv_oracle.demo_setup("gaussian", ...), BSNR 30, 7 x 7 Gaussian
taps, tau = sigma^2, mu = 0.05.  Each reference (the literal restatement, tests/analysis_restatement.py) is computed once per
session and never modified."""
import functools

import numpy as np

from conftest import synth_image

import analysis_restatement as ar
import wavelet_cases as wc
import wavelet_restatement as wr

# name: (M, N), filter length, levels, stop rule, tolA, start (0, 2 or "random"), MAXITERA, and the outer iteration at which the
# literal restatement stops on the CPU (tests/test_analysis_cpu.py asserts it, and that the criterion at that iteration and at
# the one before are each at least 1 % away from tolA)
CASES = {
    "a": ((64, 64), 2, 4, 1, 1e-4, 2, 60, 36),              # rule 1 inside (2, 60): the stop the host sees one iteration late
    "b": ((128, 128), 4, 4, 2, 1.04e-3, 0, 30, 14),         # D4, rule 2 on the image, zero start
    # rule 3: objective(2) is already below tolA, but the rule is not evaluated before outer = 2, where the objective is above
    "c": ((128, 128), 2, 3, 3, 3.1e6, "random", 30, 3),
    "d": ((100, 90), 2, 3, 1, 0.0, 2, 10, 10),              # chirp-z FFT path, runs to MAXITERA
    # 2 621 440 coefficients: beyond what one grid of the element-wise passes covers (1024 workgroups x 256 lanes x 2)
    "e": ((512, 512), 2, 4, 1, 0.0, 2, 4, 4),
    "f": ((16, 18), 2, 3, 1, 1e-3, 2, 40, 5),               # partly filled last workgroup
    "g": ((48, 40), 4, 3, 2, 2e-3, 0, 40, 10),              # D4, rectangular
}
INSIDE = "abcfg"                                            # the cases whose rule fires inside the loop


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, H, h, levels, tau, mu, init, stop, tolA, maxiter, stops_at, p_true) of a case."""
    shape, K, levels, stop, tolA, init, maxiter, stops_at = CASES[name]
    x = synth_image(shape[0], shape[1], 4)
    st = wc.setup(x)
    if init == "random":
        init = np.random.default_rng(21).uniform(0, 255, size=shape)
    return dict(x=x, y=st["y"], H=st["model"].H_FFT(*st["p_true"]), h=wc.daub(K), levels=levels, tau=st["sigma"] ** 2, mu=0.05,
                init=init, stop=stop, tolA=tolA, maxiter=maxiter, stops_at=stops_at, p_true=st["p_true"])


def _run(fn, p, **kw):
    args = dict(true_x=p["x"], stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"], initialization=p["init"])
    args.update(kw)
    return fn(p["y"], p["H"], p["h"], p["levels"], p["tau"], p["mu"], **args)


@functools.lru_cache(maxsize=None)
def reference(name):
    """SALSA_v2.m line for line on the case (read-only for its users)."""
    return _run(ar.salsa_analysis_literal, problem(name))


@functools.lru_cache(maxsize=None)
def operator_form(name):
    """The (s, bu) form on the case (read-only for its users)."""
    return _run(ar.salsa_analysis_operator, problem(name))


def calls(p, n_outer):
    """What the call counter advances by: AT(y), the invLS probe, AT(zeros) for the zero start, the initial A, then invLS and A
    per outer iteration (P and PT are not counted by the reference)."""
    zero_start = not isinstance(p["init"], np.ndarray) and p["init"] == 0
    return 3 + (1 if zero_start else 0) + 2 * n_outer


def huge_tau(p):
    """A tau whose threshold tau / mu is above every soft argument of a run from the zero start, so that u stays zero.  While u
    is zero, bu_k = -W'S_k with S_k = x_1 + ... + x_k, and the argument of the next soft is W'(x_k + S_k).  In the Fourier domain
    S_{k+1} = S_k |H|^2 / (|H|^2 + mu) + B'y / (|H|^2 + mu) grows from 0 towards B'y / mu, and x_{k+1} = (B'y - mu S_k) /
    (|H|^2 + mu) stays below B'y / mu, frequency by frequency; max|W'v| <= ||v||_2 for the Parseval frame.  Hence every argument
    is below 2 ||B'y||_2 / mu; the threshold is five times that."""
    ATy = np.real(np.fft.ifft2(np.conj(p["H"]) * np.fft.fft2(p["y"])))
    return 10.0 * float(np.linalg.norm(ATy))
