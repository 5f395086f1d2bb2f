"""The wavelet-l1 FISTA problems shared by tests/test_fista_l1_cpu.py and tests/test_gpu_fista_l1.py, built exactly as
tests/wavelet_cases.py builds its own: synth_image(M, N, 4), sbtv_oracle.demo_setup("gaussian", ...), BSNR 30, 7 x 7 Gaussian
taps, tau = sigma^2.  Each reference (the literal restatement, tests/fista_l1_restatement.py) is computed once per session
and never modified."""
import functools
import os

import numpy as np

from conftest import GOLDEN, synth_image

import fista_l1_restatement as fr
import wavelet_cases as wc
import wavelet_restatement as wr

# name: (M, N), filter length, levels, L, stop rule, tolerance, maxiters, start (None or "random")
CASES = {
    # rule 1 fires strictly inside (2, 80), at k = 55: the stop that the host sees one iteration late
    "a": ((64, 64), 2, 4, 1.0, 1, 1e-4, 80, None),
    "b": ((128, 128), 4, 4, 1.0, 2, 3e-3, 40, None),                    # rule 2, stops at k = 28
    "c": ((128, 128), 2, 3, 2.0, 3, 3.049e6, 40, None),                 # rule 3, L != 1, stops at k = 9
    "d": ((100, 90), 2, 3, 1.0, 1, 0.0, 10, None),                      # chirp-z FFT path, runs to maxiters
    # 2 621 440 coefficients: beyond what one grid of the element-wise passes covers (1024 workgroups x 256 lanes x 2)
    "e": ((512, 512), 2, 4, 1.0, 1, 0.0, 5, None),
    "f": ((16, 18), 4, 3, 1.0, 1, 1.1e-3, 40, None),                    # partly filled last workgroup, arbitrary-size FFT
    "g": ((64, 64), 4, 4, 1.0, 1, 0.0, 12, "random"),                   # xw_init
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, H, h, levels, tau, L, true_xw, init, stop, tol, maxiters, p_true) of a case."""
    shape, K, levels, L, stop, tol, maxiters, init = CASES[name]
    if shape == (512, 512):
        x = np.load(os.path.join(GOLDEN, "man_512.npy")).astype(np.float64)
    else:
        x = synth_image(shape[0], shape[1], 4)
    st = wc.setup(x)
    h = wc.daub(K)
    true_xw = wr.mrdwt_TI2D(x, h, levels)
    if init == "random":
        init = np.random.default_rng(21).standard_normal(true_xw.shape)
    return dict(x=x, y=st["y"], H=st["model"].H_FFT(*st["p_true"]), h=h, levels=levels, tau=st["sigma"] ** 2, L=L,
                true_xw=true_xw, init=init, stop=stop, tol=tol, maxiters=maxiters, p_true=st["p_true"])


def _run(fn, p, **kw):
    args = dict(true_xw=p["true_xw"], L=p["L"], xw_init=p["init"])
    args.update(kw)
    return fn(p["y"], p["H"], p["h"], p["levels"], p["tau"], p["stop"], p["tol"], p["maxiters"], **args)


@functools.lru_cache(maxsize=None)
def reference(name):
    """my_fista_l1.m line for line on the case (read-only for its users)."""
    return _run(fr.fista_l1_literal, problem(name))


@functools.lru_cache(maxsize=None)
def operator_form(name):
    """The one-synthesis form on the case (read-only for its users)."""
    return _run(fr.fista_l1_operator, problem(name))


def huge_tau(p):
    """Ten times max|W'B'b|: a threshold above every coefficient, x stays at its zero start."""
    ATb = wr.mrdwt_TI2D(np.real(np.fft.ifft2(np.conj(p["H"]) * np.fft.fft2(p["y"]))), p["h"], p["levels"])
    return 10.0 * float(np.max(np.abs(ATb)))
