"""The wavelet-l1 solver problems shared by tests/test_wavelet_cpu.py and tests/test_gpu_wavelet.py: built with synth_image,
sbtv_oracle.demo_setup("gaussian", ...), BSNR 30 and 7 x 7 taps as tests/test_gpu_masked.py builds its problems.  Each
reference (the literal restatement, tests/wavelet_restatement.py) is computed once per session and never modified."""
import functools
import os

import numpy as np

from conftest import GOLDEN, synth_image

import wavelet_restatement as wr

PSF_PARAMS = (0.4, 0.3)
# name: (M, N), filter length, levels, stop rule, tolA, initialization (0, 2 or "random"), MAXITERA, tau / sigma^2, mu
SOLVER_CASES = {
    # the stop rule fires strictly inside (2, 60): the restatement stops at outer iteration 26 (confirmed on the CPU,
    # tests/test_wavelet_cpu.py asserts it), so the rule that the host evaluates one iteration late is exercised
    "a": ((64, 64), 2, 4, 1, 1e-4, 2, 60, 1.0, 0.05),
    "b": ((128, 128), 4, 4, 2, 0.0, 0, 30, 1.0, 0.05),
    "c": ((128, 128), 2, 3, 3, 0.0, "random", 30, 1.0, 0.05),
    "d": ((100, 90), 2, 3, 1, 0.0, 2, 10, 1.0, 0.05),                   # chirp-z FFT path
    "e": ((1024, 1024), 2, 4, 1, 0.0, 2, 6, 1.0, 0.05),                 # pipelined row kernel
}


def daub(K):
    """Scaling filters for the restatement without the library: Haar and D4 in closed form."""
    return wr.daub_closed_form(K)


def setup(x, seed=3):
    import sbtv_oracle as o
    rng = np.random.default_rng(seed)
    return o.demo_setup("gaussian", x, rng.standard_normal(x.shape), evMax=1.0, BSNR=30.0, true_params=PSF_PARAMS)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, H, h, levels, tau, mu, true_xw, init, stop, tolA, maxiter, st) of a solver case."""
    shape, K, levels, stop, tolA, init, maxiter, tauf, mu = SOLVER_CASES[name]
    if shape == (1024, 1024):
        x = np.tile(np.load(os.path.join(GOLDEN, "man_512.npy")).astype(np.float64), (2, 2))
    else:
        x = synth_image(shape[0], shape[1], 4)
    st = setup(x)
    h = daub(K)
    true_xw = wr.mrdwt_TI2D(x, h, levels)
    if init == "random":
        init = np.random.default_rng(21).standard_normal(true_xw.shape)
    return dict(x=x, y=st["y"], H=st["model"].H_FFT(*st["p_true"]), h=h, levels=levels, tau=tauf * st["sigma"] ** 2, mu=mu,
                true_xw=true_xw, init=init, stop=stop, tolA=tolA, maxiter=maxiter, p_true=st["p_true"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The literal SALSA_v2 iteration on the case (read-only for its users)."""
    p = problem(name)
    return wr.salsa_wavelet_literal(p["y"], p["H"], p["h"], p["levels"], p["tau"], p["mu"], true_xw=p["true_xw"],
                                    stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"], initialization=p["init"])
