"""The theta-estimation problems shared by tests/test_wavelet_sapg_cpu.py and tests/test_gpu_wavelet_sapg.py, built as
tests/wavelet_cases.py builds its own: synth_image, sbtv_oracle.demo_setup("gaussian", ..., BSNR 30, (0.4, 0.3)).  The
constants are those of SALSA/run_deblur_synthesis_L1.m:65-83,143-150: th_init 0.01, bounds 1e-3 .. 1, d_scale 0.1 / th_init,
d_exp 0.8, burnIn 20, Lf = 1 / sigma^2 (evMax = 1), lambda = min(5 / Lf, 2), gamma = 0.98 / (Lf + 1 / lambda).  Each reference
(the literal restatement, tests/wavelet_sapg_restatement.py) is computed once per session and never modified."""
import functools
import math
import os

import numpy as np

from conftest import GOLDEN, synth_image

import wavelet_cases as wc
import wavelet_restatement as wr
import wavelet_sapg_restatement as wsr

# name: (M, N), filter length, levels, samples, warmup, batch, PSF size, noise seed
CASES = {
    "a": ((64, 64), 2, 4, 120, 10, 1, 7, 7),
    "b": ((100, 90), 4, 3, 40, 0, 2, 7, 11),          # chirp-z FFT path, no warm-up, two chains with their own noise
    "c": ((34, 30), 2, 3, 2, 0, 1, 7, 12),            # one step: 7140 coefficients, 14 workgroups, the last one part full
    "d": ((2, 2), 2, 2, 3, 0, 1, 1, 13),              # smallest legal size (one tap: a symmetric 2 x 2 mask leaves a constant)
    "e": ((1024, 1024), 2, 4, 6, 2, 1, 7, 14),        # pipelined row kernel, grid-stride loop over 2048 workgroups
}
BURNIN = 20


def bands(levels):
    return 3 * (levels - 1) + 1


def options(sigma, samples, warmup):
    """op of run_deblur_synthesis_L1.m:65-83,143-150 with evMax = 1."""
    Lf = 1.0 / sigma ** 2
    lam = min(5.0 / Lf, 2.0)
    th_init = 0.01
    return {"samples": samples, "warmup": warmup, "burnIn": min(BURNIN, samples), "th_init": th_init, "min_th": 1e-3,
            "max_th": 1.0, "d_exp": 0.8, "d_scale": 0.1 / th_init, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam),
            "sigma2": sigma ** 2, "sigma": sigma}


def _setup(x, psf_size, seed):
    """wavelet_cases.setup for a PSF of another size than 7 x 7: the data synthesis of sbtv_oracle.demo_setup."""
    if psf_size == 7:
        st = wc.setup(x, seed=seed)
        return st["y"], st["sigma"], st["model"].H_FFT(*st["p_true"])
    import sbtv_oracle as o
    model = o.BlurModel("gaussian", x.shape, psf_size=psf_size)
    Ax = model.A(x, *wc.PSF_PARAMS)
    nrm = float(np.linalg.norm(Ax - np.mean(np.mean(Ax, axis=0)), "fro"))
    sigma = nrm / math.sqrt(x.size * 10 ** (30.0 / 10))
    y = Ax + sigma * np.random.default_rng(seed).standard_normal(x.shape)
    return y, sigma, model.H_FFT(*wc.PSF_PARAMS)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(y (B, M, N), H, h, levels, op, psf_size, batch) of a case; the images of a batch share blur and constants."""
    shape, K, levels, samples, warmup, batch, psf_size, _ = CASES[name]
    ys, sigma, H = [], None, None
    for b in range(batch):
        if shape == (1024, 1024):
            x = np.tile(np.load(os.path.join(GOLDEN, "man_512.npy")).astype(np.float64), (2, 2))
        elif shape == (2, 2):
            x = 255.0 * np.random.default_rng(4).random(shape)       # synth_image clips four pixels to one value
        else:
            x = synth_image(shape[0], shape[1], 4 + 5 * b)
        y, s, H = _setup(x, psf_size, 3 + 3 * b)
        ys.append(y)
        sigma = s if sigma is None else sigma                # one sigma2 per call: that of image 0
    return dict(y=np.stack(ys), H=H, h=wc.daub(K), levels=levels, op=options(sigma, samples, warmup), psf_size=psf_size,
                batch=batch)


def noise(name):
    """(steps, B, M, (3J+1) N) injected normals of a case (case a: default_rng(7)); not cached, case e is 0.5 GB."""
    shape, _, levels, samples, warmup, batch, _, seed = CASES[name]
    steps = max(warmup - 1, 0) + samples - 1
    return np.random.default_rng(seed).standard_normal((steps, batch, shape[0], bands(levels) * shape[1]))


def run(fn, p, nz, samples=None):
    """fn (a restatement) on every chain of problem p with noise nz (steps, B, ...): [(theta_EB, results)] per chain."""
    op = dict(p["op"])
    if samples is not None:
        op["samples"] = samples
    return [fn(p["y"][b], p["H"], p["h"], p["levels"], op, nz[:, b]) for b in range(p["batch"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The literal loop of SAPG_algorithm_1.m on every chain of the case (read-only for its users)."""
    return run(wsr.sapg_wavelet_literal, problem(name), noise(name))
