"""The fixed-theta problems shared by tests/test_wavelet_posterior_cpu.py and tests/test_gpu_wavelet_posterior.py.  Data,
blur and constants come from tests/wavelet_sapg_cases.py (its `problem` where a case of that file has the geometry, its
`_setup` / `options` otherwise).  Each reference (tests/wavelet_myula_restatement.py) is computed once per session and never
modified."""
import functools

import numpy as np

from conftest import synth_image

import wavelet_cases as wc
import wavelet_myula_restatement as wmr
import wavelet_sapg_cases as wsc

# name: problem of wavelet_sapg_cases or ((M, N), filter length, levels), samples, theta per chain, sigma2 factor per chain,
# noise seed
CASES = {
    "a": ("a", 24, (0.03,), (1.0,), 21),                      # 64 x 64 Haar, levels 4
    "b": ("b", 10, (0.02, 0.05), (1.0, 1.5), 22),             # 100 x 90 D4, levels 3: chirp-z, tiles cut at both edges,
                                                              # two chains with their own theta, sigma2 and noise
    "c": (((66, 18), 2, 2), 6, (0.03,), (1.0,), 23),          # J = 1; second tiles of two rows / two columns
    "d": ("d", 3, (0.03,), (1.0,), 24),                       # 2 x 2, levels 2
    "e": (((512, 256), 2, 4), 4, (0.03,), (1.0,), 25),        # dimX / 2 > 2048 workgroups x 256 lanes: grid-stride loop
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(y (B, M, N), H, h, levels, op (samples, lambda, gamma, sigma2, ...), theta (B,), sigma2 (B,), psf_size, batch)."""
    src, samples, theta, s2f, _ = CASES[name]
    if isinstance(src, str):
        p = dict(wsc.problem(src))
    else:
        shape, K, levels = src
        y, sigma, H = wsc._setup(synth_image(shape[0], shape[1], 4), 7, 3)
        p = dict(y=y[None], H=H, h=wc.daub(K), levels=levels, op=wsc.options(sigma, samples, 0), psf_size=7, batch=1)
    p["op"] = dict(p["op"], samples=samples)
    p["theta"] = np.array(theta)
    p["sigma2"] = p["op"]["sigma2"] * np.array(s2f)
    assert p["batch"] == len(theta)
    return p


def noise(name, samples=None):
    """(samples-1, B, M, (3J+1) N) injected normals of a case."""
    p = problem(name)
    S = p["op"]["samples"] if samples is None else samples
    B, M, N = p["y"].shape
    return np.random.default_rng(CASES[name][4]).standard_normal((S - 1, B, M, wsc.bands(p["levels"]) * N))


def chain(p, b, nz, samples=None, theta=None):
    """The restatement on chain b of problem p with noise nz (steps, M, (3J+1) N)."""
    op = dict(p["op"]) if samples is None else dict(p["op"], samples=samples)
    return wmr.myula_wavelet_chain(p["y"][b], p["H"], p["h"], p["levels"], op, float(p["theta"][b] if theta is None else theta),
                                   float(p["sigma2"][b]), nz)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement on every chain of the case (read-only for its users)."""
    p, nz = problem(name), noise(name)
    return [chain(p, b, nz[:, b]) for b in range(p["batch"])]
