"""The SK-ROCK runs on the TV posterior shared by tests/test_skrock_tv_cpu.py and tests/test_gpu_skrock_tv.py.  A problem is
that of test_plain_myula_chain_matches_oracle: demo_setup("gaussian", synth_image, noise, evMax = 0.99), theta = 0.02,
chambolleit = 25; the step is delta = 0.8 max_step(stages, eta, sigma2, lambda) (||A|| = 1: a normalised non-negative PSF).
Each reference (tests/skrock_tv_restatement.py) is computed once per session and never modified.

No case may sit on the edge of the Chambolle stop rule (tests/test_skrock_tv_cpu.py checks it): should one, change its SEED."""
import functools

import numpy as np

from conftest import synth_image

import sbtv_oracle as o
import skrock_tv_restatement as skr

ETA, THETA, CHAMBOLLEIT = 0.05, 0.02, 25

# name -> (M, N, stages, steps, seed): s = 2 has no middle stage; s = 3 is odd (the sample and P_next swap buffers); 24 x 40 is
# rectangular and takes the chirp-z path
CASES = {"sq-s2": (32, 32, 2, 4, 8), "sq-s3": (32, 32, 3, 4, 8), "sq-s10": (32, 32, 10, 3, 8), "rect-s5": (24, 40, 5, 3, 9)}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def build(M, N, stages, steps, seed, chambolleit=CHAMBOLLEIT):
    """The problem of an explicit case (tests/tv_sampler_geometry_cases.py has further ones):
    dict(y, model, p (PSF parameters), sigma2, lambda, noise (steps, M, N), op, theta)."""
    rng = np.random.default_rng(seed)
    st = o.demo_setup("gaussian", synth_image(M, N, 21), rng.standard_normal((M, N)), evMax=0.99)
    s2, lam = st["sigma"] ** 2, st["lam"]
    op = {"samples": steps + 1, "stages": stages, "lambda": lam, "delta": 0.8 * skr.max_step(stages, ETA, s2, lam),
          "eta": ETA, "chambolleit": chambolleit}
    return dict(y=st["y"], model=st["model"], p=st["p_true"], sigma2=s2, noise=rng.standard_normal((steps, M, N)), op=op,
                theta=THETA, **{"lambda": lam})


def problem(name):
    return build(*CASES[name])


def chain_of(q, noise=None, theta=None, sigma2=None, **kw):
    """The restatement on a problem (its own noise, theta and sigma2 unless given)."""
    return skr.skrock_tv_chain(q["y"], q["model"], q["p"], q["op"], q["theta"] if theta is None else theta,
                               q["sigma2"] if sigma2 is None else sigma2, q["noise"] if noise is None else noise, **kw)


def chain(name, **kw):
    return chain_of(problem(name), **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement on the case's injected normals (read-only for its users)."""
    return chain(name)
