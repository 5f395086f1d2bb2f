"""The masked-observation SAPG / MYULA runs shared by tests/test_masked_sapg_cpu.py and tests/test_gpu_sapg_masked.py.  The
protocol is that of tests/sapg_skrock_cases.py: demo_setup(kind, synth_image(M, N, 7), noise of seed 11, evMax = 0.99),
chambolleit = 25, samples 12, warmup 4, burnIn 8, the demo's c_theta, c_p and c_sigma each multiplied by 0.02 (at the
reference's own scales a 32 x 32 chain throws theta and sigma2 against their clamps within two iterations).  The observation is
the demo's y; the mask is the case's.  The 8 x 6 case cannot hold the demo's 7 x 7 PSF: its data are synthesised by the demo's
formulas with its own 3 x 3 PSF.
Each reference (tests/masked_sapg_restatement.py) is computed once per session and never modified.

No case may sit on the edge of the Chambolle stop rule (tests/test_masked_sapg_cpu.py checks it): should one, change its SEED."""
import functools
import math

import numpy as np

from conftest import synth_image

import sbtv_oracle as o
import masked_sapg_restatement as msr

CHAMBOLLEIT, SCALE = 25, 0.02
SAMPLES, WARMUP, BURNIN = 12, 4, 8
NAMES_OF = {"gaussian": ("w1", "w2"), "moffat": ("alpha", "beta"), "laplace": ("b",)}


def valid_mask(shape, taille):
    """Ones where row >= taille-1 and column >= taille-1 (sbtv.valid_mask, restated)."""
    m = np.zeros(shape)
    m[taille - 1:, taille - 1:] = 1.0
    return m


def _holes(shape, seed):
    return (np.random.default_rng(seed).random(shape) >= 0.3).astype(np.float64)


def _weights(shape, seed):
    return np.random.default_rng(seed).choice([0.0, 0.5, 1.0], size=shape)


def _zero_row(shape, row):
    m = np.ones(shape)
    m[row, :] = 0.0
    return m


# name -> dict(kind, M, N, seed, mask: shape -> mask[, psf_size, fix])
CASES = {
    # three derivative passes, tuned power-of-two FFT
    "gauss-valid": dict(kind="gaussian", M=32, N=32, seed=11, fix=(False, False), mask=lambda s: valid_mask(s, 7)),
    "moffat-holes": dict(kind="moffat", M=32, N=32, seed=11, mask=lambda s: _holes(s, 21)),            # scattered zeros
    # one PSF parameter, weights, n_obs != sum(m)
    "laplace-weights": dict(kind="laplace", M=32, N=32, seed=11, mask=lambda s: _weights(s, 22)),
    # chirp-z path, tvnorm_partials path, tail workgroup
    "moffat-rect": dict(kind="moffat", M=24, N=40, seed=11, mask=lambda s: valid_mask(s, 7)),
    "laplace-9x9": dict(kind="laplace", M=32, N=32, seed=11, psf_size=9, mask=lambda s: valid_mask(s, 9)),   # taps path above 8 x 8
    # r reused as the gradient's input, no spectra rebuilt, sigma2 free
    "gauss-fixed": dict(kind="gaussian", M=32, N=32, seed=11, fix=(True, True), mask=lambda s: valid_mask(s, 7)),
    "tiny": dict(kind="laplace", M=8, N=6, seed=11, psf_size=3, mask=lambda s: _zero_row(s, 2)),      # fewer pixels than one workgroup
}
NAMES = list(CASES)


def _setup(kind, x, noise, evMax, taille):
    """o.demo_setup; where its 7 x 7 PSF does not fit the image, the same formulas (run_laplace_demo.m:109-142) with a PSF of
    `taille`."""
    if min(x.shape) >= 7:
        return o.demo_setup(kind, x, noise, evMax=evMax)
    d = o.DEMO[kind]
    p_true = tuple(d["true"])
    model = o.BlurModel(kind, x.shape, psf_size=taille)
    dimX, BSNR, th_init = x.size, 30.0, 0.01
    Ax = model.A(x, *p_true)
    nrm = float(np.linalg.norm(Ax - np.mean(np.mean(Ax, axis=0)), "fro"))
    sig = lambda bsnr: nrm / math.sqrt(dimX * 10 ** (bsnr / 10))
    sigma, smin, smax = sig(BSNR), sig(d["bsnr_min"]), sig(d["bsnr_max"])
    lf = lambda s2: evMax ** 2 / s2
    Lf = (min if d["lf"] == "min" else max)(lf(smin ** 2), lf(smax ** 2))
    lam = min(5 / Lf, d["lambdaMax"])
    gamma = d["gamma_mult"] * d["gammaFrac"] * (1 / (Lf + 1 / lam))
    return dict(kind=kind, model=model, y=Ax + sigma * noise, x=x, sigma=sigma, sigma_min=smin ** 2, sigma_max=smax ** 2,
                sigma_init=(smin ** 2 + smax ** 2) / 2, Lf=Lf, lam=lam, gamma=gamma, p_true=p_true, th_init=th_init, dimX=dimX,
                d_exp=0.8, d_scale=0.01 / th_init, min_th=1e-3, max_th=1.0)


def problem(name, samples=SAMPLES, warmup=WARMUP, burnIn=BURNIN):
    return build(tuple(sorted(CASES[name].items())), samples, warmup, burnIn)


@functools.lru_cache(maxsize=None)
def build(case, samples=SAMPLES, warmup=WARMUP, burnIn=BURNIN):
    """The problem of an explicit case, given as its sorted items (tests/tv_sampler_geometry_cases.py has further ones; a case
    may name its own chambolleit): dict(setup, model, kind, mask, noise (steps, M, N), kw: what the restatement takes beyond
    setup / mask / noise, op, c: what sbtv.SAPG_masked takes)."""
    q = dict(case)
    cit = q.get("chambolleit", CHAMBOLLEIT)
    kind, M, N = q["kind"], q["M"], q["N"]
    d = o.DEMO[kind]
    rng = np.random.default_rng(q["seed"])
    taille = q.get("psf_size", 7)
    st = _setup(kind, synth_image(M, N, 7), rng.standard_normal((M, N)), 0.99, taille)
    model = st["model"] if st["model"].psf_size == taille else o.BlurModel(kind, (M, N), psf_size=taille)
    steps = max(warmup - 1, 0) + samples - 1
    noise = rng.standard_normal((steps, M, N))
    mask = q["mask"]((M, N))
    fix = tuple(q.get("fix", d["fix"]))
    cr = dict(theta=SCALE * d["c_theta"], p=tuple(SCALE * v for v in d["c_p"]), sigma=SCALE * d["c_sigma"])
    kw = dict(samples=samples, warmup=warmup, burnIn=burnIn, chambolleit=cit, model=model, fix=fix, c=cr)
    op = dict(samples=samples, warmup=warmup, burnIn=burnIn, chambolleit=cit, psf_size=taille, phi=0.0,
              th_init=st["th_init"], min_th=st["min_th"], max_th=st["max_th"], sigma=st["sigma"], sigma_init=st["sigma_init"],
              sigma_min=st["sigma_min"], sigma_max=st["sigma_max"], d_scale=st["d_scale"], d_exp=st["d_exp"], fix_sigma=0,
              gamma=st["gamma"])
    op["lambda"] = st["lam"]
    c = dict(theta=cr["theta"], sigma=cr["sigma"], lam=1.0, gam=1.0)
    for i, nm in enumerate(NAMES_OF[kind]):
        op[nm], op[nm + "_init"], op["min_" + nm], op["max_" + nm] = st["p_true"][i], d["init"][i], d["pmin"][i], d["pmax"][i]
        op["fix_" + nm] = int(fix[i])
        c[nm] = cr["p"][i]
    return dict(setup=st, model=model, kind=kind, mask=mask, noise=noise, kw=kw, op=op, c=c)


def chain_of(q, noise=None, mask=None, **kw):
    """The restatement on a problem (its own noise and mask unless given; kw overrides what the restatement takes)."""
    return msr.sapg_masked_chain(q["setup"], q["mask"] if mask is None else mask, noise=q["noise"] if noise is None else noise,
                                 **dict(q["kw"], **kw))


def chain(name, **kw):
    return chain_of(problem(name), **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement on the case's mask and injected normals (read-only for its users)."""
    return chain(name)


# ---- the fixed-parameter chain (sbtv_myula_masked): the case's data at th_init, p_true and the true sigma2
MYULA_SAMPLES = 8


def myula_problem(name):
    return myula_build(tuple(sorted(CASES[name].items())))


@functools.lru_cache(maxsize=None)
def myula_build(case, samples=MYULA_SAMPLES):
    """dict(y, mask, model, p, lam, gam, theta, s2, samples, noise (samples-2, M, N), chambolleit) of an explicit case."""
    q = build(case)
    st = q["setup"]
    M, N = st["y"].shape
    noise = np.random.default_rng(dict(case)["seed"] + 1).standard_normal((samples - 2, M, N))
    return dict(y=st["y"], mask=q["mask"], model=q["model"], p=st["p_true"], lam=st["lam"], gam=st["gamma"], theta=st["th_init"],
                s2=st["sigma"] ** 2, samples=samples, noise=noise, chambolleit=q["kw"]["chambolleit"])


def myula_chain_of(q, noise=None, **kw):
    q = dict(q, **kw)
    if noise is not None:
        q["noise"] = noise
    return msr.myula_masked_chain(q["y"], q["mask"], q["model"], q["p"], q["lam"], q["gam"], q["theta"], q["s2"], q["samples"],
                                  q["noise"], **{k: q[k] for k in ("chambolleit", "alt_tols", "perturb") if k in q})


def myula_chain(name, **kw):
    return myula_chain_of(myula_problem(name), **kw)


@functools.lru_cache(maxsize=None)
def myula_reference(name):
    return myula_chain(name)
