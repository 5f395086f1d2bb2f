"""The SAPG runs with an SK-ROCK kernel shared by tests/test_sapg_skrock_cpu.py and tests/test_gpu_sapg_skrock.py.  A problem is
that of test_sapg_matches_oracle_with_injected_noise: demo_setup(kind, synth_image(M, N, 7), noise of seed 11, evMax = 0.99),
chambolleit = 25, eta = 0.05, samples 12, warmup 4, burnIn 8; the step is dt = 0.8 max_step(stages, eta, min(sigma_min,
sigma_max), lambda), the bound at the smallest sigma2 the chain may reach.  The demo's c_theta, c_p and c_sigma are each
multiplied by 0.02: at the reference's own scales a 32 x 32 chain throws theta and sigma2 against their clamps within two
iterations, and with Moffat it leaves the stability region once sigma2 sits on its lower bound.
Each reference (tests/sapg_skrock_restatement.py) is computed once per session and never modified.

No case may sit on the edge of the Chambolle stop rule (tests/test_sapg_skrock_cpu.py checks it): should one, change its SEED."""
import functools

import numpy as np

from conftest import synth_image

import sbtv_oracle as o
import sapg_skrock_restatement as ssr

ETA, CHAMBOLLEIT, SCALE = 0.05, 25, 0.02
SAMPLES, WARMUP, BURNIN = 12, 4, 8
NAMES_OF = {"gaussian": ("w1", "w2"), "moffat": ("alpha", "beta"), "laplace": ("b",)}

# name -> dict(kind, M, N, stages, seed[, psf_size, fix, fix_sigma])
CASES = {
    "gauss-s2": dict(kind="gaussian", M=32, N=32, stages=2, seed=11, fix=(False, False)),   # no middle stage; both widths free
    "moffat-s3": dict(kind="moffat", M=32, N=32, stages=3, seed=11),          # odd s: the sample and P_next swap buffers
    "laplace-s10": dict(kind="laplace", M=32, N=32, stages=10, seed=11),      # one PSF parameter
    "moffat-rect-s5": dict(kind="moffat", M=24, N=40, stages=5, seed=11),     # chirp-z path, tvnorm_partials path
    "laplace-9x9-s2": dict(kind="laplace", M=32, N=32, stages=2, seed=11, psf_size=9),      # the > 8 x 8 tap path
    "gauss-fixed-s3": dict(kind="gaussian", M=32, N=32, stages=3, seed=11, fix=(True, True)),   # no spectra rebuilt, sigma2 free
}
NAMES = list(CASES)


def problem(name, samples=SAMPLES, warmup=WARMUP, burnIn=BURNIN):
    return build(tuple(sorted(CASES[name].items())), samples, warmup, burnIn)


@functools.lru_cache(maxsize=None)
def build(case, samples=SAMPLES, warmup=WARMUP, burnIn=BURNIN):
    """The problem of an explicit case, given as its sorted items (tests/tv_sampler_geometry_cases.py has further ones; a case
    may name its own chambolleit): dict(setup, model, kind, stages, dt, noise (steps, M, N), kw: what the restatement takes
    beyond setup / noise, op, c: what sbtv.SAPG_skrock takes)."""
    q = dict(case)
    cit = q.get("chambolleit", CHAMBOLLEIT)
    kind, M, N, stages = q["kind"], q["M"], q["N"], q["stages"]
    d = o.DEMO[kind]
    rng = np.random.default_rng(q["seed"])
    st = o.demo_setup(kind, synth_image(M, N, 7), rng.standard_normal((M, N)), evMax=0.99)
    taille = q.get("psf_size", 7)
    model = st["model"] if taille == 7 else o.BlurModel(kind, (M, N), psf_size=taille)
    steps = max(warmup - 1, 0) + samples - 1
    noise = rng.standard_normal((steps, M, N))
    fix = tuple(q.get("fix", d["fix"]))
    dt = 0.8 * ssr.max_step(stages, ETA, min(st["sigma_min"], st["sigma_max"]), st["lam"])
    cr = dict(theta=SCALE * d["c_theta"], p=tuple(SCALE * v for v in d["c_p"]), sigma=SCALE * d["c_sigma"])
    kw = dict(samples=samples, warmup=warmup, burnIn=burnIn, stages=stages, dt=dt, eta=ETA, chambolleit=cit, model=model,
              fix=fix, c=cr)
    op = dict(samples=samples, warmup=warmup, burnIn=burnIn, chambolleit=cit, psf_size=taille, phi=0.0,
              th_init=st["th_init"], min_th=st["min_th"], max_th=st["max_th"], sigma=st["sigma"], sigma_init=st["sigma_init"],
              sigma_min=st["sigma_min"], sigma_max=st["sigma_max"], d_scale=st["d_scale"], d_exp=st["d_exp"], fix_sigma=0)
    op["lambda"] = st["lam"]
    c = dict(theta=cr["theta"], sigma=cr["sigma"], lam=1.0)
    for i, nm in enumerate(NAMES_OF[kind]):
        op[nm], op[nm + "_init"], op["min_" + nm], op["max_" + nm] = st["p_true"][i], d["init"][i], d["pmin"][i], d["pmax"][i]
        op["fix_" + nm] = int(fix[i])
        c[nm] = cr["p"][i]
    return dict(setup=st, model=model, kind=kind, stages=stages, dt=dt, noise=noise, kw=kw, op=op, c=c)


def chain_of(q, noise=None, **kw):
    """The restatement on a problem (its own noise unless given; kw overrides what the restatement takes)."""
    return ssr.sapg_skrock_chain(q["setup"], noise=q["noise"] if noise is None else noise, **dict(q["kw"], **kw))


def chain(name, **kw):
    return chain_of(problem(name), **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement on the case's injected normals (read-only for its users)."""
    return chain(name)
