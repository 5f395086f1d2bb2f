"""The semi-blind wavelet-l1 problems shared by tests/test_wavelet_sb_cpu.py and tests/test_gpu_wavelet_sb.py: synth_image (or
the tiled man_512), sbtv_oracle.demo_setup(kind, ..., BSNR 30) for y, sigma and the sigma2 bounds, the script's constants as
tests/wavelet_sapg_cases.options sets them, PSF bounds and true values from sbtv_oracle.DEMO.  Each reference (the literal
restatement, tests/wavelet_sb_restatement.py) is computed once per session and never modified."""
import functools
import os

import numpy as np

from conftest import GOLDEN, synth_image

import wavelet_cases as wc
import wavelet_sapg_cases as wsc
import wavelet_sb_restatement as wsb

# name: (M, N), filter length, levels, kind, start values per chain, c_p, sigma2 free, fix_p, warmup, samples, noise seed
CASES = {
    "A": ((64, 64), 2, 4, "laplace", [(0.1,)], (10.0,), False, (False,), 10, 160, 31),
    "B": ((100, 90), 4, 3, "gaussian", [(0.7, 0.6), (0.5, 0.8)], (1.0, 1.0), False, (False, False), 0, 60, 32),
    "C": ((64, 64), 2, 4, "laplace", [(0.1,)], (10.0,), True, (False,), 0, 80, 33),
    "D": ((34, 30), 2, 3, "moffat", [(0.6, 3.5)], (1.0, 1.0), False, (False, True), 0, 3, 34),
    "E": ((1024, 1024), 2, 4, "laplace", [(0.1,)], (10.0,), False, (False,), 2, 6, 35),
}
C_SIGMA = 1000.0


def image(shape, b=0):
    if shape == (1024, 1024):
        return np.tile(np.load(os.path.join(GOLDEN, "man_512.npy")).astype(np.float64), (2, 2))
    return synth_image(shape[0], shape[1], 4 + 5 * b)


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(y (B, M, N), model, kind, h, levels, ops (one op per chain: they differ in p_init only), batch)."""
    import sbtv_oracle as o
    shape, K, levels, kind, starts, c_p, sigma_free, fix_p, warmup, samples, _ = CASES[name]
    d = o.DEMO[kind]
    ys, st0 = [], None
    for b in range(len(starts)):
        x = image(shape, b)
        st = o.demo_setup(kind, x, np.random.default_rng(3 + 3 * b).standard_normal(x.shape), evMax=1.0, BSNR=30.0)
        ys.append(st["y"])
        st0 = st if st0 is None else st0                     # one sigma2 per call: that of image 0
    s_lo, s_hi = sorted((st0["sigma_min"], st0["sigma_max"]))
    base = wsc.options(st0["sigma"], samples, warmup)
    if sigma_free:
        base["sigma2"] = (s_lo + s_hi) / 2                    # sigma2(1): the midpoint of its bounds
        del base["sigma"]
    base.update(p_true=tuple(d["true"]), p_min=tuple(d["pmin"]), p_max=tuple(d["pmax"]), fix_p=tuple(fix_p), c_p=tuple(c_p),
                fix_sigma=not sigma_free, sigma2_min=s_lo, sigma2_max=s_hi, c_sigma=C_SIGMA, psf_size=7)
    ops = [dict(base, p_init=tuple(p0)) for p0 in starts]
    return dict(y=np.stack(ys), model=st0["model"], kind=kind, h=wc.daub(K), levels=levels, ops=ops, batch=len(starts),
                sigma_true2=st0["sigma"] ** 2)


def noise(name, samples=None):
    """(steps, B, M, (3J+1) N) injected normals of a case; not cached, case E is 0.5 GB."""
    shape, _, levels, _, starts, _, _, _, warmup, S, seed = CASES[name]
    steps = max(warmup - 1, 0) + (S if samples is None else samples) - 1
    return np.random.default_rng(seed).standard_normal((steps, len(starts), shape[0], wsc.bands(levels) * shape[1]))


def run(fn, p, nz, xw0=None, **opkw):
    """fn (a restatement) on every chain of problem p with noise nz (steps, B, ...): [(eb, results)] per chain."""
    return [fn(p["y"][b], p["model"], p["h"], p["levels"], dict(p["ops"][b], **opkw), nz[:, b],
               None if xw0 is None else xw0[b]) for b in range(p["batch"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The literal loop on every chain of the case (read-only for its users)."""
    return run(wsb.literal, problem(name), noise(name))
