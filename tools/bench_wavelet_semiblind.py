#!/usr/bin/env python3
"""Semi-blind estimation for the wavelet-l1 prior (`sbtv.SAPG_wavelet_semiblind`, Haar, levels 4, Philox normals): time per
iteration of three settings next to `sbtv.SAPG_wavelet` on the same problem in the same process:
  fixed      every parameter fixed at its true value (the chain of SAPG_wavelet: its overhead is the price of the entry)
  laplace    Laplace PSF, b free, sigma2 fixed
  gaussian   Gaussian PSF, w1 and w2 free, sigma2 free
Device-resident images of the bench's problem blurred with the family's true PSF (7 x 7), constants of
SALSA/run_deblur_synthesis_L1.m:65-83; every shape is warmed up, then `--rounds` timed runs of `--steps` iterations.  One JSON
line per size with the median and the best run of each setting and the overhead over SAPG_wavelet (profiles/wavelet_semiblind.md).

  python tools/bench_wavelet_semiblind.py [--sizes 512 2048] [--steps 50] [--rounds 5]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv, bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--levels", type=int, default=4)
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(2)
TRUE = {"gaussian": tuple(bench.W_TRUE), "laplace": (0.3,)}
BOUNDS = {"gaussian": ((0.1, 0.1), (1.0, 1.0)), "laplace": ((1e-3,), (1.0,))}
START = {"gaussian": (0.7, 0.6), "laplace": (0.1,)}


def options(sigma, samples):
    Lf = 1.0 / sigma ** 2
    lam = min(5.0 / Lf, 2.0)
    return {"samples": samples, "warmup": 0, "burnIn": min(20, samples), "th_init": 0.01, "min_th": 1e-3, "max_th": 1.0,
            "d_exp": 0.8, "d_scale": 0.1 / 0.01, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam), "sigma": sigma, "seed": 1}


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


def observe(x, kind, sigma, seed=2):
    """y = B_true x + sigma n with the circular blur of the family's true taps (top-left convention, utils/resize.m)."""
    taps = sbtv.psf_family(kind, 7, TRUE[kind])[0]
    pad = np.zeros(x.shape)
    pad[:7, :7] = taps
    Bx = np.real(np.fft.ifft2(np.fft.fft2(pad) * np.fft.fft2(x)))
    return Bx + sigma * np.random.default_rng(seed).standard_normal(x.shape), taps


for size in a.sizes:
    x, _, sigma, _ = bench.make_problem(1, size)
    x = np.asarray(x, dtype=np.float64).reshape(size, size)
    S = a.steps + 1
    out = {"size": size, "levels": a.levels, "steps": a.steps, "rounds": a.rounds, "dtype": "f64", "data": "synthetic",
           "noise": "philox"}
    o = options(sigma, S)
    runs = {}
    for kind in ("gaussian", "laplace"):
        y, taps = observe(x, kind, sigma)
        yd = sbtv.to_device(y)
        lo, hi = BOUNDS[kind]
        sb = dict(o, p_true=TRUE[kind], p_min=lo, p_max=hi, sigma2_min=0.1 * sigma ** 2, sigma2_max=10 * sigma ** 2, c_sigma=1000.0)
        if kind == "gaussian":
            A = sbtv.BlurOperator(taps, ctx=ctx)
            runs["theta_only"] = lambda yd=yd, A=A: sbtv.SAPG_wavelet(yd, A, h, a.levels, o, ctx=ctx)
            runs["fixed"] = lambda yd=yd, sb=sb: sbtv.SAPG_wavelet_semiblind(
                yd, "gaussian", h, a.levels, dict(sb, p_init=TRUE["gaussian"], fix_p=(True, True), fix_sigma=True), ctx=ctx)
            runs["gaussian"] = lambda yd=yd, sb=sb: sbtv.SAPG_wavelet_semiblind(
                yd, "gaussian", h, a.levels, dict(sb, p_init=START["gaussian"], fix_p=(False, False), c_p=(1.0, 1.0),
                                                  fix_sigma=False), ctx=ctx)
        else:
            runs["laplace"] = lambda yd=yd, sb=sb: sbtv.SAPG_wavelet_semiblind(
                yd, "laplace", h, a.levels, dict(sb, p_init=START["laplace"], fix_p=(False,), c_p=(10.0,), fix_sigma=True),
                ctx=ctx)
    # the all-fixed chain is the chain of SAPG_wavelet: a diverged driver is not timed
    th0 = np.asarray(runs["theta_only"]()[1]["thetas"])
    th1 = np.asarray(runs["fixed"]()[1]["thetas"])
    out["fixed_thetas_equal_theta_only"] = bool(np.array_equal(th0, th1))
    if not np.allclose(th0, th1, rtol=1e-9, atol=0):
        print(json.dumps(out), flush=True)
        sys.exit("the all-fixed chain differs from SAPG_wavelet")
    for key in ("theta_only", "fixed", "laplace", "gaussian"):
        runs[key]()                                           # warm-up of this shape and setting
        ts = timed(runs[key], a.rounds)
        out[key + "_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out[key + "_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    for key in ("fixed", "laplace", "gaussian"):
        out[key + "_over_theta_only"] = out[key + "_ms_per_iteration_median"] / out["theta_only_ms_per_iteration_median"]
    print(json.dumps(out), flush=True)
