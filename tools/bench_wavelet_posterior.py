#!/usr/bin/env python3
"""Fixed-theta MYULA on the wavelet coefficients (`sbtv.myula_wavelet`, Haar, levels 4, Philox normals): ms per iteration
  none        without moments
  image       with the image moments on every iteration (fused into the level-1 synthesis launch)
  image+coef  with the image and the coefficient moments on every iteration (the latter fused into the step kernel)
and, as the baseline, the iteration of `sbtv.SAPG_wavelet` (warmup 0), which is the same iteration plus the one-workgroup
parameter update.  `--only sapg` times that alone and needs nothing of the new entry, so with SBTV_LIBRARY it also times a
build of the tree before it.  Device-resident image of the bench's problem with the constants of
SALSA/run_deblur_synthesis_L1.m:65-83 and a 7 x 7 Gaussian blur, theta 0.03.  Every shape is warmed up, then `--rounds` (5)
timed runs of `--steps` iterations each: `best3` is the best of the first three, `spread` is (max - min) / median of all.
The added time of a moment set is printed next to its byte model at 8 TB/s (32 B per pixel; 32 (3J+1) B per pixel for the
coefficients) and, for the image moments, next to what a separate pass would move (40 B per pixel: it re-reads the image).
One JSON line per size."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv, bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, nargs="+", default=[400, 40], help="iterations per timed run, one value per size")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--theta", type=float, default=0.03)
ap.add_argument("--only", default=None, help="sapg | myula: that part alone")
a = ap.parse_args()
HBM_BYTES_PER_S = 8e12
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(2)
nb = 3 * (a.levels - 1) + 1


def options(sigma, samples):
    Lf = 1.0 / sigma ** 2
    lam = min(5.0 / Lf, 2.0)
    return {"samples": samples, "warmup": 0, "burnIn": min(20, samples), "th_init": 0.01, "min_th": 1e-3, "max_th": 1.0,
            "d_exp": 0.8, "d_scale": 0.1 / 0.01, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam), "sigma": sigma, "seed": 1}


def timed(fn, rounds, steps):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ms = [1e3 * t / steps for t in ts]
    return {"best3": min(ms[:3]), "median": statistics.median(ms), "min": min(ms), "max": max(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


for size, steps in zip(a.sizes, a.steps + a.steps[-1:] * len(a.sizes)):
    x, y, sigma, _ = bench.make_problem(1, size)
    yd = sbtv.to_device(y)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    o = options(sigma, steps + 1)
    out = {"size": size, "wavelet": 2, "levels": a.levels, "steps": steps, "rounds": a.rounds, "dtype": "f64",
           "data": "synthetic", "noise": "philox", "library": os.environ.get("SBTV_LIBRARY", "default")}
    if a.only in (None, "sapg"):
        sbtv.SAPG_wavelet(yd, op, h, a.levels, options(sigma, 4), ctx=ctx)                       # warm-up
        out["sapg_ms_per_iteration"] = timed(lambda: sbtv.SAPG_wavelet(yd, op, h, a.levels, o, ctx=ctx), a.rounds, steps)
    if a.only in (None, "myula"):
        modes = (("none", None), ("image", True), ("image+coef", dict(coefficients=True)))
        run = lambda post, oo=o: sbtv.myula_wavelet(yd, op, h, a.levels, oo, theta=a.theta, sigma2=sigma ** 2, posterior=post,
                                                    ctx=ctx)
        for name, post in modes:
            run(post, options(sigma, 4))                                                         # warm-up
        for name, post in modes:
            out[name + "_ms_per_iteration"] = timed(lambda: run(post), a.rounds, steps)
        px = size * size
        base = out["none_ms_per_iteration"]["best3"]
        out["image_added_us"] = 1e3 * (out["image_ms_per_iteration"]["best3"] - base)
        out["image_model_us"] = 1e6 * 32 * px / HBM_BYTES_PER_S
        out["separate_pass_model_us"] = 1e6 * 40 * px / HBM_BYTES_PER_S
        out["coef_added_us"] = 1e3 * (out["image+coef_ms_per_iteration"]["best3"] - out["image_ms_per_iteration"]["best3"])
        out["coef_model_us"] = 1e6 * 32 * nb * px / HBM_BYTES_PER_S
    print(json.dumps(out), flush=True)
