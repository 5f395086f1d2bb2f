#!/usr/bin/env python3
"""Overhead of the posterior moments (sbtv_SAPG_algorithm_moments) against the same SAPG call without them.

  python tools/bench_posterior.py                 # both shapes below, device-resident y, Philox noise
  python tools/bench_posterior.py --shape 512     # SAPG 512x512, one chain, Gaussian PSF (element-wise MYULA step)
  python tools/bench_posterior.py --shape 8x1024  # SAPG 8 x 1024x1024, Laplace PSF (fused epilogue of the column pass)

Every SAPG iteration after burnIn = 2 is selected (thin = 1): the worst case, 32 B more per pixel and iteration.  The two
calls alternate `--reps` times; the best time of each is reported (ms per SAPG iteration) with the ratio, one JSON line
per shape on stdout.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))

import numpy as np
import sbtv
import torch


def problem(shape):
    man = np.load(os.path.join(ROOT, "tests", "golden", "man_512.npy")).astype(np.float64)
    if shape == "512":
        kind, M, B, samples = "gaussian", 512, 1, 600
    else:
        kind, M, B, samples = "laplace", 1024, 8, 120
    x = np.tile(man, (M // 512, M // 512))
    st = sbtv.demo_setup(kind, x, np.random.default_rng(0).standard_normal(x.shape), evMax=1.0)
    op = dict(samples=samples, warmup=2, burnIn=2, psf_size=7, phi=0.0, gamma=st["gamma"], th_init=0.01, min_th=1e-3,
              max_th=1.0, sigma=st["sigma"], sigma_init=st["sigma_init"], sigma_min=st["sigma_min"],
              sigma_max=st["sigma_max"], d_scale=1.0, d_exp=0.8, fix_sigma=0, seed=3)
    op["lambda"] = st["lambda"]
    if kind == "gaussian":
        op.update(w1=0.4, w2=0.3, w1_init=0.5, w2_init=0.3, min_w1=0.1, min_w2=0.1, max_w1=1.0, max_w2=1.0, fix_w1=1, fix_w2=1)
        c = dict(theta=0.01, w1=10.0, w2=10.0, sigma=1000.0, lam=1.0, gam=1.0)
        fn = sbtv.SAPG_algorithm_Guassian
    else:
        op.update(b=0.3, b_init=0.3, min_b=0.1, max_b=1.0, fix_b=0)
        c = dict(theta=0.01, b=100.0, sigma=1e4, lam=1.0, gam=1.0)
        fn = sbtv.SAPG_algorithm_laplace
    y = np.repeat(st["y"][None], B, axis=0) if B > 1 else st["y"]
    return fn, sbtv.to_device(y, "cuda:0"), op, c, samples, B, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("512", "8x1024", "all"), default="all")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for shape in (("512", "8x1024") if a.shape == "all" else (a.shape,)):
        fn, yd, op, c, samples, B, M = problem(shape)
        fn(yd, dict(op, samples=4), c)                                   # workspaces, module load
        fn(yd, dict(op, samples=4), c, posterior=True)
        best = {"plain": 1e30, "moments": 1e30}
        for _ in range(a.reps):
            for tag, kw in (("plain", {}), ("moments", {"posterior": dict(first=0, thin=1)})):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(yd, op, c, **kw)
                torch.cuda.synchronize()
                best[tag] = min(best[tag], time.perf_counter() - t0)
        ms = {k: 1e3 * v / (samples + op["warmup"] - 2) for k, v in best.items()}
        print(json.dumps({"shape": f"{B}x{M}x{M}", "samples": samples, "selected": samples - 1,
                          "ms_per_iteration_plain": round(ms["plain"], 4),
                          "ms_per_iteration_moments": round(ms["moments"], 4),
                          "overhead": round(ms["moments"] / ms["plain"] - 1.0, 4),
                          "moment_bytes_per_iteration": 32 * B * M * M}), flush=True)


if __name__ == "__main__":
    main()
