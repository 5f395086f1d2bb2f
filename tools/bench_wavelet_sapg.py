#!/usr/bin/env python3
"""Estimation of theta for the wavelet-l1 prior (`sbtv.SAPG_wavelet`, Haar, levels 4 unless told otherwise): time per iteration
of the device-resident driver (Philox normals) against the SAME iteration composed in Python from the entry points that
exist without it (`sbtv.mirdwt_TI2D`, `sbtv.mrdwt_TI2D`, `sbtv.soft`, the A / AT calls of `sbtv.BlurOperator`, torch
arithmetic and `torch.randn` on device tensors).  `--only composed` needs nothing of the driver, so it also runs on a tree
that does not have it.  The composition keeps eta / theta in 0-dim device tensors; `sbtv.soft` takes its threshold from the
host, so it reads theta(ii-2) back, which is one iteration old when it is needed; that read-back waits for the stream, so
the composition is also timed with the threshold written in torch on the device theta (`composed_nosync_*`), where nothing
waits inside the loop.  Device-resident images of the bench's
problem with the constants of SALSA/run_deblur_synthesis_L1.m:65-83 and a 7 x 7 Gaussian blur; every shape is warmed up,
then `--rounds` timed runs of `--steps` iterations; with injected noise the theta traces of the two must agree to 1e-9 relative, or the script stops with an error before it
times anything.  One JSON
line per size with the median and the best run."""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv, bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--wavelet", type=int, default=2, help="length of the Daubechies filter")
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--only", default=None, help="fused | composed: that part alone (e.g. under a profiler)")
ap.add_argument("--injected", action="store_true", help="time the driver with injected device noise instead of Philox")
a = ap.parse_args()
PARITY_RTOL = 1e-9          # the parity tolerance of tests/test_gpu_wavelet_sapg.py
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
nb = 3 * (a.levels - 1) + 1


def options(sigma, samples):
    Lf = 1.0 / sigma ** 2
    lam = min(5.0 / Lf, 2.0)
    return {"samples": samples, "warmup": 0, "burnIn": min(20, samples), "th_init": 0.01, "min_th": 1e-3, "max_th": 1.0,
            "d_exp": 0.8, "d_scale": 0.1 / 0.01, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam), "sigma": sigma, "seed": 1}


def composed(yd, op, o, noise=None, readback=True):
    """SAPG_algorithm_1.m:165-216 (theta part), one library call or torch expression per line; returns the theta trace.
    readback: threshold with `sbtv.soft` (the host reads theta back every iteration: a stream synchronisation); False: the
    threshold in torch from the device theta, so that nothing waits inside the loop."""
    lam, gam, s2, S = o["lambda"], o["gamma"], o["sigma"] ** 2, o["samples"]
    sq2g, lo, hi = math.sqrt(2 * gam), math.log(o["min_th"]), math.log(o["max_th"])
    if readback:
        soft = lambda X, th: sbtv.soft(X, lam * float(th), ctx=ctx)
    else:
        soft = lambda X, th: torch.sign(X) * torch.clamp(torch.abs(X) - lam * th, min=0.0)
    X = sbtv.mrdwt_TI2D(yd, h, a.levels, ctx=ctx)
    dimX = X.numel()
    eta = torch.tensor(math.log(o["th_init"]), dtype=torch.float64, device=X.device)
    thetas = [torch.tensor(o["th_init"], dtype=torch.float64, device=X.device)]
    prox = soft(X, thetas[0])
    for ii in range(2, S + 1):
        r = op.A(sbtv.mirdwt_TI2D(X, h, a.levels, ctx=ctx)) - yd
        G = sbtv.mrdwt_TI2D(op.AT(r), h, a.levels, ctx=ctx)
        # (normals in the memory layout of X: column-major)
        Z = noise[ii - 2] if noise is not None else torch.randn(X.shape[::-1], dtype=torch.float64, device=X.device).t()
        X = X + gam * (prox - X) / lam - gam * (G / s2) + sq2g * Z
        prox = soft(X, thetas[-1])
        g = torch.sum(torch.abs(X))
        delta = o["d_scale"] * (ii ** (-o["d_exp"]) / dimX)
        eta = torch.clamp(eta + delta * (dimX / thetas[-1] - g) * torch.exp(eta), lo, hi)
        thetas.append(torch.exp(eta))
    return torch.stack(thetas).cpu().numpy()


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


for size in a.sizes:
    x, y, sigma, _ = bench.make_problem(1, size)
    yd = sbtv.to_device(y)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    S = a.steps + 1
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "steps": a.steps, "rounds": a.rounds, "dtype": "f64",
           "data": "synthetic", "dimX": nb * size * size}
    fused = lambda o, nz=None: sbtv.SAPG_wavelet(yd, op, h, a.levels, o, noise=nz, ctx=ctx)
    chk = options(sigma, 6)
    # five injected steps: column-major (M, nb N) arrays, the layout of the coefficient tensors the transforms return
    nz = torch.randn((5, nb * size, size), dtype=torch.float64, device=yd.device, generator=torch.Generator(yd.device).manual_seed(3))
    nzv = nz.permute(0, 2, 1)
    if a.only in (None, "composed"):
        tc = composed(yd, op, chk, nzv)                      # warm-up, and the reference of the check
        out["composed_thetas"] = tc.tolist()
    if a.only in (None, "fused"):
        tf = fused(chk, nz)[1]["thetas"]
        out["fused_thetas"] = np.asarray(tf).tolist()
    if a.only in (None, "composed"):
        out["composed_nosync_thetas_rel_diff"] = float(np.max(np.abs(composed(yd, op, chk, nzv, readback=False) / tc - 1.0)))
    if a.only is None:
        out["thetas_rel_diff"] = float(np.max(np.abs(np.asarray(tf) / tc - 1.0)))
        if not out["thetas_rel_diff"] <= PARITY_RTOL:            # a diverged driver is not timed
            print(json.dumps(out), flush=True)
            sys.exit(f"theta traces of the driver and the composition differ by {out['thetas_rel_diff']:.3g} > {PARITY_RTOL}")
    o = options(sigma, S)
    if a.only in (None, "fused"):
        big = None
        if a.injected:
            big = torch.randn((a.steps, nb * size, size), dtype=torch.float64, device=yd.device)
        ts = timed(lambda: fused(o, big), a.rounds)
        out["fused_noise"] = "injected" if a.injected else "philox"
        out["fused_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["fused_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only in (None, "composed"):
        for key, rb in (("composed", True), ("composed_nosync", False)):
            ts = timed(lambda: composed(yd, op, o, readback=rb), a.rounds)
            out[key + "_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
            out[key + "_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only is None:
        out["composed_over_fused"] = out["composed_ms_per_iteration_median"] / out["fused_ms_per_iteration_median"]
        out["composed_nosync_over_fused"] = out["composed_nosync_ms_per_iteration_median"] / out["fused_ms_per_iteration_median"]
    print(json.dumps(out), flush=True)
