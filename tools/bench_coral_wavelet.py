#!/usr/bin/env python3
"""CoRAL with the TV + wavelet-l1 regulariser (`sbtv.CoRAL_wavelet`, Haar, levels 4 unless told otherwise): time per outer
iteration of the driver against the SAME iteration composed in Python from the entry points (`sbtv.chambolle_prox_TV_stop`,
`sbtv.soft`, `sbtv.mirdwt_TI2D`, `sbtv.mrdwt_TI2D`, `sbtv.TVnorm`, the A / AT / invLS calls of `sbtv.BlurOperator`) and torch
arithmetic on device tensors, and, in the same process, `sbtv.SALSA_analysis` (the wavelet term alone) and `sbtv.SALSA_v2` with
the same 'TVITERS' (the TV term alone) per outer iteration at the same shapes: the driver does their combined work with one FFT
triple instead of two.  Device-resident images of the bench's problem, tau1 = tau2 = 0.5 sigma^2, mu1 = mu2 = 0.05, start B'y,
K outer iterations with an unreachable tolerance; every shape is warmed up first, then `--rounds` timed runs of each; one JSON
line per size with the median and the best run."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv, bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--wavelet", type=int, default=2, help="length of the Daubechies filter")
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--tviters", type=int, default=5)
ap.add_argument("--only", default=None, help="driver | composed | analysis | salsa: that part alone (e.g. under a profiler)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9              # the peak every byte-model fraction of this project is taken against


def composed(yd, op, tau1, tau2, mu1, mu2, K):
    """CoRAL_v2.m:349-433 with P1 = identity / TV, P2 = W, P2T = W' / soft (include/sbtv.h, sbtv_CoRAL_wavelet), one library call
    or torch expression per line."""
    mu = mu1 + mu2
    ATy = op.AT(yd)
    x = ATy
    u, bu = x, x.clone()
    P2Tx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
    bv = P2Tx.clone()
    duals = (torch.zeros_like(x), torch.zeros_like(x))
    obj = []
    for _ in range(K):
        u, px, py = sbtv.chambolle_prox_TV_stop(x - bu, "lambda", tau1 / mu1, "maxiter", a.tviters, "dualvars", duals, ctx=ctx)
        duals = (px, py)
        v = sbtv.soft(P2Tx - bv, tau2 / mu2, ctx=ctx)
        r = ATy + mu1 * (u + bu) + mu2 * sbtv.mirdwt_TI2D(v + bv, h, a.levels, ctx=ctx)
        x = op.invLS(r, mu)
        P2Tx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
        bu = bu + (u - x)
        bv = bv + (v - P2Tx)
        res = yd - op.A(x)
        obj.append(float(0.5 * torch.sum(res * res) + tau2 * torch.sum(torch.abs(v))) + tau1 * sbtv.TVnorm(u, ctx=ctx))
    return x, np.array(obj)


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


def measure(out, name, fn):
    fn(5)
    ts = timed(lambda: fn(a.steps), a.rounds)
    out[name + "_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
    out[name + "_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    out[name + "_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps


for size in a.sizes:
    x, y, sigma, noise = bench.make_problem(1, size)
    yd = sbtv.to_device(y)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    tau1 = tau2 = 0.5 * sigma ** 2
    mu1 = mu2 = 0.05
    loop = ("AT", op.T, "STOPCRITERION", 1, "TOLERANCEA", -1.0, "INITIALIZATION", 2)
    frame = ("WAVELET", h, "LEVELS", a.levels)
    driver = lambda K: sbtv.CoRAL_wavelet(yd, op, tau1, tau2, "MU1", mu1, "MU2", mu2, *frame, "TVITERS", a.tviters,
                                          "LS", op.LS(mu1 + mu2), *loop, "MAXITERA", K, ctx=ctx)
    analysis = lambda K: sbtv.SALSA_analysis(yd, op, tau2, "MU", mu2, *frame, *loop, "MAXITERA", K, ctx=ctx)
    salsa = lambda K: sbtv.SALSA_v2(yd, op, tau1, "MU", mu1, "LS", op.LS(mu1), "TVINITIALIZATION", 1, "TVITERS", a.tviters, *loop,
                                    "MAXITERA", K, ctx=ctx)
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "tviters": a.tviters, "steps": a.steps, "rounds": a.rounds,
           "dtype": "f64", "data": "synthetic"}
    if a.only in (None, "driver", "composed"):
        f = driver(5)                                        # warm-up, and the two must be the same iteration
        c = composed(yd, op, tau1, tau2, mu1, mu2, 5)
        out["objective_driver"] = [float(v) for v in f[3][1:]]
        out["objective_composed"] = [float(v) for v in c[1]]
        out["objective_rel_diff"] = float(np.max(np.abs(f[3][1:] / c[1] - 1.0)))
        out["x_max_abs_diff"] = float(torch.max(torch.abs(f[0] - c[0])))
    if a.only in (None, "driver"):
        measure(out, "driver", driver)
        out["s_pass_model_us_at_peak"] = 1e6 * 32 * size * size / HBM_PEAK      # three pixel arrays in, one out
        out["post_pass_model_us_at_peak"] = 1e6 * 40 * size * size / HBM_PEAK   # x, u, bu in, bu, g1 out (no true, no xprev)
    if a.only in (None, "composed"):
        ts = timed(lambda: composed(yd, op, tau1, tau2, mu1, mu2, a.steps), a.rounds)
        out["composed_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["composed_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only in (None, "analysis"):
        measure(out, "analysis", analysis)
    if a.only in (None, "salsa"):
        measure(out, "salsa", salsa)
    if a.only is None:
        out["composed_over_driver"] = out["composed_ms_per_iteration_median"] / out["driver_ms_per_iteration_median"]
        out["analysis_plus_salsa_ms_per_iteration_median"] = (out["analysis_ms_per_iteration_median"] +
                                                              out["salsa_ms_per_iteration_median"])
        out["driver_over_analysis_plus_salsa"] = (out["driver_ms_per_iteration_median"] /
                                                  out["analysis_plus_salsa_ms_per_iteration_median"])
    print(json.dumps(out), flush=True)
