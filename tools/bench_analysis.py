#!/usr/bin/env python3
"""Analysis-prior wavelet SALSA (`sbtv.SALSA_analysis`, Haar, levels 4 unless told otherwise): time per outer iteration of the
driver against the SAME iteration composed in Python from the entry points (`sbtv.soft`, `sbtv.mirdwt_TI2D`,
`sbtv.mrdwt_TI2D`, the A / AT / invLS calls of `sbtv.BlurOperator`) and torch arithmetic on device tensors, and, for comparison,
`sbtv.SALSA_wavelet` (the synthesis form) per outer iteration at the same shapes.  Device-resident images of the bench's
problem, tau = sigma^2, mu = 0.05, start B'y, K outer iterations with an unreachable tolerance; every shape is warmed up
first, then `--rounds` timed runs of each; one JSON line per size with the median and the best run."""
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
ap.add_argument("--only", default=None, help="driver | composed | synthesis: that part alone (e.g. under a profiler)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9              # the peak every byte-model fraction of this project is taken against


def composed(yd, op, tau, mu, K):
    """SALSA_v2.m:389-451 with P = W, PT = W' (include/sbtv.h, sbtv_SALSA_analysis), one library call or torch expression
    per line."""
    ATy = op.AT(yd)
    x = ATy
    PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
    bu = torch.zeros_like(PTx)
    obj = []
    for _ in range(K):
        u = sbtv.soft(PTx - bu, tau / mu, ctx=ctx)
        r = ATy + mu * sbtv.mirdwt_TI2D(u + bu, h, a.levels, ctx=ctx)
        x = op.invLS(r, mu)
        PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
        bu = bu + (u - PTx)
        res = yd - op.A(x)
        obj.append(0.5 * torch.sum(res * res) + tau * torch.sum(torch.abs(u)))
    return x, torch.stack(obj).cpu().numpy()


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


for size in a.sizes:
    x, y, sigma, noise = bench.make_problem(1, size)
    yd = sbtv.to_device(y)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    tau, mu = sigma ** 2, 0.05
    common = ("MU", mu, "WAVELET", h, "LEVELS", a.levels, "AT", op.T, "STOPCRITERION", 1, "TOLERANCEA", -1.0, "INITIALIZATION", 2)
    driver = lambda K: sbtv.SALSA_analysis(yd, op, tau, *common, "MAXITERA", K, ctx=ctx)
    synthesis = lambda K: sbtv.SALSA_wavelet(yd, op, tau, *common, "MAXITERA", K, ctx=ctx)
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "steps": a.steps, "rounds": a.rounds, "dtype": "f64",
           "data": "synthetic"}
    if a.only in (None, "driver", "composed"):
        f = driver(5)                                        # warm-up, and the two must be the same iteration
        c = composed(yd, op, tau, mu, 5)
        out["objective_rel_diff"] = float(np.max(np.abs(f[3][1:] / c[1] - 1.0)))
        out["x_max_abs_diff"] = float(torch.max(torch.abs(f[0] - c[0])))
    if a.only in (None, "driver"):
        ts = timed(lambda: driver(a.steps), a.rounds)
        out["driver_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["driver_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
        out["driver_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps
        coef = (3 * (a.levels - 1) + 1) * size * size
        out["step_pass_model_us_at_peak"] = 1e6 * 40 * coef / HBM_PEAK   # five coefficient arrays, 40 B per coefficient
    if a.only in (None, "composed"):
        ts = timed(lambda: composed(yd, op, tau, mu, a.steps), a.rounds)
        out["composed_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["composed_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only is None:
        out["composed_over_driver"] = out["composed_ms_per_iteration_median"] / out["driver_ms_per_iteration_median"]
    if a.only in (None, "synthesis"):
        synthesis(5)
        ts = timed(lambda: synthesis(a.steps), a.rounds)
        out["synthesis_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["synthesis_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
        out["synthesis_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps
    print(json.dumps(out), flush=True)
