#!/usr/bin/env python3
"""Masked-observation wavelet SALSA (`sbtv.SALSA_masked_analysis`, Haar, levels 4 unless told otherwise, the frame mask of
`sbtv.valid_mask`): time per outer iteration of the driver against the SAME iteration composed in Python from the entry points
(`sbtv.soft`, `sbtv.mirdwt_TI2D`, `sbtv.mrdwt_TI2D`, the A / AT / invLS calls of `sbtv.BlurOperator`) and torch arithmetic on
device tensors, and, for comparison, its two parents per outer iteration at the same shapes in the same process:
`sbtv.SALSA_analysis` (the fully observed likelihood, same prior) and `sbtv.SALSA_masked` (the same likelihood, TV prior with
TViters 10 as tools/bench_admm.py runs it).  Device-resident images of the bench's problem, tau = sigma^2, mu1 = 0.05, mu2 = 0.1,
start B'(m .* y), K outer iterations with an unreachable tolerance, no 'TRUE_X'; every shape is warmed up first, then `--rounds`
timed runs of each; one JSON line per size with the median and the best run, and the pixel pass's 56 B / pixel model at the
peak (its measured time comes from a kernel trace of `--only driver`)."""
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
ap.add_argument("--only", default=None, help="driver | composed | analysis | masked: that part alone (e.g. under a profiler)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9              # the peak every byte-model fraction of this project is taken against


def composed(yd, md, op, tau, mu1, mu2, K):
    """The iteration of include/sbtv.h (sbtv_SALSA_masked_analysis), one library call or torch expression per line."""
    my = md * yd
    x = op.AT(my)
    Bx = op.A(x)
    PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
    bu, bv = torch.zeros_like(PTx), torch.zeros_like(Bx)
    r = mu1 / mu2
    obj = []
    for _ in range(K):
        u = sbtv.soft(PTx - bu, tau / mu1, ctx=ctx)
        v = (my + mu2 * (Bx - bv)) / (md + mu2)
        x = op.invLS(op.AT(v + bv) + r * sbtv.mirdwt_TI2D(u + bu, h, a.levels, ctx=ctx), r)
        Bx = op.A(x)
        PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
        bu = bu + (u - PTx)
        bv = bv + (v - Bx)
        res = Bx - yd
        obj.append(0.5 * torch.sum(md * (res * res)) + tau * torch.sum(torch.abs(u)))
    return x, torch.stack(obj).cpu().numpy()


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


def record(out, name, fn):
    ts = timed(lambda: fn(a.steps), a.rounds)
    out[name + "_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
    out[name + "_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    out[name + "_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps


for size in a.sizes:
    x, y, sigma, noise = bench.make_problem(1, size)
    m = sbtv.valid_mask((size, size), 7)
    yd, md, ymd = sbtv.to_device(y), sbtv.to_device(m), sbtv.to_device(y * m)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    tau, mu1, mu2, theta = sigma ** 2, 0.05, 0.1, bench.THETA
    stop = ("AT", op.T, "STOPCRITERION", 1, "TOLERANCEA", -1.0, "INITIALIZATION", 2)
    frame = ("WAVELET", h, "LEVELS", a.levels)
    driver = lambda K: sbtv.SALSA_masked_analysis(ymd, op, md, tau, "MU1", mu1, "MU2", mu2, *frame, *stop, "MAXITERA", K, ctx=ctx)
    analysis = lambda K: sbtv.SALSA_analysis(yd, op, tau, "MU", mu1, *frame, *stop, "MAXITERA", K, ctx=ctx)
    masked = lambda K: sbtv.SALSA_masked(ymd, op, md, theta * tau, "MU1", theta / 10, "MU2", mu2, "TVITERS", 10, *stop, "MAXITERA", K,
                                         ctx=ctx)
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "steps": a.steps, "rounds": a.rounds, "dtype": "f64",
           "data": "synthetic"}
    if a.only in (None, "driver", "composed"):
        f = driver(5)                                        # warm-up, and the two must be the same iteration
        c = composed(ymd, md, op, tau, mu1, mu2, 5)
        out["objective_rel_diff"] = float(np.max(np.abs(f[3][1:] / c[1] - 1.0)))
        out["x_max_abs_diff"] = float(torch.max(torch.abs(f[0] - c[0])))
    if a.only in (None, "driver"):
        record(out, "driver", driver)
        out["pixel_pass_model_us_at_peak"] = 1e6 * 56 * size * size / HBM_PEAK     # five arrays read, two written: 56 B per pixel
    if a.only in (None, "composed"):
        ts = timed(lambda: composed(ymd, md, op, tau, mu1, mu2, a.steps), a.rounds)
        out["composed_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["composed_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only is None:
        out["composed_over_driver"] = out["composed_ms_per_iteration_median"] / out["driver_ms_per_iteration_median"]
    if a.only in (None, "analysis"):
        analysis(5)
        record(out, "analysis", analysis)
    if a.only in (None, "masked"):
        masked(5)
        record(out, "masked", masked)
    print(json.dumps(out), flush=True)
