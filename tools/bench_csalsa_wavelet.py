#!/usr/bin/env python3
"""C-SALSA with the wavelet analysis prior (`sbtv.csalsa_wavelet`, Haar, levels 4, mu1 = mu2 = 1 unless told otherwise): time per
outer iteration of the driver against the SAME iteration composed in Python from the entry points (`sbtv.soft`,
`sbtv.mirdwt_TI2D`, `sbtv.mrdwt_TI2D`, the A / AT / invLS calls of `sbtv.BlurOperator`) and torch arithmetic on device tensors,
and, for comparison, `sbtv.SALSA_analysis` (the unconstrained analysis form) per outer iteration at the same shapes.
Device-resident images of the bench's problem, sigma of the problem, the default epsilon, start B'y, K iterations with an
unreachable tolerance; every shape is warmed up first, then `--rounds` timed runs of each; one JSON line per size with the median
and the best run, and the byte models of the two step passes (wav_cstep_kernel 32 B per coefficient, wav_astep_kernel 40 B).
The time of the step kernels themselves comes from a kernel trace of `--only drivers` (both drivers in one process)."""
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
ap.add_argument("--mu1", type=float, default=1.0)
ap.add_argument("--mu2", type=float, default=1.0)
ap.add_argument("--only", default=None, help="driver | composed | analysis | drivers (driver and analysis, e.g. under a profiler)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9              # the peak every byte-model fraction of this project is taken against


def composed(yd, op, mu1, mu2, eps, K):
    """CSALSA_v2.m:401-501 with P = W, PT = W' (include/sbtv.h, sbtv_CSALSA_wavelet), one library call or torch expression per
    line; K - 1 iterations, as the loop runs outer = 2..K.  Returns x and the traces criterion, objective = ||W'x||_1."""
    x = op.AT(yd)
    PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
    u = torch.zeros_like(PTx)
    bu = torch.zeros_like(PTx)
    v = torch.zeros_like(yd)
    bv = torch.zeros_like(yd)
    crit, obj = [], []
    for _ in range(K - 1):
        r = mu1 * sbtv.mirdwt_TI2D(u + bu, h, a.levels, ctx=ctx) + mu2 * op.AT(yd + v + bv)
        x = op.invLS(r, mu1)
        PTx = sbtv.mrdwt_TI2D(x, h, a.levels, ctx=ctx)
        u = sbtv.soft(PTx - bu, 1.0 / mu1, ctx=ctx)
        Ax = op.A(x)
        ve = Ax - yd - bv
        n_ve = torch.linalg.vector_norm(ve)
        v = ve * torch.clamp(eps / n_ve, max=1.0)
        bv = bv - (Ax - yd - v)
        bu = bu - (PTx - u)
        crit.append(torch.linalg.vector_norm(Ax - yd))
        obj.append(torch.sum(torch.abs(PTx)))
    return x, torch.stack(crit).cpu().numpy(), torch.stack(obj).cpu().numpy()


def timed(fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts


for size in a.sizes:
    x, y, sigma, noise = bench.make_problem(1, size)
    yd = sbtv.to_device(y)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    eps = float(np.sqrt(size * size + 8 * np.sqrt(size * size)) * sigma)
    frame = ("WAVELET", h, "LEVELS", a.levels, "AT", op.T, "TOLERANCEA", -1.0, "INITIALIZATION", 2)
    # K + 1 entries: the state before the loop and K iterations, as many as the K of SALSA_analysis
    driver = lambda K: sbtv.csalsa_wavelet(yd, op, a.mu1, a.mu2, sigma, *frame, "STOPCRITERION", 3, "MAXITERA", K + 1, ctx=ctx)
    analysis = lambda K: sbtv.SALSA_analysis(yd, op, sigma ** 2, "MU", 0.05, *frame, "STOPCRITERION", 1, "MAXITERA", K, ctx=ctx)
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "mu1": a.mu1, "mu2": a.mu2, "steps": a.steps,
           "rounds": a.rounds, "dtype": "f64", "data": "synthetic"}
    coef = (3 * (a.levels - 1) + 1) * size * size
    out["cstep_model_us_at_peak"] = 1e6 * 32 * coef / HBM_PEAK           # four coefficient arrays, 32 B per coefficient
    out["astep_model_us_at_peak"] = 1e6 * 40 * coef / HBM_PEAK           # five coefficient arrays, 40 B per coefficient
    if a.only in (None, "driver", "composed"):
        f = driver(5)                                        # warm-up, and the two must be the same iteration
        c = composed(yd, op, a.mu1, a.mu2, eps, 6)
        out["criterion_rel_diff"] = float(np.max(np.abs(f[6][1:] / c[1] - 1.0)))
        out["objective_rel_diff"] = float(np.max(np.abs(f[3][1:] / c[2] - 1.0)))
        out["x_max_abs_diff"] = float(torch.max(torch.abs(f[0] - c[0])))
    if a.only in (None, "driver", "drivers"):
        driver(5)
        ts = timed(lambda: driver(a.steps), a.rounds)
        out["driver_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["driver_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
        out["driver_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps
    if a.only in (None, "composed"):
        ts = timed(lambda: composed(yd, op, a.mu1, a.mu2, eps, a.steps + 1), a.rounds)
        out["composed_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["composed_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only is None:
        out["composed_over_driver"] = out["composed_ms_per_iteration_median"] / out["driver_ms_per_iteration_median"]
    if a.only in (None, "analysis", "drivers"):
        analysis(5)
        ts = timed(lambda: analysis(a.steps), a.rounds)
        out["analysis_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["analysis_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
        out["analysis_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps
    print(json.dumps(out), flush=True)
