#!/usr/bin/env python3
"""Wavelet-l1 deconvolution (`sbtv.SALSA_wavelet`, Haar, levels 4 unless told otherwise): time per outer iteration of the
fused driver against the SAME iteration composed in Python from the entry points (`sbtv.soft`, `sbtv.mirdwt_TI2D`,
`sbtv.mrdwt_TI2D`, the A / AT / invLS calls of `sbtv.BlurOperator`, i.e. sbtv_A_wrapper) and torch arithmetic on device
tensors, and the two transforms alone against their byte model (5 * M N * 8 bytes per level).  Device-resident images of
the bench's problem, K outer iterations with an unreachable tolerance; every shape is warmed up first, then `--rounds`
timed runs of each; one JSON line per size with the median and the best run."""
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
ap.add_argument("--only", default=None, help="fused | composed | transforms: that part alone (e.g. under a profiler)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
h = sbtv.daubcqf(a.wavelet)
J = a.levels - 1
HBM_PEAK = bench.HBM_PEAK_GBS * 1e9              # the peak every byte-model fraction of this project is taken against


def composed(yd, op, tau, mu, K):
    """The operator form of include/sbtv.h (sbtv_SALSA_wavelet), one library call or torch expression per line."""
    ATy = op.AT(yd)
    xw = sbtv.mrdwt_TI2D(ATy, h, a.levels, ctx=ctx)
    bu = torch.zeros_like(xw)
    obj = []
    for _ in range(K):
        u = sbtv.soft(xw - bu, tau / mu, ctx=ctx)
        s = u + bu
        z = sbtv.mirdwt_TI2D(s, h, a.levels, ctx=ctx)
        xi = op.invLS(ATy + mu * z, mu)
        we = sbtv.mrdwt_TI2D(xi - z, h, a.levels, ctx=ctx)
        xw = s + we
        bu = -we
        r = yd - op.A(xi)
        obj.append(0.5 * torch.sum(r * r) + tau * torch.sum(torch.abs(u)))
    return xw, torch.stack(obj).cpu().numpy()


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
    fused = lambda K: sbtv.SALSA_wavelet(yd, op, tau, "MU", mu, "WAVELET", h, "LEVELS", a.levels, "AT", op.T, "STOPCRITERION", 1,
                                         "TOLERANCEA", -1.0, "MAXITERA", K, "INITIALIZATION", 2, ctx=ctx)
    out = {"size": size, "wavelet": a.wavelet, "levels": a.levels, "steps": a.steps, "rounds": a.rounds, "dtype": "f64",
           "data": "synthetic"}
    if a.only in (None, "fused", "composed"):
        f = fused(5)                                         # warm-up, and the two must be the same iteration
        c = composed(yd, op, tau, mu, 5)
        out["objective_rel_diff"] = float(np.max(np.abs(f[4][1:] / c[1] - 1.0)))
    if a.only in (None, "fused"):
        ts = timed(lambda: fused(a.steps), a.rounds)
        out["fused_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["fused_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
        out["fused_loop_ms_per_iteration"] = ctx.last_timing()["loop_ms"] / a.steps
    if a.only in (None, "composed"):
        ts = timed(lambda: composed(yd, op, tau, mu, a.steps), a.rounds)
        out["composed_ms_per_iteration_median"] = 1e3 * statistics.median(ts) / a.steps
        out["composed_ms_per_iteration_best"] = 1e3 * min(ts) / a.steps
    if a.only in (None, "transforms"):
        z = sbtv.mrdwt_TI2D(yd, h, a.levels, ctx=ctx)
        sbtv.mirdwt_TI2D(z, h, a.levels, ctx=ctx)
        reps = 20
        model = J * 5 * size * size * 8                     # bytes: each level reads one image and writes four (or the mirror)
        for name, fn in (("analysis", lambda: [sbtv.mrdwt_TI2D(yd, h, a.levels, ctx=ctx) for _ in range(reps)]),
                         ("synthesis", lambda: [sbtv.mirdwt_TI2D(z, h, a.levels, ctx=ctx) for _ in range(reps)])):
            t = statistics.median(timed(fn, a.rounds)) / reps
            out[name + "_us"] = 1e6 * t
            out[name + "_fraction_of_byte_model"] = (model / HBM_PEAK) / t
    print(json.dumps(out), flush=True)
