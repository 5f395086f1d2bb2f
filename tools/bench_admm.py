#!/usr/bin/env python3
"""Secondary benchmark: outer iterations/s of the ADMM front-ends beside SALSA_v2: C-SALSA
(`sbtv.csalsa`, SALSA/CSALSA_v2.m), CoRAL (`sbtv.CoRAL`, SALSA/CoRAL_v2.m) and the masked-observation SALSA
(`sbtv.SALSA_masked`, frame mask of `sbtv.valid_mask`), on the bench's 2048 x 2048 problem (and 512 x 512), device-resident
images, K outer iterations with an unreachable tolerance.  Every configuration of every size is warmed up first; the timed
rounds then alternate between the configurations (--only NAME: that configuration alone, e.g. under a profiler).  One JSON
line per configuration and size: the best round's wall time per iteration and the device time of its loop."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv, bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 512])
ap.add_argument("--only", default=None, help="run this configuration alone (SALSA_v2, csalsa, CoRAL, masked)")
a = ap.parse_args()
ctx = sbtv.default_context(0)


def configs(size):
    x, y, sigma, noise = bench.make_problem(1, size)
    yd, xd = sbtv.to_device(y), sbtv.to_device(x)
    op = sbtv.BlurOperator(sbtv.Gaussian_psf(7, *bench.W_TRUE), ctx=ctx)
    theta, s2 = bench.THETA, sigma ** 2
    m = sbtv.valid_mask((size, size), 7)
    md, ymd = sbtv.to_device(m), sbtv.to_device(y * m)
    common = ("STOPCRITERION", 1, "TOLERANCEA", -1.0, "TRUE_X", xd, "VERBOSE", 0)
    runs = {
        "SALSA_v2": lambda K: sbtv.SALSA_v2(yd, op, theta * s2, "MU", theta / 10, "AT", op.T, "LS", op.LS(theta / 10),
                                            "TVINITIALIZATION", 1, "TVITERS", 10, "MAXITERA", K, *common, ctx=ctx),
        "csalsa": lambda K: sbtv.csalsa(yd, op, 1.0, 1.0, sigma, "AT", op.T, "LS", op.invLS, "TVINITIALIZATION", 1, "TVITERS", 10,
                                        "MAXITERA", K, *common, ctx=ctx),
        "CoRAL": lambda K: sbtv.CoRAL(yd, op, 0.5 * theta * s2, 0.5 * theta * s2, "MU1", theta / 20, "MU2", theta / 20, "AT", op.T,
                                      "LS", op.LS(theta / 10), "TVINITIALIZATION1", 1, "TVITERS1", 10, "TVINITIALIZATION2", 1,
                                      "TVITERS2", 10, "MAXITERA", K, *common, ctx=ctx),
        "masked": lambda K: sbtv.SALSA_masked(ymd, op, md, theta * s2, "MU1", theta / 10, "MU2", 0.1, "AT", op.T, "TVITERS", 10,
                                              "MAXITERA", K, *common, ctx=ctx),
    }
    if a.only:
        runs = {a.only: runs[a.only]}
    return runs


all_runs = {size: configs(size) for size in a.sizes}
for size, runs in all_runs.items():                      # warm-up of every shape: plans, workspaces, twiddles, clocks
    for fn in runs.values():
        fn(20)
torch.cuda.synchronize()
for size, runs in all_runs.items():
    best = {name: (1e9, 0.0, 0) for name in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            t0 = time.perf_counter(); out = fn(a.steps); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if dt < best[name][0]:
                best[name] = (dt, ctx.last_timing()["loop_ms"], len(out[3]) - (0 if name == "csalsa" else 1))
    for name, (dt, loop_ms, n) in best.items():
        print(json.dumps({"metric": f"{name} outer iterations/s (TV, TViters 10), {size}x{size} Gaussian blur", "value": a.steps / dt,
                          "unit": "outer iterations/s", "n_gpus": 1, "ms_per_iteration": 1e3 * dt / a.steps,
                          "loop_ms_per_iteration": loop_ms / a.steps, "steps": a.steps, "objective_entries": n, "dtype": "f64",
                          "data": "synthetic", "higher_is_better": True}), flush=True)
