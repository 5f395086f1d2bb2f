#!/usr/bin/env python3
"""Masked-observation SAPG (`sbtv.SAPG_masked`, chambolleit 25, Philox normals, no warm-up): ms per iteration in both iteration
shapes - a PSF parameter free (new spectra, B X and the residual formed twice) and the PSF fixed (the residual of the sums is the
next gradient's input) - next to the ms per iteration of the circular loop (`sbtv.SAPG_algorithm_laplace` / `_moffat`) on the
same data in the same process, and `over_circular`, their ratio.  `--shapes` lists size:chains pairs (512:1 1024:8).
Device-resident images (tests/golden/man_512.npy, tiled), demo_setup of the family, the demo's step scales times `--scale`,
a valid mask of the 7 x 7 PSF.  Every shape is warmed up, then `--rounds` (5) timed runs of `--steps` iterations each: `best3` is
the best of the first three, `spread` is (max - min) / median of all.  One JSON line per shape.  `--only masked` / `--only
circular` times one of the two alone; SBTV_PACKAGE_DIR names the package directory of another checkout (its sbtv/ and lib/),
so that `--only circular` measures the circular loop of a commit without the masked entries in the same session.

`--demo N`: instead, the end-to-end run on a 256 x 256 crop of tests/golden/man_512.npy blurred LINEARLY with the true PSF (an
explicit valid convolution, no wrap-round), noise of BSNR 30 dB added, embedded with sbtv.embed_observation: the EB estimates of
`SAPG_masked` (N samples, warm-up N/10, burn-in N/2) next to those of the circular `SAPG_algorithm_*` on the same embedded
observation, and the PSNR over the observed pixels of `SALSA_masked` at each set of estimates (tau = theta_EB sigma2_EB, the PSF
at its EB parameters)."""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SBTV_PACKAGE_DIR") or os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np, torch, sbtv

FAMILY = {"laplace": dict(names=("b",), init=(0.1,), pmin=(1e-3,), pmax=(1.0,), c=dict(theta=0.01, b=100.0, sigma=1e4),
                          fn=sbtv.SAPG_algorithm_laplace),
          "moffat": dict(names=("alpha", "beta"), init=(1.0, 10.0), pmin=(1e-2, 0.1), pmax=(1.0, 10.0),
                         c=dict(theta=0.1, alpha=10.0, beta=1e4, sigma=1e4), fn=sbtv.SAPG_algorithm_moffat)}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, nargs="+", default=[200, 30], help="iterations per timed run, one value per shape")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--shapes", nargs="+", default=["512:1", "1024:8"], help="size:chains")
ap.add_argument("--kind", default="moffat", choices=sorted(FAMILY))
ap.add_argument("--scale", type=float, default=1.0, help="factor on the demo's c_theta, c_p and c_sigma")
ap.add_argument("--only", default=None, help="masked | circular: that part alone")
ap.add_argument("--demo", type=int, default=0, help="samples of the end-to-end run (0: the timing runs)")
a = ap.parse_args()
ctx = sbtv.default_context(0)
fam = FAMILY[a.kind]
T = 7


def timed(fn, rounds, steps):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ms = [1e3 * t / steps for t in ts]
    return {"best3": min(ms[:3]), "median": statistics.median(ms), "min": min(ms), "max": max(ms),
            "spread": (max(ms) - min(ms)) / statistics.median(ms)}


def options(st, fixed=False, **kw):
    op = dict(warmup=0, burnIn=1, psf_size=T, phi=0.0, gamma=st["gamma"], th_init=0.01, min_th=1e-3, max_th=1.0, sigma=st["sigma"],
              sigma_init=st["sigma_init"], sigma_min=st["sigma_min"], sigma_max=st["sigma_max"], d_scale=1.0, d_exp=0.8,
              fix_sigma=0, seed=1)
    op["lambda"] = st["lambda"]
    for q, nm in enumerate(fam["names"]):
        op[nm], op[nm + "_init"], op["min_" + nm], op["max_" + nm], op["fix_" + nm] = st["p_true"][q], fam["init"][q], fam["pmin"][q], fam["pmax"][q], int(fixed)
    op.update(kw)
    return op


def valid_convolution(x, taps):
    """'valid' part of the LINEAR convolution of x with the taps, as an explicit sum (tests/masked_restatement.py)."""
    t = taps.shape[0]
    M, N = x.shape
    out = np.zeros((M - t + 1, N - t + 1))
    for i in range(t):
        for j in range(t):
            out += taps[i, j] * x[t - 1 - i:M - i, t - 1 - j:N - j]
    return out


def psnr_over(mask, x_true, x):
    sel = np.asarray(mask) > 0
    return 10.0 * math.log10(255.0 ** 2 / float(np.mean((x_true[sel] - x[sel]) ** 2)))


if a.demo:
    x = np.load(os.path.join(ROOT, "tests", "golden", "man_512.npy")).astype(np.float64)[128:384, 128:384]
    # demo_setup for the noise level, lambda and gamma of the family; its circular y is not used
    st = sbtv.demo_setup(a.kind, x, np.zeros_like(x), evMax=0.99, ctx=ctx)
    taps = np.asarray(sbtv.psf_family(a.kind, T, st["p_true"])[0])
    y_obs = valid_convolution(x, taps)
    y_obs = y_obs + st["sigma"] * np.random.default_rng(1).standard_normal(y_obs.shape)
    y, mask = sbtv.embed_observation(y_obs, T, shape=x.shape)
    S = a.demo
    c = dict({k: a.scale * v for k, v in fam["c"].items()}, lam=1.0, gam=1.0)
    op = options(st, samples=S, warmup=max(S // 10, 1), burnIn=max(S // 2, 1))
    out = {"demo": "man_512[128:384, 128:384]", "kind": a.kind, "samples": S, "scale": a.scale, "n_obs": int(mask.sum()),
           "true": dict({nm: st["p_true"][q] for q, nm in enumerate(fam["names"])}, sigma2=st["sigma"] ** 2)}
    x0 = np.where(mask > 0, y, float(np.mean(y_obs)))            # the same start for both loops: the unobserved border at the mean
    for tag, run in (("masked", lambda: sbtv.SAPG_masked(a.kind, y, mask, op, c, x0=x0, ctx=ctx)),
                     ("circular", lambda: fam["fn"](y, op, c, x0=x0, ctx=ctx))):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        est = dict(theta=float(r[0]), sigma2=float(r[-2]), **{nm: float(r[1 + q]) for q, nm in enumerate(fam["names"])})
        A = sbtv.BlurOperator(sbtv.psf_family(a.kind, T, [est[nm] for nm in fam["names"]])[0], ctx=ctx)
        xs = sbtv.SALSA_masked(y, A, mask, est["theta"] * est["sigma2"], "MU1", est["theta"] / 10, "AT", A.T, "MAXITERA", 300,
                               "TOLERANCEA", 1e-5, "INITIALIZATION", 2, ctx=ctx)[0]
        # the image the observation saw: x itself, where the embedded observation sits
        out[tag] = dict(estimates=est, seconds=time.perf_counter() - t0, psnr_salsa_masked=psnr_over(mask, x, np.asarray(xs)))
    print(json.dumps(out), flush=True)
    sys.exit(0)

for shape, steps in zip(a.shapes, a.steps + a.steps[-1:] * len(a.shapes)):
    size, chains = (int(v) for v in shape.split(":"))
    img = np.load(os.path.join(ROOT, "tests", "golden", "man_512.npy")).astype(np.float64)
    r = max(1, size // img.shape[0])
    x = np.tile(img, (r, r))[:size, :size]
    st = sbtv.demo_setup(a.kind, x, np.random.default_rng(1).standard_normal(x.shape), evMax=0.99, ctx=ctx)
    yd = sbtv.to_device(np.repeat(st["y"][None], chains, axis=0) if chains > 1 else st["y"])
    md = sbtv.to_device(np.repeat(sbtv.valid_mask(x.shape, T)[None], chains, axis=0) if chains > 1 else sbtv.valid_mask(x.shape, T))
    c = dict({k: a.scale * v for k, v in fam["c"].items()}, lam=1.0, gam=1.0)
    out = {"size": size, "chains": chains, "kind": a.kind, "steps": steps, "rounds": a.rounds, "dtype": "f64", "noise": "philox",
           "scale": a.scale, "package": os.environ.get("SBTV_PACKAGE_DIR", "this checkout")}
    for fixed in (False, True):
        tag = "psf_fixed" if fixed else "psf_free"
        if a.only in (None, "circular"):
            run = lambda n: fam["fn"](yd, options(st, fixed, samples=n + 1), c, ctx=ctx)
            run(3)                                                                               # warm-up
            out[f"circular_{tag}_ms_per_iteration"] = timed(lambda: run(steps), a.rounds, steps)
        if a.only in (None, "masked"):
            run = lambda n: sbtv.SAPG_masked(a.kind, yd, md, options(st, fixed, samples=n + 1), c, ctx=ctx)
            run(3)                                                                               # warm-up
            r = timed(lambda: run(steps), a.rounds, steps)
            if f"circular_{tag}_ms_per_iteration" in out:
                r["over_circular"] = r["median"] / out[f"circular_{tag}_ms_per_iteration"]["median"]
            out[f"masked_{tag}_ms_per_iteration"] = r
    print(json.dumps(out), flush=True)
