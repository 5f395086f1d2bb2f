#!/usr/bin/env python3
"""SALSA/run_deblur_synthesis_L1.m end to end on the MI355X through the host mirror: 9 x 9 uniform blur at BSNR 30 ->
empirical-Bayes estimate of theta for the Laplace prior on the coefficients of the redundant 4-level Haar frame
(`sbtv.SAPG_wavelet`, :125-156) -> MAP image by `sbtv.SALSA_wavelet` at tau = theta_EB sigma^2, mu = theta_EB (:160-185).
With `--posterior S` also S samples of the posterior at theta_EB (`sbtv.myula_wavelet`, started at the MAP coefficients): the
MMSE image next to the MAP image, and the per-pixel standard deviation; `--out DIR` is where both are saved (.npy and .pgm).
`--sampler skrock` draws them with `sbtv.skrock_wavelet` instead (`--stages` gradient evaluations per sample, `--delta` or
0.8 of the stability bound), and prints ||X||_1 of the first and the last sample.
With `--semiblind KIND` (gaussian, moffat or laplace) the blur is NOT given to the estimator: the image is blurred with the
7 x 7 PSF of the family at its true parameters, `sbtv.SAPG_wavelet_semiblind` estimates (theta, p) from one chain with sigma^2
known, the taps are rebuilt from p_EB, `sbtv.SALSA_wavelet` solves with them, and the estimates are printed next to the
true values with the PSNR.

  python tools/run_wavelet_demo.py [--image tests/golden/man_512.npy] [--samples 3000] [--seed 1] [--posterior S] [--out DIR]
                                   [--sampler skrock --stages 10 [--delta D]]
  python tools/run_wavelet_demo.py --semiblind laplace [--samples 3000] [--seed 1]

Constants follow the script (:65-83,99,106-107,164-166).  The reference's uniform_blur is centred; the library's taps sit in
the top-left corner (utils/resize.m), which delays the blurred image by 4 pixels in both directions.  The observation is made
with the centred blur, as the script makes it, the solver is given the 9 x 9 taps, so its estimate is the image advanced by 4
pixels: it is rolled back before the MSE.  A non-negative mask of unit sum has spectral norm 1 (|H| <= H(0) = 1), which is
what the script's power iteration (:101) returns.  MATLAB's randn('state',1) stream cannot be reproduced: noise comes from
NumPy (observation) and the device Philox generator (MYULA)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semi-blind-image-deblurring-problems-with-tv_amd"))
import numpy as np
import sbtv


# --semiblind: true parameters, start values, bounds (run_*_demo.m, as sbtv_oracle.DEMO lists them) and step scales c_p
SEMIBLIND = {
    "gaussian": dict(true=(0.4, 0.3), init=(0.7, 0.6), pmin=(0.1, 0.1), pmax=(1.0, 1.0), c_p=(1.0, 1.0)),
    "moffat": dict(true=(0.4, 3.5), init=(0.6, 3.5), pmin=(1e-2, 0.1), pmax=(1.0, 10.0), c_p=(1.0, 1.0), fix=(False, True)),
    "laplace": dict(true=(0.3,), init=(0.1,), pmin=(1e-3,), pmax=(1.0,), c_p=(10.0,)),
}


def semiblind(a, x, ctx):
    """(theta, p) from one chain with sigma^2 known, then the MAP image with the taps of p_EB."""
    kind, d = a.semiblind, SEMIBLIND[a.semiblind]
    dimX, t, levels, bsnr = x.size, 7, 4, 30.0
    rng = np.random.default_rng(a.seed)
    h = sbtv.daubcqf(2)
    c = t // 2
    pad = np.zeros(x.shape)
    pad[:t, :t] = sbtv.psf_family(kind, t, d["true"])[0]
    Bx = np.real(np.fft.ifft2(np.fft.fft2(np.roll(pad, (-c, -c), axis=(0, 1))) * np.fft.fft2(x)))    # the centred blur
    sigma = np.linalg.norm(Bx - Bx.mean()) / math.sqrt(dimX * 10 ** (bsnr / 10))
    y = Bx + sigma * rng.standard_normal(x.shape)
    Lf = (1.0 / sigma) ** 2
    lam = min(5.0 / Lf, 2.0)
    op = {"samples": a.samples, "burnIn": min(20, a.samples), "th_init": 0.01, "min_th": 1e-3, "max_th": 1.0, "d_exp": 0.8,
          "d_scale": 0.1 / 0.01, "warmup": 0, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam), "sigma": sigma, "seed": a.seed,
          "p_init": d["init"], "p_true": d["true"], "p_min": d["pmin"], "p_max": d["pmax"], "c_p": d["c_p"],
          "fix_p": d.get("fix", (False,) * len(d["true"])), "fix_sigma": True}
    print(f"image {x.shape}, {kind} PSF {t} x {t} at {d['true']}, sigma {sigma:.4f}, {a.samples} samples from p = {d['init']}")
    t0 = time.perf_counter()
    eb, res = sbtv.SAPG_wavelet_semiblind(y, kind, h, levels, op, ctx=ctx)
    t_eb = time.perf_counter() - t0
    print(f"theta_EB {eb['theta']:.6g} (last {res['last_theta']:.6g}) in {t_eb:.2f} s")
    for q, (pe, pt) in enumerate(zip(eb["p"], d["true"])):
        print(f"p{q}_EB {pe:.6g}   true {pt:.6g}   last {res['ps'][q, -1]:.6g}   last relative change of the mean "
              f"{res['tol_ps'][q, -1]:.2e}")
    A = sbtv.BlurOperator(sbtv.psf_family(kind, t, tuple(eb["p"]))[0], ctx=ctx)
    out = sbtv.SALSA_wavelet(y, A, eb["theta"] * sigma ** 2, "MU", eb["theta"], "WAVELET", h, "LEVELS", levels, "AT", A.T,
                             "TOLERANCEA", 1e-4, "MAXITERA", 500, "VERBOSE", 0, ctx=ctx)
    xMAP = np.roll(np.asarray(out[1]), (c, c), axis=(0, 1))              # the taps sit in the top-left corner: roll back
    At = sbtv.BlurOperator(sbtv.psf_family(kind, t, d["true"])[0], ctx=ctx)
    ref = sbtv.SALSA_wavelet(y, At, eb["theta"] * sigma ** 2, "MU", eb["theta"], "WAVELET", h, "LEVELS", levels, "AT", At.T,
                             "TOLERANCEA", 1e-4, "MAXITERA", 500, "VERBOSE", 0, ctx=ctx)
    xREF = np.roll(np.asarray(ref[1]), (c, c), axis=(0, 1))
    print(f"SALSA_wavelet with the taps of p_EB: PSNR {sbtv.PSNR(x, xMAP, ctx=ctx):.2f} dB; with the true taps "
          f"{sbtv.PSNR(x, xREF, ctx=ctx):.2f} dB; observation {sbtv.PSNR(x, y, ctx=ctx):.2f} dB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default=os.path.join(ROOT, "tests", "golden", "man_512.npy"))
    ap.add_argument("--samples", type=int, default=3000)                 # op.samples (:65)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--posterior", type=int, default=0, metavar="S",
                    help="after theta_EB, S MYULA samples at theta_EB: MMSE image and standard-deviation map")
    ap.add_argument("--posterior-first", type=int, default=0, help="first iteration used (default: S / 10 + 1)")
    ap.add_argument("--sampler", default="myula", choices=("myula", "skrock"), help="the sampler of --posterior")
    ap.add_argument("--stages", type=int, default=10, help="skrock: gradient evaluations per sample")
    ap.add_argument("--delta", type=float, default=None, help="skrock: step (default: 0.8 of the stability bound)")
    ap.add_argument("--out", default=os.path.join(ROOT, "out"), help="directory for the mean / standard-deviation maps")
    ap.add_argument("--semiblind", default=None, choices=sorted(SEMIBLIND), metavar="KIND",
                    help="estimate (theta, p) of this PSF family with sigma^2 known instead of taking the blur as given")
    a = ap.parse_args()
    x = np.load(a.image).astype(np.float64)
    if a.semiblind:
        return semiblind(a, x, sbtv.default_context(0))
    dimX = x.size
    rng = np.random.default_rng(a.seed)
    ctx = sbtv.default_context(0)
    blur_length, levels, bsnr = 9, 4, 30.0                               # :99,107,88
    h = sbtv.daubcqf(2)                                                  # :106
    taps = np.full((blur_length, blur_length), 1.0 / blur_length ** 2)
    c = blur_length // 2
    pad = np.zeros(x.shape)
    pad[:blur_length, :blur_length] = taps
    Hc = np.fft.fft2(np.roll(pad, (-c, -c), axis=(0, 1)))                # the centred blur of uniform_blur.m
    Bx = np.real(np.fft.ifft2(Hc * np.fft.fft2(x)))                      # :120
    sigma = np.linalg.norm(Bx - Bx.mean()) / math.sqrt(dimX * 10 ** (bsnr / 10))     # :121
    y = Bx + sigma * rng.standard_normal(x.shape)                        # :123
    evMax = 1.0
    Lf = (evMax / sigma) ** 2                                            # :143
    lam = min(5.0 / Lf, 2.0)                                             # :80-81,149
    op = {"samples": a.samples, "burnIn": min(20, a.samples), "th_init": 0.01, "min_th": 1e-3, "max_th": 1.0, "d_exp": 0.8,
          "d_scale": 0.1 / 0.01, "warmup": 0, "lambda": lam, "gamma": 0.98 / (Lf + 1.0 / lam), "sigma": sigma,
          "seed": a.seed}                                                # :65-83,150
    A = sbtv.BlurOperator(taps, ctx=ctx)
    print(f"image {x.shape}, sigma {sigma:.4f}, lambda {lam:.4g}, gamma {op['gamma']:.4g}, {a.samples} samples")
    t0 = time.perf_counter()
    theta_EB, res = sbtv.SAPG_wavelet(y, A, h, levels, op, ctx=ctx)      # :153-156
    t_eb = time.perf_counter() - t0
    print(f"theta_EB {theta_EB:.6g} (last theta {res['last_theta']:.6g}, last relative change of the mean "
          f"{res['tol_thetas'][-1]:.2e}) in {t_eb:.2f} s")
    WTx = sbtv.mrdwt_TI2D(np.roll(x, (-c, -c), axis=(0, 1)), h, levels, ctx=ctx)    # the true coefficients of what is estimated
    t0 = time.perf_counter()
    out = sbtv.SALSA_wavelet(y, A, theta_EB * sigma ** 2, "MU", theta_EB, "WAVELET", h, "LEVELS", levels, "AT", A.T,
                             "TRUE_X", WTx, "TOLERANCEA", 1e-4, "MAXITERA", 500, "VERBOSE", 0, ctx=ctx)    # :164-182
    t_map = time.perf_counter() - t0
    xMAP = np.roll(np.asarray(out[1]), (c, c), axis=(0, 1))              # :184, rolled back by 4 pixels
    mse = 10 * math.log10(np.linalg.norm(x - xMAP) ** 2 / dimX)          # :185
    print(f"SALSA_wavelet: {len(out[4]) - 1} outer iterations in {t_map:.2f} s, MSE {mse:.2f} dB "
          f"(observation: {10 * math.log10(np.linalg.norm(x - y) ** 2 / dimX):.2f} dB)")
    print(f"wall time {t_eb + t_map:.2f} s")
    if a.posterior >= 2:
        first = a.posterior_first or a.posterior // 10 + 1
        t0 = time.perf_counter()
        if a.sampler == "skrock":
            pop = {"samples": a.posterior, "stages": a.stages, "lambda": lam, "delta": a.delta, "seed": a.seed + 1}
            post = sbtv.skrock_wavelet(y, A, h, levels, pop, theta=theta_EB, sigma2=sigma ** 2, xw0=np.asarray(out[0]),
                                       posterior=dict(first=first), ctx=ctx)
        else:
            pop = {"samples": a.posterior, "lambda": lam, "gamma": op["gamma"], "seed": a.seed + 1}
            post = sbtv.myula_wavelet(y, A, h, levels, pop, theta=theta_EB, sigma2=sigma ** 2, xw0=np.asarray(out[0]),
                                      posterior=dict(first=first), ctx=ctx)
        t_post = time.perf_counter() - t0
        xMMSE = np.roll(np.asarray(post["posteriormean"]), (c, c), axis=(0, 1))
        sd = np.roll(np.sqrt(np.asarray(post["posteriorvar"])), (c, c), axis=(0, 1))
        mmse = 10 * math.log10(np.linalg.norm(x - xMMSE) ** 2 / dimX)
        err = np.abs(x - xMMSE)
        if a.sampler == "skrock":
            delta = a.delta if a.delta is not None else 0.8 * sbtv.skrock_max_step(a.stages, 0.05, sigma ** 2, lam)
            print(f"skrock_wavelet: {a.stages} stages, delta {delta:.4g} ({delta / op['gamma']:.1f} gamma); ||X||_1 of the first "
                  f"sample {post['gXTrace'][0]:.6g}, of the last {post['gXTrace'][-1]:.6g}")
        print(f"{a.sampler}_wavelet at theta_EB: {a.posterior} samples in {t_post:.2f} s, iterations {first}.. used "
              f"({post['posteriorcount']}); MSE of the MMSE image {mmse:.2f} dB (MAP {mse:.2f} dB); standard deviation: "
              f"mean {sd.mean():.3f}, max {sd.max():.3f}; correlation of |x - MMSE| with it {np.corrcoef(err.ravel(), sd.ravel())[0, 1]:.2f}")
        os.makedirs(a.out, exist_ok=True)
        np.save(os.path.join(a.out, "wavelet_posterior_mean.npy"), xMMSE)
        np.save(os.path.join(a.out, "wavelet_posterior_std.npy"), sd)
        sbtv.save_image(os.path.join(a.out, "wavelet_posterior_mean.pgm"), xMMSE, 0.0, 255.0)
        sbtv.save_image(os.path.join(a.out, "wavelet_posterior_std.pgm"), sd)
        print(f"saved mean and standard-deviation maps under {a.out}")


if __name__ == "__main__":
    main()
