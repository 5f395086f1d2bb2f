"""The parameter-estimation problems at PSF sizes other than 7 x 7 and with a rotated Gaussian, shared by
tests/test_psf_sizes_cpu.py and tests/test_gpu_psf_sizes.py.  Data synthesis as tests/wavelet_sapg_cases._setup: a
sbtv_oracle.BlurModel of the case's size and phi, the BSNR formulas of sbtv_oracle.demo_setup (BSNR 30, evMax 0.99 for the TV
loops, 1.0 for the wavelet loop) for sigma, sigma_min, sigma_max and the step sizes, synth_image.  Injected noise, every PSF
parameter free, start values away from the bounds.  Each reference (sbtv_oracle.SAPG_algorithm / SAPG_algorithm_shared, or
tests/wavelet_sb_restatement.literal) is computed once per session and never modified.

The step constants.  sbtv_oracle.DEMO[kind]["c_p"] belongs to 7 x 7 masks on 512 x 512 images; on these small images and with
masks of 8 x 8 and more it throws every free parameter onto a bound within three iterations, after which the taps are rebuilt
from a constant and nothing is tested.  `scale` multiplies DEMO's c_p (for the wavelet cases `c_p` is the constant itself).
Each value was found by running the reference at powers of ten (T5: 3e-5, between the 1e-4 that throws b onto p_min at
12 x 12 and 1e-5) and keeping one at which, over the whole run, every parameter stays strictly inside its bounds, every step
moves it by 1e-4 relative or more, and a 1e-15 perturbation of y stays 100 times below every bar of the GPU tests;
tests/test_psf_sizes_cpu.py asserts all of it on the cached references.  What the search saw at the next larger power of ten:
T4, T5, T6, T7, T9, W1 leave the bounds; T2, T3, T8, W2 stay inside (the Gaussian scale is the one found for 8 x 8 and more with
a rotation); W3 at c_p = 1 is 70 times worse conditioned.  The wavelet loop's c_sigma = 1 keeps sigma2 moving for the
whole run (at the 1000 of tests/wavelet_sb_cases.py it sits on sigma2_max from the second iteration on)."""
import functools
import math

import numpy as np

from conftest import synth_image

import wavelet_cases as wc
import wavelet_sapg_cases as wsc
import wavelet_sb_restatement as wsb

SAMPLES, WARMUP, BURNIN, CHAMBOLLEIT = 12, 4, 4, 25
P_INIT = {"gaussian": (0.55, 0.45), "moffat": (0.6, 5.0), "laplace": (0.2,)}
NAMES = {"gaussian": ("w1", "w2"), "moffat": ("alpha", "beta"), "laplace": ("b",)}

# name: kind, PSF size, phi, chains, share_gradients, (M, N), scale of DEMO[kind]["c_p"], noise seed     what it reaches
# (the default policy deals T6's two chains to two lanes, one spectrum set each: the GPU tests run it with the lanes off as well)
TV_CASES = {
    "T1": ("gaussian", 3, 0.0, 1, False, (48, 32), 1.0, 41),       # wave branch, 9 lanes
    "T2": ("gaussian", 8, 0.6, 1, False, (48, 32), 0.01, 42),      # wave branch, all 64 lanes, even size, rotation
    "T3": ("gaussian", 9, 0.6, 1, False, (48, 32), 0.01, 43),      # block branch, first size
    "T4": ("moffat", 15, 0.0, 1, False, (48, 32), 0.001, 44),      # block branch, 225 lanes, pow / log
    "T5": ("laplace", 12, 0.0, 1, False, (48, 32), 3e-5, 45),      # block branch, npar = 1, D2s = D1s
    "T6": ("moffat", 5, 0.0, 2, False, (48, 32), 0.01, 46),        # wave branch, 25 lanes; nspec = 2 with the lanes off
    "T7": ("laplace", 3, 0.0, 6, False, (48, 32), 0.01, 47),       # lanes off: second trip of `sset += 4`
    "T8": ("gaussian", 9, 0.3, 3, True, (48, 32), 0.01, 48),       # nspec = 1 < batch on the block branch
    "T9": ("gaussian", 11, 0.6, 1, False, (34, 30), 0.01, 49),     # chirp-z plan: any_psf_spectrum_kernel, three sets
}

# name: kind, PSF size, phi, start values per chain, (M, N), c_p, noise seed; Haar, 3 levels, samples 6, warmup 0
WAV_CASES = {
    "W1": ("gaussian", 9, 0.6, [(0.55, 0.45)], (34, 30), (0.01, 0.01), 51),
    "W2": ("moffat", 15, 0.0, [(0.6, 5.0)], (64, 64), (0.001, 1.0), 52),           # 225 lanes, g0_scale
    "W3": ("laplace", 3, 0.0, [(0.2,), (0.35,)], (64, 64), (0.1,), 53),           # two chains, two sets of taps
}
WAV_SAMPLES, WAV_BURNIN, WAV_LEVELS, WAV_C_SIGMA = 6, 3, 3, 1.0

# (key, rtol, atol) of tests/test_gpu_sapg_fista.py::test_sapg_matches_oracle_with_injected_noise, and grad_theta at the bar of
# test_sapg_shared_gradient_chains_match_oracle; gXTrace without its last entry, the warm-up trace and the gradients without
# their first (neither side writes them)
TV_BARS = (("thetas", 1e-9, 0.0), ("sigmas", 1e-9, 0.0), ("logPiTraceX", 1e-9, 0.0), ("logPiTrace_WU", 1e-9, 0.0),
           ("ps", 1e-8, 0.0), ("grads_p", 1e-6, 1e-6), ("grad_theta", 1e-9, 0.0), ("err_psf", 1e-6, 1e-18), ("gXTrace", 1e-10, 0.0),
           ("Xlast_sample", 1e-8, 1e-8), ("theta_EB", 1e-9, 0.0), ("sigma_EB", 1e-9, 0.0))
# tests/test_gpu_wavelet_sb.py::_check: every trace, the EB estimates and max|X - ref| / max|X| to 1e-9
WAV_RTOL = 1e-9


def setup(kind, x, noise, psf_size, phi, evMax=0.99, BSNR=30.0):
    """sbtv_oracle.demo_setup for a PSF of another size and rotation: the same dict."""
    import sbtv_oracle as o
    d = o.DEMO[kind]
    p_true = tuple(d["true"])
    model = o.BlurModel(kind, x.shape, psf_size=psf_size, phi=phi)
    dimX = x.size
    Ax = model.A(x, *p_true)
    nrm = float(np.linalg.norm(Ax - np.mean(np.mean(Ax, axis=0)), "fro"))
    sigma = nrm / math.sqrt(dimX * 10 ** (BSNR / 10))
    sigma_min = nrm / math.sqrt(dimX * 10 ** (d["bsnr_min"] / 10))
    sigma_max = nrm / math.sqrt(dimX * 10 ** (d["bsnr_max"] / 10))
    y = Ax + sigma * noise
    lf = lambda s2: evMax ** 2 / s2
    Lf = (min if d["lf"] == "min" else max)(lf(sigma_min ** 2), lf(sigma_max ** 2))
    lam = min(5 / Lf, d["lambdaMax"])
    gamma = d["gamma_mult"] * d["gammaFrac"] * (1 / (Lf + 1 / lam))
    return dict(kind=kind, model=model, y=y, x=x, sigma=sigma, sigma_min=sigma_min ** 2, sigma_max=sigma_max ** 2,
                sigma_init=(sigma_min ** 2 + sigma_max ** 2) / 2, Lf=Lf, lam=lam, gamma=gamma, p_true=p_true, th_init=0.01,
                dimX=dimX, d_exp=0.8, d_scale=1.0, min_th=1e-3, max_th=1.0)


# ---- TV SAPG -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tv_problem(name):
    """dict(kind, size, phi, chains, shared, sts (one setup per image; they share image 0's step sizes and sigma2 settings, as one
    call has one option struct), c (the oracle's step constants), noise (steps, chains, M, N))."""
    import sbtv_oracle as o
    kind, size, phi, chains, shared, (M, N), scale, seed = TV_CASES[name]
    rng = np.random.default_rng(seed)
    sts = []
    for b in range(1 if shared else chains):
        st = setup(kind, synth_image(M, N, 4 + 5 * b), rng.standard_normal((M, N)), size, phi)
        if sts:
            for k in ("lam", "gamma", "sigma", "sigma_init", "sigma_min", "sigma_max"):
                st[k] = sts[0][k]
        sts.append(st)
    d = o.DEMO[kind]
    c = dict(theta=d["c_theta"], p=tuple(scale * v for v in d["c_p"]), sigma=d["c_sigma"])
    noise = rng.standard_normal((WARMUP - 1 + SAMPLES - 1, chains, M, N))
    return dict(kind=kind, size=size, phi=phi, chains=chains, shared=shared, sts=sts, c=c, noise=noise)


def _perturbed(y):
    """y (1 + 1e-15 r), r uniform in [-1, 1], fixed seed: the input of the conditioning check."""
    return y * (1.0 + 1e-15 * np.random.default_rng(99).uniform(-1.0, 1.0, y.shape))


def tv_run(p, perturb=False):
    """The oracle on problem p: one result per chain (shared gradients: per-chain views of SAPG_algorithm_shared's result), each
    with the keys of TV_BARS."""
    import sbtv_oracle as o
    kind, nz = p["kind"], p["noise"]
    npar = len(P_INIT[kind])
    kw = dict(samples=SAMPLES, warmup=WARMUP, burnIn=BURNIN, chambolleit=CHAMBOLLEIT, p_init=P_INIT[kind],
              fix=(False,) * npar, c=p["c"])
    sts = [dict(st, y=_perturbed(st["y"])) if perturb else st for st in p["sts"]]
    out = []
    if p["shared"]:
        step = [0] * p["chains"]

        def randn(shape, k):
            z = nz[step[k], k]
            step[k] += 1
            return z
        r = o.SAPG_algorithm_shared(sts[0], p["chains"], randn=randn, **kw)
        for k in range(p["chains"]):
            out.append(dict(r, logPiTraceX=r["logPiTraceX"][k], gXTrace=r["gXTrace"][k], Xlast_sample=r["Xlast_samples"][k]))
    else:
        for b, st in enumerate(sts):
            it = iter(nz[:, b])
            out.append(o.SAPG_algorithm(st, randn=lambda s: next(it), **kw))
    for r in out:
        r["grads_p"] = r["grads"][1:1 + npar]
        r["grad_theta"] = r["grads"][0]
    return out


@functools.lru_cache(maxsize=None)
def tv_reference(name, perturb=False):
    return tv_run(tv_problem(name), perturb)


def tv_compare(got, ref, tighten=1.0, label="", shared=False):
    """Every assertion of TV_BARS on one chain (`got` in the oracle's keys), each bar divided by `tighten`; returns the worst
    error of every key as a fraction of its bar, {key: (max|got - ref|, fraction)}."""
    worst = {}
    for key, rtol, atol in TV_BARS:
        if key not in ref or (shared and key == "logPiTrace_WU"):      # the shared-gradient oracle keeps no warm-up trace
            continue
        a, c = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        if key == "gXTrace":
            a, c = a[..., :-1], c[..., :-1]
        elif key in ("logPiTrace_WU", "grads_p", "grad_theta"):
            a, c = a[..., 1:], c[..., 1:]
        assert a.shape == c.shape, (key, a.shape, c.shape)
        assert np.all(np.isfinite(c)), key
        err, bar = np.abs(a - c), (atol + rtol * np.abs(c)) / tighten
        worst[key] = (float(np.max(err)), float(np.max(err / bar)) if np.all(bar > 0) else float(np.max(err) > 0))
        assert np.all(err <= bar), f"{label} {key}: max|got - ref| = {np.max(err):.3e}, {np.max(err / np.maximum(bar, 1e-300)):.3g} of the bar"
    return worst


# ---- wavelet semi-blind --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wav_problem(name):
    """The dict of tests/wavelet_sb_cases.problem (tests/test_gpu_wavelet_sb.py's helpers take it) plus psf_size, phi."""
    import sbtv_oracle as o
    kind, size, phi, starts, (M, N), c_p, _ = WAV_CASES[name]
    d = o.DEMO[kind]
    ys, st0 = [], None
    for b in range(len(starts)):
        x = synth_image(M, N, 4 + 5 * b)
        st = setup(kind, x, np.random.default_rng(3 + 3 * b).standard_normal(x.shape), size, phi, evMax=1.0)
        ys.append(st["y"])
        st0 = st if st0 is None else st0                     # one sigma2 per call: that of image 0
    s_lo, s_hi = sorted((st0["sigma_min"], st0["sigma_max"]))
    base = wsc.options(st0["sigma"], WAV_SAMPLES, 0)
    base["sigma2"] = (s_lo + s_hi) / 2
    del base["sigma"]
    base.update(burnIn=WAV_BURNIN, p_true=tuple(d["true"]), p_min=tuple(d["pmin"]), p_max=tuple(d["pmax"]),
                fix_p=(False,) * len(d["true"]), c_p=tuple(c_p), fix_sigma=False, sigma2_min=s_lo,
                sigma2_max=s_hi, c_sigma=WAV_C_SIGMA, psf_size=size, phi=phi)
    ops = [dict(base, p_init=tuple(p0)) for p0 in starts]
    return dict(y=np.stack(ys), model=st0["model"], kind=kind, h=wc.daub(2), levels=WAV_LEVELS, ops=ops, batch=len(starts),
                sigma_true2=st0["sigma"] ** 2, psf_size=size, phi=phi)


def wav_noise(name):
    _, _, _, starts, (M, N), _, seed = WAV_CASES[name]
    return np.random.default_rng(seed).standard_normal((WAV_SAMPLES - 1, len(starts), M, wsc.bands(WAV_LEVELS) * N))


def wav_run(p, nz, perturb=False):
    """[(eb, results)] per chain of the literal restatement."""
    return [wsb.literal(_perturbed(p["y"][b]) if perturb else p["y"][b], p["model"], p["h"], p["levels"], p["ops"][b], nz[:, b])
            for b in range(p["batch"])]


@functools.lru_cache(maxsize=None)
def wav_reference(name, perturb=False):
    return wav_run(wav_problem(name), wav_noise(name), perturb)


# ---- the taps of given parameters with the error bars of section (b) of tests/test_gpu_psf_sizes.py -------------------
def taps_and_bars(kind, t, p, phi=0.0, eps=1e-13):
    """(taps, [derivative taps], tap bar, [derivative-tap bars]) of sbtv_oracle.PSF_TAPS at parameters p.  The taps f / a to
    rtol eps: exp / pow within a few ulp, the sum a of at most 225 positive terms another 225 * 1.1e-16.  A derivative tap
    (e a - f a') / a^2 is a difference of like terms: the same relative error eps on e, f, a, a' carried through the quotient
    gives eps (|e| a + f |a'|) / a^2 per tap.  f, e, a, a' are the oracle's un-normalised values and sums (`_unnormalised`)."""
    import sbtv_oracle as o
    pp = tuple(p) + ((phi,) if kind == "gaussian" else ())
    taps = o.PSF_TAPS[kind][0](t, pp)
    dtaps = [fn(t, pp) for fn in o.PSF_TAPS[kind][1]]
    f, es = _unnormalised(kind, t, pp)
    a = float(np.sum(f))
    bars = [eps * (np.abs(e) * a + f * abs(float(np.sum(e)))) / a ** 2 for e in es]
    return taps, dtaps, eps * np.abs(taps), bars


def _unnormalised(kind, t, p):
    """f and [e_q] before normalisation, the expressions of sbtv_oracle (Sum_gauss_psf, sum_mof_psf, sum_lap_psf) as arrays."""
    import sbtv_oracle as o
    if kind == "gaussian":
        w1, w2, phi = p
        U, V = o._grid(t, phi)
        ex = np.exp(-(w1 ** 2 * U ** 2 + w2 ** 2 * V ** 2) / 2)
        return (w1 * w2 / (2 * math.pi)) * ex, [(w2 / (2 * math.pi)) * (1 - w1 ** 2 * U ** 2) * ex,
                                                (w1 / (2 * math.pi)) * (1 - w2 ** 2 * V ** 2) * ex]
    X = np.arange(-t + (t + 1) / 2, t - (t + 1) / 2 + 1)
    if kind == "moffat":
        a, b = p
        xy = X[:, None] ** 2 + X[None, :] ** 2
        pw = (xy * a ** 2 / b + 1) ** (-(b + 2) / 2)
        f = a ** 2 * pw / (2 * math.pi)
        dal = (2 - ((b + 2) * xy * a ** 2) / (2 * (b + xy * a ** 2))) * pw * (a / (2 * math.pi))
        dbe = (-np.log(xy * a ** 2 / b + 1) + ((b + 2) * xy * a ** 2) / (b * (b + xy * a ** 2))) * pw * (a ** 2 / (4 * math.pi))
        return f, [dal, dbe]
    b, = p
    s = np.abs(X)[:, None] + np.abs(X)[None, :]
    return (b ** 2 / 4) * np.exp(-b * s), [((2 * b - b ** 2 * s) / 4) * np.exp(-b * s)]
