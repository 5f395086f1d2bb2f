"""The TV + wavelet-l1 CoRAL problems shared by tests/test_coral_wavelet_cpu.py and tests/test_gpu_coral_wavelet.py, built as
tests/analysis_cases.py builds its own: synth_image(M, N, 4), wavelet_cases.setup (sbtv_oracle.demo_setup("gaussian", ...), BSNR
30, 7 x 7 Gaussian taps).  tau1, tau2 are given in units of sigma^2.  Each reference (the literal restatement,
tests/coral_wavelet_restatement.py) is computed once per session and never modified."""
import functools

import numpy as np

from conftest import synth_image

import coral_wavelet_restatement as cr
import wavelet_cases as wc

# name: (M, N), filter length, levels, TViters, stop rule, tolA, start (0, 2 or "random"), MAXITERA, tau1 / sigma^2, tau2 / sigma^2,
# mu1, mu2, and the outer iteration at which the literal restatement stops on the CPU (tests/test_coral_wavelet_cpu.py asserts it,
# and that the criterion at that iteration and at the one before are each at least 1 % away from tolA)
CASES = {
    "1": ((64, 64), 2, 4, 5, 1, 1e-4, 2, 60, 0.5, 0.5, 0.05, 0.05, 27),        # rule 1 inside (2, 60): the lagged stop
    "2": ((16, 18), 2, 3, 5, 1, 1e-3, 2, 40, 0.5, 0.5, 0.05, 0.05, 10),        # partly filled last workgroup
    "3": ((48, 40), 4, 3, 3, 1, 1e-3, 0, 40, 0.5, 0.5, 0.05, 0.1, 6),          # D4, rectangular, zero start, mu1 != mu2
    "4": ((100, 90), 2, 3, 5, 1, 0.0, 2, 10, 0.5, 0.5, 0.05, 0.05, 10),        # chirp-z FFT path, runs to MAXITERA
    "5": ((15, 16), 2, 3, 5, 1, 1e-3, 2, 40, 0.5, 0.5, 0.05, 0.05, 11),        # odd M: TV(u) by the stand-alone reduction
    # D4, rule 2 on the image, zero start, ten Chambolle iterations: two launches per prox
    "6": ((128, 128), 4, 4, 10, 2, 1.1e-3, 0, 30, 0.3, 0.7, 0.05, 0.02, 10),
    # 262 144 pixels, 2 621 440 coefficients: the grid-stride loops of both pixel passes; the Chambolle path for larger images
    "7": ((512, 512), 2, 4, 5, 1, 0.0, 2, 4, 0.5, 0.5, 0.05, 0.05, 4),
    # rule 3 from a random start image: objective(2) is below tolA, but the rule is not evaluated before outer = 2, where the
    # objective is above
    "8": ((64, 64), 2, 3, 5, 3, 3.5e5, "random", 30, 0.5, 0.5, 0.05, 0.05, 5),
}
INSIDE = "123568"                                           # the cases whose rule fires inside the loop


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(x, y, H, h, levels, tau1, tau2, mu1, mu2, TViters, init, stop, tolA, maxiter, stops_at, p_true, sigma) of a case."""
    shape, K, levels, tviters, stop, tolA, init, maxiter, t1, t2, mu1, mu2, stops_at = CASES[name]
    x = synth_image(shape[0], shape[1], 4)
    st = wc.setup(x)
    if init == "random":
        init = np.random.default_rng(21).uniform(0, 255, size=shape)
    s2 = st["sigma"] ** 2
    return dict(x=x, y=st["y"], H=st["model"].H_FFT(*st["p_true"]), h=wc.daub(K), levels=levels, tau1=t1 * s2, tau2=t2 * s2,
                mu1=mu1, mu2=mu2, TViters=tviters, init=init, stop=stop, tolA=tolA, maxiter=maxiter, stops_at=stops_at,
                p_true=st["p_true"], sigma=st["sigma"])


def run(fn, p, **kw):
    args = dict(TViters=p["TViters"], true_x=p["x"], stopcriterion=p["stop"], tolA=p["tolA"], maxiter=p["maxiter"],
                initialization=p["init"])
    args.update(kw)
    return fn(p["y"], p["H"], p["h"], p["levels"], p["tau1"], p["tau2"], p["mu1"], p["mu2"], **args)


@functools.lru_cache(maxsize=None)
def reference(name):
    """CoRAL_v2.m line for line on the case (read-only for its users)."""
    return run(cr.coral_wavelet, problem(name))


@functools.lru_cache(maxsize=None)
def operator_form(name):
    """The state form of the device on the case (read-only for its users)."""
    return run(cr.coral_wavelet_operator, problem(name))


def calls(p, n_outer):
    """What the call counter advances by: AT(y), the invLS probe, AT(y) again, AT(zeros) for the zero start, the initial A, then
    invLS and A per outer iteration (P2 and P2' are not counted by the reference)."""
    zero_start = not isinstance(p["init"], np.ndarray) and p["init"] == 0
    return 3 + (1 if zero_start else 0) + 1 + 2 * n_outer


FLAT_GAIN = 0.9


@functools.lru_cache(maxsize=None)
def flat_problem():
    """A constant observation, 32 x 32, start 2, six iterations, Haar, levels 3: every image of the iteration is constant up to
    rounding, so every prox input has a gradient of rounding size and every Chambolle call stops at k = 1 (err far below the
    inner tolerance).  Optimistic launches (all TViters steps) must be caught by the host's check and the solve repeated with
    exact launches.  The taps are those of the other cases times FLAT_GAIN: with a PSF of unit sum the iteration would sit at its
    fixed point x = y from the start, and objective(2), the residual and x - u would be rounding noise that no relative bar can
    compare; with |H(0)| = 0.9 every trace entry is of ordinary size."""
    x = np.full((32, 32), 100.0)
    st = wc.setup(synth_image(32, 32, 4))                    # for the PSF and a noise level
    s2 = st["sigma"] ** 2
    return dict(x=x, y=x.copy(), H=FLAT_GAIN * st["model"].H_FFT(*st["p_true"]), h=wc.daub(2), levels=3, tau1=0.5 * s2,
                tau2=0.5 * s2, mu1=0.05, mu2=0.05, TViters=5, init=2, stop=1, tolA=0.0, maxiter=6, stops_at=6,
                p_true=st["p_true"], sigma=st["sigma"], gain=FLAT_GAIN)


@functools.lru_cache(maxsize=None)
def flat_reference():
    return run(cr.coral_wavelet, flat_problem())


def huge_tau2(p, n):
    """A tau2 whose threshold tau2 / mu2 is above every soft argument of a run of n outer iterations from the zero start, so
    that v stays exactly zero: analysis_cases.huge_tau scaled to this iteration, where the TV split feeds the x-step too.
    While v is zero, bv_k = -W'S_k with S_k = x_1 + ... + x_k, and the soft argument of iteration k + 1 is W'x_k - bv_k =
    W'(x_k + S_k); max|W'a| <= ||a||_2 for the Parseval frame, so it is at most t_k = a_k + s_k, a_k = ||x_k||_2, s_k = ||S_k||_2.
    The TV prox returns u_k = g - lambda div p with g = x_{k-1} - bu_{k-1}, lambda = tau1 / mu1 and Chambolle's duals, which stay
    in |p| <= 1 pixel by pixel (the update (p + t grad) / (1 + t |grad|) keeps them there); ||div||^2 <= 8, so
    ||u_k + bu_{k-1}||_2 = ||x_{k-1} - lambda div p||_2 <= a_{k-1} + lambda sqrt(8 M N).  The x-step, with v_k = 0 and
    W bv_{k-1} = -W W'S_{k-1} = -S_{k-1}, is x_k = invLS(B'y + mu1 (u_k + bu_{k-1}) - mu2 S_{k-1}) with ||invLS|| <= 1 / mu,
    mu = mu1 + mu2:
        a_k <= ||B'y|| / mu + a_{k-1} + c + s_{k-1},    c = tau1 sqrt(8 M N) / mu        (mu1 / mu <= 1, mu2 / mu <= 1)
    and s_k <= s_{k-1} + a_k.  With A = ||B'y|| / mu + c and t_0 = 0: t_k <= 2 a_k + s_{k-1} <= 2 A + 3 t_{k-1}, hence
    t_k <= (3^k - 1) A.  The arguments of iterations 1 .. n are t_0 .. t_{n-1} < 3^(n-1) A; the threshold is 3^n A, three
    times that."""
    ATy = np.real(np.fft.ifft2(np.conj(p["H"]) * np.fft.fft2(p["y"])))
    mu = p["mu1"] + p["mu2"]
    M, N = p["y"].shape
    A = float(np.linalg.norm(ATy)) / mu + p["tau1"] * np.sqrt(8.0 * M * N) / mu
    return p["mu2"] * 3.0 ** n * A
