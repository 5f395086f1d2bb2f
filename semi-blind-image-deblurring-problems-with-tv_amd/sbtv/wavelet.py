"""Host mirror of the wavelet-l1 path (SALSA/run_deblur_synthesis_L1.m): the redundant, translation-invariant wavelet frame
`mrdwt_TI2D` / `mirdwt_TI2D` (SALSA/mrdwt_TI2D.m, mirdwt_TI2D.m; the Rice Wavelet Toolbox MEX behind them is not shipped
with the reference, the transform is defined in include/sbtv.h), `soft` (SALSA/soft.m), `daubcqf` and the solver
`SALSA_wavelet` (SALSA_v2 with 'Psi' = soft and the 'LS' of the demo), `SALSA_analysis` (its analysis-prior form, 'P' = W and
'PT' = W', on the image), `SALSA_masked_analysis` (the same prior on the masked-observation likelihood of SALSA_masked),
`csalsa_wavelet` (the constrained form of that, csalsa with the same 'P' / 'PT', for a known noise
level), and `SAPG_wavelet`, the empirical-Bayes estimate of the regularisation parameter that the script runs
first (the theta part of SALSA/SAPG_algorithm_1.m), and `myula_wavelet`, the MYULA chain at a fixed theta with the posterior
mean / variance of its samples.  Coefficients are (M, (3J+1) N) arrays, J = levels - 1:
[a_J | LH1 HL1 HH1 | LH2 ...], or (B, M, (3J+1) N) for a batch; host and device arrays as everywhere in this package."""
from __future__ import annotations

import copy
import ctypes as C
import math

import numpy as np

from . import _lib as L
from .admm import _common
from .operators import _InvLS
from .sapg import _moment_buffers, _moments_opts
from .tv import _parse_varargin

_WAVELET_OPTIONS = {"MU", "WAVELET", "LEVELS", "AT", "STOPCRITERION", "TOLERANCEA", "MAXITERA", "TRUE_X", "INITIALIZATION",
                    "VERBOSE", "SPECULATE"}

_vp = L.vptr


def daubcqf(N):
    """Daubechies scaling filter of even length N = 2, 4, 6, 8, minimum phase, sum(h) = sqrt(2) (SALSA/daubcqf.m with 'min').
    Spectral factorisation: with y = (2 - z - 1/z) / 4 the polynomial P(y) = sum_k C(N/2-1+k, k) y^k has N/2 - 1 roots, each
    gives a pair (z, 1/z); the minimum-phase filter takes the one inside the unit circle next to the N/2 zeros at z = -1."""
    N = int(N)
    if N not in (2, 4, 6, 8):
        raise ValueError("daubcqf: N must be 2, 4, 6 or 8")
    p = N // 2
    h = np.array([1.0])
    for _ in range(p):
        h = np.convolve(h, [1.0, 1.0])
    if p > 1:
        coef = [math.comb(p - 1 + k, k) for k in range(p)]              # ascending powers of y
        for yr in np.roots(coef[::-1]):
            b = 2.0 - 4.0 * yr                                           # z^2 - b z + 1 = 0
            d = np.sqrt(b * b - 4.0 + 0j)
            z = (b + d) / 2.0
            if abs(z) > 1.0:
                z = (b - d) / 2.0
            h = np.convolve(h, [1.0, -z])
        h = np.real(h)
    return h * (math.sqrt(2.0) / h.sum())


def _filter(h):
    a = np.ascontiguousarray(np.asarray(h, dtype=np.float64).ravel())
    return a, _vp(a), int(a.size)


def _resized(ref: L.Images, N):
    """An output buffer like `ref` with N columns per image."""
    r = copy.copy(ref)
    r.N = int(N)
    return L.empty_like_images(r)


def _bands(levels):
    return 3 * (int(levels) - 1) + 1


def mrdwt_TI2D(x, h, levels, ctx=None):
    """z = mrdwt_TI2D(x, h, levels): analysis W' of the redundant wavelet frame, (M, N) -> (M, (3 (levels-1) + 1) N)."""
    ctx = ctx or L.default_context()
    xi = L.Images(x)
    ha, hp, K = _filter(h)
    zo = _resized(xi, xi.N * max(_bands(levels), 1))
    ctx.check(ctx.lib.sbtv_mrdwt_TI2D(ctx.h, xi.ptr, xi.M, xi.N, xi.B, hp, K, int(levels), zo.ptr, xi.flags), xi.flags)
    return L.images_result(zo, (x.dim() == 2) if xi.torch else xi.squeeze)


def mirdwt_TI2D(z, h, levels, ctx=None):
    """x = mirdwt_TI2D(z, h, levels): synthesis W, the exact adjoint of mrdwt_TI2D; W W' = I for an orthonormal h."""
    ctx = ctx or L.default_context()
    zi = L.Images(z)
    ha, hp, K = _filter(h)
    nb = max(_bands(levels), 1)
    if zi.N % nb:
        raise ValueError("z must have (3 (levels-1) + 1) N columns")
    xo = _resized(zi, zi.N // nb)
    ctx.check(ctx.lib.sbtv_mirdwt_TI2D(ctx.h, zi.ptr, zi.M, zi.N // nb, zi.B, hp, K, int(levels), xo.ptr, zi.flags), zi.flags)
    return L.images_result(xo, (z.dim() == 2) if zi.torch else zi.squeeze)


def soft(x, T, ctx=None):
    """y = soft(x, T) = sign(x) .* max(abs(x) - T, 0) (SALSA/soft.m); T a scalar or one value per array of a batch."""
    ctx = ctx or L.default_context()
    xi = L.Images(x)
    Ta, Tp = L.dvec(T, xi.B)
    yo = L.empty_like_images(xi)
    ctx.check(ctx.lib.sbtv_soft(ctx.h, xi.ptr, xi.M, xi.N, xi.B, Tp, yo.ptr, xi.flags), xi.flags)
    return L.images_result(yo, (x.dim() == 2) if xi.torch else xi.squeeze)


def _solver_options(name, varargin, kw, ctx):
    """(options, context) of SALSA_wavelet / SALSA_analysis: the name / value pairs, keywords over them; no group."""
    opts = _parse_varargin(varargin, _WAVELET_OPTIONS)
    for k, v in kw.items():
        opts[k.upper()] = v
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError(f"{name} has no sharded variant")
    return opts, ctx


def _check_coefficients(yi, nb, *arrays):
    """The coefficient arguments (None: not given) of a solve on the images yi: nb bands each, in the memory space of yi."""
    for other in arrays:
        if other is not None:
            if (other.B, other.M, other.N) != (yi.B, yi.M, nb * yi.N):
                raise ValueError("coefficient arrays must be (M, (3 (levels-1) + 1) N) per image")
            if other.flags != yi.flags:
                raise ValueError("all image arguments must live in the same memory space")


def _traces(B, *lengths):
    """One zeroed (B, n) trace per length n."""
    return [np.zeros((B, n)) for n in lengths]


def _counters(B, count):
    return [(C.c_int * B)() for _ in range(count)]


def _trimmed(n, single, *traces):
    """Each (trace, extra) cut to the n[b] + extra entries that image b wrote: one array for a single image, else a list
    with one per image; a trace of None (not asked for) comes back empty."""
    out = []
    for t, extra in traces:
        if t is None:
            out.append(np.array([]) if single else [])
        elif single:
            out.append(t[0, :int(n[0]) + extra].copy())
        else:
            out.append([t[b, :n[b] + extra].copy() for b in range(len(n))])
    return tuple(out)


def _salsa_result(images, single, numA, numAt, nout, objective, distance, times, mses):
    """The return tuple of SALSA_wavelet / SALSA_analysis after `images`: the counters and the traces of the iterations run."""
    counts = (int(numA[0]), int(numAt[0])) if single else (np.array(numA[:]), np.array(numAt[:]))
    return images + counts + _trimmed(np.array(nout[:]), single, (objective, 1), (distance, 0), (times, 1), (mses, 1))


def SALSA_wavelet(y, A, tau, *varargin, ctx=None, **kw):
    """[xw, x, numA, numAt, objective, distance, times, mses] = SALSA_wavelet(y, A, tau, 'MU', mu, 'WAVELET', h, 'LEVELS', L,
    'AT', A.T, ...)

    minimise 0.5 ||y - A W xw||^2 + tau ||xw||_1 over the coefficients xw of the redundant wavelet frame W (`mirdwt_TI2D`), as
    SALSA_v2 does in SALSA/run_deblur_synthesis_L1.m:160-180; the iteration is stated in include/sbtv.h (sbtv_SALSA_wavelet).
    x = W xw is the image estimate.  Options: 'MU' (required), 'WAVELET' (an orthonormal scaling filter, default daubcqf(2)),
    'LEVELS' (4), 'AT', 'STOPCRITERION', 'TOLERANCEA', 'MAXITERA', 'TRUE_X' (the true COEFFICIENTS, e.g. mrdwt_TI2D(x_true)),
    'INITIALIZATION' (0, 2 = W' A' y, or a coefficient array), 'VERBOSE', and 'SPECULATE' (sbtv_salsa_opts.speculate: 0 makes the
    host evaluate the stop rule without the one-iteration lag; the result is the same)."""
    opts, ctx = _solver_options("SALSA_wavelet", varargin, kw, ctx)
    levels = int(opts.get("LEVELS", 4))
    nb = max(_bands(levels), 1)
    # the coefficient arguments have (3J+1) N columns: _common compares TRUE_X with y, so they are handled here
    copts = {k: v for k, v in opts.items() if k not in ("TRUE_X", "INITIALIZATION")}
    so, yi, _, _ = _common(y, A, copts, ctx, 1)
    if "MU" not in opts:
        raise L.SbtvError(-1, "SALSA_wavelet: 'MU' is required")
    ha, hp, K = _filter(opts.get("WAVELET", daubcqf(2)))
    B, M, N = yi.B, yi.M, yi.N
    init = opts.get("INITIALIZATION", 0)
    xinit = None
    if np.ndim(init) > 0 or L._is_torch(init):
        xinit = L.Images(init)
        so.initialization = 33333
    else:
        so.initialization = int(init)
        if so.initialization not in (0, 2):
            raise L.SbtvError(-7, "Unknown 'Initialization' option")
    true = opts.get("TRUE_X", None)
    ti = L.Images(true) if true is not None else None
    so.compute_mse = 1 if ti is not None else 0
    _check_coefficients(yi, nb, xinit, ti)
    Kmax = so.maxiter
    xwo = _resized(yi, nb * N)
    xo = L.empty_like_images(yi)
    objective, distance, times, mses = _traces(B, Kmax + 1, Kmax, Kmax + 1, Kmax + 1)
    numA, numAt, nout = _counters(B, 3)
    taps = A._cm(B)
    keep = [L.dvec(v, B) for v in (tau, opts["MU"])]
    tv, mu = (k[1] for k in keep)
    ctx.check(ctx.lib.sbtv_SALSA_wavelet(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, levels, tv, mu, C.byref(so),
                                         ti.ptr if ti else None, xinit.ptr if xinit else None, xwo.ptr, xo.ptr,
                                         _vp(objective), _vp(distance), _vp(times), _vp(mses) if ti else None, numA, numAt,
                                         nout, yi.flags), yi.flags)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    return _salsa_result((L.images_result(xwo, sq), L.images_result(xo, sq)), sq or B == 1, numA, numAt, nout, objective,
                         distance, times, mses if ti else None)


def SALSA_analysis(y, A, tau, *varargin, ctx=None, **kw):
    """[x, numA, numAt, objective, distance, times, mses] = SALSA_analysis(y, A, tau, 'MU', mu, 'WAVELET', h, 'LEVELS', L,
    'AT', A.T, ...)

    minimise 0.5 ||y - A x||^2 + tau ||W' x||_1 over the IMAGE x, W' the analysis operator of the redundant wavelet frame
    (`mrdwt_TI2D`): the analysis-prior form, which SALSA_v2 solves when it is given 'P' = W and 'PT' = W' (SALSA/SALSA_v2.m:98-101,
    389-440) with 'Psi' = soft and 'LS' = real(ifft2(fft2(r) ./ (|H|^2 + mu))); the iteration is stated in include/sbtv.h
    (sbtv_SALSA_analysis).  The options of SALSA_wavelet; 'TRUE_X' is the true IMAGE and an array 'INITIALIZATION' a start image
    (0: zeros, 2: A' y).  distance is ||W'x - u|| / sqrt(||W'x||^2 + ||u||^2), mses ||x - true||^2 / numel(x)."""
    opts, ctx = _solver_options("SALSA_analysis", varargin, kw, ctx)
    levels = int(opts.get("LEVELS", 4))
    init = opts.get("INITIALIZATION", 0)
    if not (np.ndim(init) > 0 or L._is_torch(init)) and int(init) not in (0, 2):
        raise L.SbtvError(-7, "Unknown 'Initialization' option")          # the random start of SALSA_v2 is not offered
    so, yi, xinit, ti = _common(y, A, opts, ctx, 1)
    if "MU" not in opts:
        raise L.SbtvError(-1, "SALSA_analysis: 'MU' is required")
    ha, hp, K = _filter(opts.get("WAVELET", daubcqf(2)))
    B, M, N = yi.B, yi.M, yi.N
    for other in (xinit, ti):
        if other is not None and (other.B, other.M, other.N) != (B, M, N):
            raise ValueError("'TRUE_X' and an array 'INITIALIZATION' must be images of the size of y")
    Kmax = so.maxiter
    xo = L.empty_like_images(yi)
    objective, distance, times, mses = _traces(B, Kmax + 1, Kmax, Kmax + 1, Kmax + 1)
    numA, numAt, nout = _counters(B, 3)
    taps = A._cm(B)
    keep = [L.dvec(v, B) for v in (tau, opts["MU"])]
    tv, mu = (k[1] for k in keep)
    ctx.check(ctx.lib.sbtv_SALSA_analysis(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, levels, tv, mu, C.byref(so),
                                          ti.ptr if ti else None, xinit.ptr if xinit else None, xo.ptr, _vp(objective),
                                          _vp(distance), _vp(times), _vp(mses) if ti else None, numA, numAt, nout, yi.flags),
              yi.flags)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    return _salsa_result((L.images_result(xo, sq),), sq or B == 1, numA, numAt, nout, objective, distance, times,
                         mses if ti else None)


_MASKED_ANALYSIS_OPTIONS = {"MU1", "MU2", "WAVELET", "LEVELS", "AT", "STOPCRITERION", "TOLERANCEA", "MAXITERA", "TRUE_X",
                            "INITIALIZATION", "VERBOSE", "SPECULATE"}


def SALSA_masked_analysis(y, A, mask, tau, *varargin, ctx=None, **kw):
    """[x, numA, numAt, objective, distance, times, mses] = SALSA_masked_analysis(y, A, mask, tau, 'MU1', mu1, 'MU2', mu2,
    'WAVELET', h, 'LEVELS', L, 'AT', A.T, ...)

    minimise 0.5 * sum(mask .* (A x - y).^2) + tau ||W' x||_1 over the IMAGE x: the likelihood of `SALSA_masked` (`mask` holds
    non-negative weights of the shape of y, 0 = pixel not observed: unknown boundaries, missing or weighted pixels) with the
    analysis prior of `SALSA_analysis` (W' = `mrdwt_TI2D`); the iteration is stated in include/sbtv.h
    (sbtv_SALSA_masked_analysis).  Options: 'MU1' (required, the weight of the coefficient split, SALSA_analysis's 'MU'), 'MU2'
    (the weight of the data split, default 0.1, the value of SALSA_masked: it decides the speed, not the answer; the default
    rests on NumPy prototype runs of this iteration at 64 x 64 and 128 x 128 with mu2 = 1 and 0.1 and on the one problem
    SALSA_masked's default was measured on, all with pixel values in 0..255), 'WAVELET' (an orthonormal scaling filter, default
    daubcqf(2)), 'LEVELS' (4), 'AT', 'STOPCRITERION', 'TOLERANCEA', 'MAXITERA', 'TRUE_X' (the true image), 'INITIALIZATION'
    (0 zeros, 2 = AT(mask .* y), or a start image), 'VERBOSE', 'SPECULATE' (sbtv_salsa_opts.speculate bit 0; the result is the
    same).  The return values are shaped as `SALSA_masked` returns them: distance is (outer, 2), column 0 the coefficient split
    ||W'x - u||, column 1 the data split ||Ax - v||, both relative.  For an observation without wrapped pixels see
    `embed_observation`."""
    opts = _parse_varargin(varargin, _MASKED_ANALYSIS_OPTIONS)
    for k, v in kw.items():
        opts[k.upper()] = v
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError("SALSA_masked_analysis has no sharded variant")
    init = opts.get("INITIALIZATION", 0)
    if not (np.ndim(init) > 0 or L._is_torch(init)) and int(init) not in (0, 2):
        raise L.SbtvError(-7, "Unknown 'Initialization' option")          # no random start
    so, yi, xinit, ti = _common(y, A, opts, ctx, 1)
    if mask is None:
        raise L.SbtvError(-1, "SALSA_masked_analysis: the mask is missing")
    mi = L.Images(mask)
    B, M, N = yi.B, yi.M, yi.N
    if (mi.B, mi.M, mi.N) != (B, M, N):
        raise ValueError("the mask must have the shape of y")
    if mi.flags != yi.flags:
        raise ValueError("all image arguments must live in the same memory space")
    if "MU1" not in opts:
        raise L.SbtvError(-1, "SALSA_masked_analysis: 'MU1' is required")
    ha, hp, K = _filter(opts.get("WAVELET", daubcqf(2)))
    levels = int(opts.get("LEVELS", 4))
    for other in (xinit, ti):
        if other is not None and (other.B, other.M, other.N) != (B, M, N):
            raise ValueError("'TRUE_X' and an array 'INITIALIZATION' must be images of the size of y")
    Kmax = so.maxiter
    xo = L.empty_like_images(yi)
    objective, times, mses = _traces(B, Kmax + 1, Kmax + 1, Kmax + 1)
    distance = np.zeros((B, Kmax, 2))
    numA, numAt, nout = _counters(B, 3)
    taps = A._cm(B)
    keep = [L.dvec(v, B) for v in (tau, opts["MU1"], opts.get("MU2", 0.1))]
    tv, m1, m2 = (k[1] for k in keep)
    ctx.check(ctx.lib.sbtv_SALSA_masked_analysis(ctx.h, yi.ptr, mi.ptr, M, N, B, _vp(taps), A.taille, hp, K, levels, tv, m1, m2,
                                                 C.byref(so), ti.ptr if ti else None, xinit.ptr if xinit else None, xo.ptr,
                                                 _vp(objective), _vp(distance), _vp(times), _vp(mses) if ti else None, numA,
                                                 numAt, nout, yi.flags), yi.flags)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    return _salsa_result((L.images_result(xo, sq),), sq or B == 1, numA, numAt, nout, objective, distance, times,
                         mses if ti else None)


_CORAL_WAVELET_OPTIONS = {"MU1", "MU2", "WAVELET", "LEVELS", "TVITERS", "AT", "LS", "STOPCRITERION", "TOLERANCEA", "MAXITERA",
                          "INITIALIZATION", "TRUE_X", "VERBOSE", "SPECULATE"}


def CoRAL_wavelet(y, A, tau1, tau2, *varargin, ctx=None, **kw):
    """[x, numA, numAt, objective, distance, times, mses] = CoRAL_wavelet(y, A, tau1, tau2, 'MU1', mu1, 'MU2', mu2, 'WAVELET', h,
    'LEVELS', L, 'TVITERS', K, 'AT', A.T, 'LS', A.LS(mu1 + mu2), ...)

    minimise 0.5 ||y - A x||^2 + tau1 TV(x) + tau2 ||W' x||_1 over the IMAGE x: CoRAL (SALSA/CoRAL_v2.m:2-476) with the compound
    regulariser TV + wavelet-l1, i.e. 'P1' = identity with 'TVINITIALIZATION1' = 1, 'P2' = W = `mirdwt_TI2D`, 'P2T' = W' =
    `mrdwt_TI2D`, 'PSI2' = soft; the iteration is stated in include/sbtv.h (sbtv_CoRAL_wavelet).  'MU1' and 'MU2' are required,
    'LS' is `A.LS(mu1 + mu2)` (the reference's convention, :137; another mu is refused).  Other options: 'WAVELET' (an
    orthonormal scaling filter, default daubcqf(2)), 'LEVELS' (4), 'TVITERS' (5), 'STOPCRITERION', 'TOLERANCEA', 'MAXITERA',
    'INITIALIZATION' (0 zeros, 2 = A' y, or a start image), 'TRUE_X' (the true image), 'VERBOSE', 'SPECULATE'
    (sbtv_salsa_opts.speculate; the result is the same).  The return values are shaped as `CoRAL` returns them: distance is
    (outer, 2), column 0 the TV split ||x - u||, column 1 the wavelet split ||W'x - v||, both relative."""
    opts = _parse_varargin(varargin, _CORAL_WAVELET_OPTIONS)
    for k, v in kw.items():
        opts[k.upper()] = v
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError("CoRAL_wavelet has no sharded variant")
    init = opts.get("INITIALIZATION", 0)
    if not (np.ndim(init) > 0 or L._is_torch(init)) and int(init) not in (0, 2):
        raise L.SbtvError(-7, "Unknown 'Initialization' option")          # the random start of CoRAL_v2 is not offered
    so, yi, xinit, ti = _common(y, A, opts, ctx, 1)
    if "MU1" not in opts or "MU2" not in opts:
        raise L.SbtvError(-1, "CoRAL_wavelet: 'MU1' and 'MU2' are required")
    B, M, N = yi.B, yi.M, yi.N
    LS = opts.get("LS", None)
    if not isinstance(LS, _InvLS) or LS.op is not A:
        raise L.SbtvError(-9, "(A^T A + \\mu I)^(-1) must be specified as a function handle.")   # :197
    keep = [L.dvec(v, B) for v in (tau1, tau2, opts["MU1"], opts["MU2"])]
    t1, t2, m1, m2 = (k[1] for k in keep)
    if not np.array_equal(np.broadcast_to(np.asarray(LS.mu, dtype=np.float64), (B,)), keep[2][0] + keep[3][0]):
        raise L.SbtvError(-9, "CoRAL_wavelet: 'LS' must be A.LS(mu1 + mu2)")                  # :137
    so.TViters = int(opts.get("TVITERS", 5))
    ha, hp, K = _filter(opts.get("WAVELET", daubcqf(2)))
    levels = int(opts.get("LEVELS", 4))
    for other in (xinit, ti):
        if other is not None and (other.B, other.M, other.N) != (B, M, N):
            raise ValueError("'TRUE_X' and an array 'INITIALIZATION' must be images of the size of y")
    Kmax = so.maxiter
    xo = L.empty_like_images(yi)
    objective, times, mses = _traces(B, Kmax + 1, Kmax + 1, Kmax + 1)
    distance = np.zeros((B, Kmax, 2))
    numA, numAt, nout = _counters(B, 3)
    taps = A._cm(B)
    ctx.check(ctx.lib.sbtv_CoRAL_wavelet(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, levels, t1, t2, m1, m2, C.byref(so),
                                         ti.ptr if ti else None, xinit.ptr if xinit else None, xo.ptr, _vp(objective),
                                         _vp(distance), _vp(times), _vp(mses) if ti else None, numA, numAt, nout, yi.flags),
              yi.flags)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    return _salsa_result((L.images_result(xo, sq),), sq or B == 1, numA, numAt, nout, objective, distance, times,
                         mses if ti else None)


_CSALSA_WAVELET_OPTIONS = {"WAVELET", "LEVELS", "AT", "STOPCRITERION", "TOLERANCEA", "MAXITERA", "INITIALIZATION", "TRUE_X",
                           "CONTINUATIONFACTOR", "EPSILON", "SPECULATE", "VERBOSE"}


def csalsa_wavelet(y, A, mu1, mu2, sigma, *varargin, ctx=None, **kw):
    """[x, numA, numAt, objective, distance1, distance2, criterion, times, mses] = csalsa_wavelet(y, A, mu1, mu2, sigma,
    'WAVELET', h, 'LEVELS', L, 'AT', A.T, ...)

    minimise ||W' x||_1 subject to ||A x - y||_2 <= epsilon over the IMAGE x: C-SALSA (SALSA/CSALSA_v2.m:160-561) with the wavelet
    analysis prior, i.e. `csalsa` with 'P' = W = `mirdwt_TI2D`, 'PT' = W' = `mrdwt_TI2D`, 'PSI' = soft and 'LS' = A.invLS; the
    iteration is stated in include/sbtv.h (sbtv_CSALSA_wavelet).  For the user who knows the noise level sigma (from the sensor, or
    the sigma2 of SAPG_wavelet_semiblind) and not a regularisation parameter: 'EPSILON' defaults to sqrt(n + 8 sqrt n) sigma.
    A.invLS(r, mu1) is the exact x-minimiser only for mu2 = 1; other mu2 run as the reference would run them.
    Options: 'WAVELET' (an orthonormal scaling filter, default daubcqf(2)), 'LEVELS' (4), 'AT', 'STOPCRITERION' (3), 'TOLERANCEA',
    'MAXITERA', 'INITIALIZATION' (0 zeros, 2 = A' y, or a start image), 'TRUE_X' (the true image), 'CONTINUATIONFACTOR' (1),
    'EPSILON' (0: the default), 'SPECULATE' (sbtv_salsa_opts.speculate bit 0; the result is the same), 'VERBOSE'.
    objective is ||W' x||_1, the objective of the problem (the reference records phi of the image).  Traces are 1-based in the
    reference; the returned arrays hold entries 1..outer in positions 0..outer-1, as `csalsa` returns them."""
    opts = _parse_varargin(varargin, _CSALSA_WAVELET_OPTIONS)
    for k, v in kw.items():
        opts[k.upper()] = v
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError("csalsa_wavelet has no sharded variant")
    init = opts.get("INITIALIZATION", 0)
    if not (np.ndim(init) > 0 or L._is_torch(init)) and int(init) not in (0, 2):
        raise L.SbtvError(-7, "Unknown 'Initialization' option")          # the random start of CSALSA_v2 is not offered
    so, yi, xinit, ti = _common(y, A, opts, ctx, 3)                       # default :171
    ha, hp, K = _filter(opts.get("WAVELET", daubcqf(2)))
    levels = int(opts.get("LEVELS", 4))
    B, M, N = yi.B, yi.M, yi.N
    for other in (xinit, ti):
        if other is not None and (other.B, other.M, other.N) != (B, M, N):
            raise ValueError("'TRUE_X' and an array 'INITIALIZATION' must be images of the size of y")
    Kmax = max(so.maxiter, 1)
    xo = L.empty_like_images(yi)
    objective, distance1, distance2, criterion, times, mses = _traces(B, *([Kmax] * 6))
    numA, numAt, nout = _counters(B, 3)
    taps = A._cm(B)
    keep = [L.dvec(v, B) for v in (mu1, mu2, sigma, opts.get("EPSILON", 0.0))]
    m1, m2, sg, ep = (k[1] for k in keep)
    ctx.check(ctx.lib.sbtv_CSALSA_wavelet(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, levels, m1, m2, sg, ep,
                                          float(opts.get("CONTINUATIONFACTOR", 1.0)), C.byref(so), ti.ptr if ti else None,
                                          xinit.ptr if xinit else None, xo.ptr, _vp(objective), _vp(distance1), _vp(distance2),
                                          _vp(criterion), _vp(times), _vp(mses) if ti else None, numA, numAt, nout, yi.flags),
              yi.flags)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    single = sq or B == 1
    counts = (int(numA[0]), int(numAt[0])) if single else (np.array(numA[:]), np.array(numAt[:]))
    return (L.images_result(xo, sq),) + counts + _trimmed(np.array(nout[:]), single, (objective, 0), (distance1, 0),
                                                          (distance2, 0), (criterion, 0), (times, 0), (mses if ti else None, 0))


def _op(op, name, default=None):
    v = op.get(name, default) if isinstance(op, dict) else getattr(op, name, default)
    if v is None:
        raise KeyError(f"op.{name} is required")
    return v


def _chain_noise(noise, yi, steps, nb, steps_text):
    """(array kept alive, pointer) of the injected normals of a chain on the coefficients: `steps` steps of [B][M, nb N]."""
    if noise is None:
        return None, None
    B, M, N = yi.B, yi.M, yi.N
    if L._is_torch(noise):
        if yi.flags != L.SBTV_DEVICE_PTRS:
            raise ValueError("all image arguments must live in the same memory space")
        # the step kernel reads steps * B * dimX doubles from this pointer: anything else is an out-of-bounds read
        want = steps * B * M * nb * N
        # (dense: its elements fill one gap-free span of memory, as a contiguous tensor or a `to_device` view does)
        span = 1 + sum((n - 1) * st for n, st in zip(noise.shape, noise.stride())) if noise.numel() else 0
        if str(noise.dtype) != "torch.float64" or noise.numel() != want or span != want or any(st < 1 for st in noise.stride()):
            raise ValueError(f"a device noise tensor must be dense float64 with ({steps_text}) * B * "
                             f"M * (3 (levels-1) + 1) N = {want} elements, in the library's layout")
        return noise, C.c_void_p(noise.data_ptr())
    if yi.flags != L.SBTV_HOST_PTRS:
        raise ValueError("all image arguments must live in the same memory space")
    a = np.asarray(noise, dtype=np.float64)
    if a.ndim == 3:
        a = a[:, None]
    if a.shape != (steps, B, M, nb * N):
        raise ValueError(f"noise must be ({steps_text}, [B,] M, (3 (levels-1) + 1) N)")
    keep = L.column_major_images(a.reshape((-1,) + a.shape[2:]))
    return keep, _vp(keep)


def SAPG_wavelet(y, A, h, levels, op, noise=None, xw0=None, ctx=None):
    """[theta_EB, results] = SAPG_wavelet(y, A, h, levels, op)

    Empirical-Bayes estimate of theta in p(xw | theta) ~ exp(-theta ||xw||_1) from y = A W xw + noise, as
    SALSA/run_deblur_synthesis_L1.m:125-156 obtains it before the MAP solve (then SALSA_wavelet at tau = theta_EB sigma^2,
    mu = theta_EB): a MYULA chain on the wavelet coefficients and the log-scale update of SALSA/SAPG_algorithm_1.m:165-216, theta
    part only (its `tau` part cannot be called by the script; include/sbtv.h, sbtv_SAPG_wavelet, states the loop).
    A: the blur (sbtv.BlurOperator); h, levels: the frame, as for mrdwt_TI2D.
    op (dict or object): samples, burnIn, th_init, min_th, max_th, d_scale, d_exp, lambda, gamma, sigma (the noise standard
    deviation, op.sigma of the script) or sigma2; optional warmup (0, as the script sets it), X0 (start coefficients, default
    W'y), seed (1), chain_offset (0).
    noise: optional (steps, [B,] M, (3J+1) N) normals instead of the device Philox stream, steps = max(warmup-1, 0) +
    samples-1; host array or a device tensor already in the library's layout (step-major, column-major coefficient arrays).
    xw0 overrides op.X0.  y may be a batch (B, M, N): one chain per image, theta_EB is then an array and results a list.
    results keys (SAPG_algorithm_1.m:219-231): last_samp, logPiTraceX, gXTrace, mean_theta, last_theta, thetas, mean_thetas,
    tol_thetas, options, logPiTrace_WU (when warmup > 0), and Xlast_sample."""
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError("SAPG_wavelet has no sharded variant")
    yi = L.Images(y)
    B, M, N = yi.B, yi.M, yi.N
    nb = max(_bands(levels), 1)
    ha, hp, K = _filter(h)
    o = L.sbtv_sapg_wavelet_opts()
    o.samples = int(_op(op, "samples"))
    o.warmup = int(_op(op, "warmup", 0))
    o.burnIn = int(_op(op, "burnIn"))
    o.lambda_ = float(_op(op, "lambda"))
    o.gamma = float(_op(op, "gamma"))
    s2 = op.get("sigma2") if isinstance(op, dict) else getattr(op, "sigma2", None)
    o.sigma2 = float(s2) if s2 is not None else float(_op(op, "sigma")) ** 2
    o.th_init = float(_op(op, "th_init"))
    o.min_th = float(_op(op, "min_th"))
    o.max_th = float(_op(op, "max_th"))
    o.d_scale = float(_op(op, "d_scale"))
    o.d_exp = float(_op(op, "d_exp"))
    o.seed = int(_op(op, "seed", 1))
    o.chain_offset = int(_op(op, "chain_offset", 0))
    S, Wn = o.samples, max(o.warmup, 0)
    if xw0 is None:
        xw0 = op.get("X0") if isinstance(op, dict) else getattr(op, "X0", None)
    x0i = L.Images(xw0) if xw0 is not None else None
    if x0i is not None:
        if (x0i.B, x0i.M, x0i.N) != (B, M, nb * N):
            raise ValueError("coefficient arrays must be (M, (3 (levels-1) + 1) N) per image")
        if x0i.flags != yi.flags:
            raise ValueError("all image arguments must live in the same memory space")
    nz_keep, nz_ptr = _chain_noise(noise, yi, max(Wn - 1, 0) + S - 1, nb, "max(warmup-1, 0) + samples-1")
    thetas, gx, logpi, tol = (np.zeros((B, max(S, 1))) for _ in range(4))
    logpi_wu = np.zeros((B, max(Wn, 1)))
    means = np.zeros((B, max(S - o.burnIn, 1)))
    eb = np.zeros(B)
    xl = _resized(yi, nb * N)
    taps = A._cm(B)
    ctx.check(ctx.lib.sbtv_SAPG_wavelet(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, int(levels), C.byref(o),
                                        x0i.ptr if x0i else None, nz_ptr, _vp(thetas), _vp(gx), _vp(logpi), _vp(logpi_wu),
                                        _vp(means), _vp(tol), _vp(eb), xl.ptr, yi.flags), yi.flags)
    xs = L.images_result(xl, False)
    results = []
    for b in range(B):
        r = dict(last_samp=S, logPiTraceX=logpi[b], gXTrace=gx[b], mean_theta=float(eb[b]), last_theta=float(thetas[b, -1]),
                 thetas=thetas[b], mean_thetas=means[b, :max(S - o.burnIn, 0)], tol_thetas=tol[b], options=op,
                 Xlast_sample=xs[b])
        if Wn > 0:
            r["logPiTrace_WU"] = logpi_wu[b, :Wn]
        results.append(r)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    if sq:
        return float(eb[0]), results[0]
    return eb, results


def _fixed_theta_chain(entry, make_opts, finish_opts, y, A, h, levels, op, theta, sigma2, noise, xw0, posterior, ctx):
    """What myula_wavelet and skrock_wavelet share: the arguments of sbtv_<entry> but its option struct.  make_opts() returns
    the struct with the sampler's own fields set (samples, lambda, seed and chain_offset are set here); finish_opts(o, sigma2)
    completes it once the per-chain sigma2 array is known."""
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError(f"{entry} has no sharded variant")
    yi = L.Images(y)
    B, M, N = yi.B, yi.M, yi.N
    nb = max(_bands(levels), 1)
    ha, hp, K = _filter(h)
    o = make_opts()
    o.samples = int(_op(op, "samples"))
    o.lambda_ = float(_op(op, "lambda"))
    o.seed = int(_op(op, "seed", 1))
    o.chain_offset = int(_op(op, "chain_offset", 0))
    get = lambda name: op.get(name) if isinstance(op, dict) else getattr(op, name, None)
    if theta is None:
        theta = _op(op, "theta")
    if sigma2 is None:
        sigma2 = get("sigma2")
        if sigma2 is None:
            sigma2 = np.asarray(_op(op, "sigma"), dtype=np.float64) ** 2
    keep = [L.dvec(theta, B), L.dvec(sigma2, B)]
    if finish_opts is not None:
        finish_opts(o, keep[1][0])
    S = o.samples
    if xw0 is None:
        xw0 = get("X0")
    x0i = L.Images(xw0) if xw0 is not None else None
    if x0i is not None:
        if (x0i.B, x0i.M, x0i.N) != (B, M, nb * N):
            raise ValueError("coefficient arrays must be (M, (3 (levels-1) + 1) N) per image")
        if x0i.flags != yi.flags:
            raise ValueError("all image arguments must live in the same memory space")
    nz_keep, nz_ptr = _chain_noise(noise, yi, max(S - 1, 0), nb, "samples-1")
    gx, logpi = np.zeros((B, max(S, 1))), np.zeros((B, max(S, 1)))
    xl = _resized(yi, nb * N)
    taps = A._cm(B)
    mo, pm, pv, pc, cm, cv, pooled = None, None, None, None, None, None, False
    if posterior is not None and posterior is not False:
        p = {} if posterior is True else dict(posterior)
        coefficients = bool(p.pop("coefficients", False))
        mo = _moments_opts(p if p else True)
        pooled = bool(mo.pooled)
        pm, pv, pc = _moment_buffers(yi, 1 if pooled else B)
        if coefficients:
            cm, cv, _ = _moment_buffers(xl, 1 if pooled else B)
    ptr = lambda im: im.ptr if im is not None else None
    fn = getattr(ctx.lib, "sbtv_" + entry)
    ctx.check(fn(ctx.h, yi.ptr, M, N, B, _vp(taps), A.taille, hp, K, int(levels), C.byref(o), keep[0][1], keep[1][1], ptr(x0i),
                 nz_ptr, _vp(gx), _vp(logpi), xl.ptr, C.byref(mo) if mo is not None else None, ptr(pm), ptr(pv),
                 _vp(pc) if pc is not None else None, ptr(cm), ptr(cv), yi.flags), yi.flags)
    xs = L.images_result(xl, False)
    moments = {}
    if mo is not None:
        moments = {k: L.images_result(v, False) for k, v in (("posteriormean", pm), ("posteriorvar", pv), ("coefmean", cm),
                                                             ("coefvar", cv)) if v is not None}
    results = []
    for b in range(B):
        r = dict(Xlast_sample=xs[b], gXTrace=gx[b], logPiTraceX=logpi[b], options=op)
        for k, v in moments.items():
            r[k] = v[0 if pooled else b]
        if mo is not None:
            r["posteriorcount"] = int(pc[0 if pooled else b])
        results.append(r)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    return results[0] if sq else results


def myula_wavelet(y, A, h, levels, op, theta=None, sigma2=None, noise=None, xw0=None, posterior=None, ctx=None):
    """results = myula_wavelet(y, A, h, levels, op, theta, sigma2)

    MYULA chain on the wavelet coefficients at a FIXED theta: samples of p(xw | y, theta) ~ exp(-||y - A W xw||^2 / (2 sigma2)
    - theta ||xw||_1), e.g. at the theta_EB of SAPG_wavelet, with the posterior mean (the MMSE image) and variance of the
    samples accumulated on the device.  It is the warm-up loop of SALSA/SAPG_algorithm_1.m:131-141 with the closures of
    run_deblur_synthesis_L1.m:135-146 (include/sbtv.h, sbtv_myula_wavelet, states it); iteration 1 is the start state, samples-1
    steps follow.
    A, h, levels: as for SAPG_wavelet.  op (dict or object): samples, lambda, gamma; optional theta, sigma2 (or sigma), X0, seed
    (1), chain_offset (0).  theta / sigma2 (default op.theta / op.sigma2): a scalar or one value per image of a batch.
    noise: optional (samples-1, [B,] M, (3J+1) N) normals instead of the device Philox stream, as for SAPG_wavelet.
    posterior: None (no moments), True, or dict(first=1, thin=1, pooled=False, coefficients=False): the iterations first,
    first + thin, ... of 1..samples; pooled: one set over the chains of the call (chains of one posterior only);
    coefficients: also the mean / variance per coefficient.
    Returns a dict (a list of dicts for a batch): Xlast_sample, gXTrace (||X(ii)||_1), logPiTraceX, options, and with posterior:
    posteriormean, posteriorvar (images W X(ii)), posteriorcount, and coefmean, coefvar when coefficients are requested.
    Device tensors in give device tensors out."""
    def make_opts():
        o = L.sbtv_myula_wavelet_opts()
        o.gamma = float(_op(op, "gamma"))
        return o
    return _fixed_theta_chain("myula_wavelet", make_opts, None, y, A, h, levels, op, theta, sigma2, noise, xw0, posterior, ctx)


def skrock_coefficients(stages, eta=0.05):
    """The SK-ROCK table of include/sbtv.h (sbtv_skrock_coefficients, host arithmetic): dict(mu, nu, kappa: arrays of
    `stages` entries, entry j-1 for stage j; omega0, omega1, ls)."""
    s = int(stages)
    mu, nu, kappa, om, ls = np.zeros(max(s, 1)), np.zeros(max(s, 1)), np.zeros(max(s, 1)), np.zeros(2), np.zeros(1)
    lib = L.load_library()
    rc = lib.sbtv_skrock_coefficients(s, float(eta), _vp(mu), _vp(nu), _vp(kappa), _vp(om), _vp(ls))
    if rc != 0:
        raise L.SbtvError(rc, lib.sbtv_last_error(None).decode())
    return dict(mu=mu, nu=nu, kappa=kappa, omega0=float(om[0]), omega1=float(om[1]), ls=float(ls[0]))


def skrock_max_step(stages, eta, sigma2, lam, normB2=1.0):
    """The largest stable SK-ROCK step l_s / (normB2 / sigma2 + 1 / lam) (sbtv_skrock_max_step, host arithmetic);
    normB2 = ||B||^2 is 1 for a normalised non-negative PSF."""
    out = C.c_double(0.0)
    lib = L.load_library()
    rc = lib.sbtv_skrock_max_step(int(stages), float(eta), float(sigma2), float(lam), float(normB2), C.byref(out))
    if rc != 0:
        raise L.SbtvError(rc, lib.sbtv_last_error(None).decode())
    return out.value


def skrock_wavelet(y, A, h, levels, op, theta=None, sigma2=None, noise=None, xw0=None, posterior=None, ctx=None):
    """results = skrock_wavelet(y, A, h, levels, op, theta, sigma2)

    SK-ROCK chain on the wavelet coefficients at a FIXED theta: the target, arguments and results of myula_wavelet, with the
    explicit stabilised step of Pereyra, Vargas Mieles and Zygalakis (2020) (include/sbtv.h, sbtv_skrock_wavelet, states it):
    `stages` gradient evaluations per step, a step delta of about stages^2 (2 - 4 eta / 3) times MYULA's gamma.  Sample 1 is
    the start state, samples-1 steps follow.
    op (dict or object): samples, stages, lambda; optional delta (None: 0.8 skrock_max_step(stages, eta, the smallest sigma2, lambda)
    with ||B||^2 = 1), eta (0.05), theta, sigma2 (or sigma), X0, seed (1), chain_offset (0).
    theta, sigma2, noise, xw0, posterior and the returned keys: as for myula_wavelet."""
    def make_opts():
        o = L.sbtv_skrock_wavelet_opts()
        o.stages = int(_op(op, "stages"))
        o.eta = float(_op(op, "eta", 0.05))
        return o

    def finish_opts(o, s2):
        delta = op.get("delta") if isinstance(op, dict) else getattr(op, "delta", None)
        if delta is None:
            # the stiffest chain of the call sets the step; arguments the bound cannot be formed from are the library's to refuse
            s2 = float(np.min(s2))
            ok = o.stages >= 2 and all(np.isfinite(v) and v > 0 for v in (o.eta, s2, o.lambda_))
            delta = 0.8 * skrock_max_step(o.stages, o.eta, s2, o.lambda_) if ok else float("nan")
        o.delta = float(delta)
    return _fixed_theta_chain("skrock_wavelet", make_opts, finish_opts, y, A, h, levels, op, theta, sigma2, noise, xw0, posterior,
                              ctx)


_PSF_KIND = {"gaussian": 0, "moffat": 1, "laplace": 2}


def _pair(v, npar, fill=0.0):
    """A one- or two-element option as a 2-vector (a one-parameter family leaves slot 1 at `fill`)."""
    a = np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()
    if a.size < npar or a.size > 2:
        raise ValueError("a per-parameter option must have one entry per PSF parameter")
    out = np.full(2, float(fill))
    out[:a.size] = a
    return out


def SAPG_wavelet_semiblind(y, kind, h, levels, op, noise=None, xw0=None, ctx=None):
    """[eb, results] = SAPG_wavelet_semiblind(y, kind, h, levels, op)

    Semi-blind empirical Bayes for the wavelet-l1 prior: theta, the parameters p of a PSF family and sigma2 estimated together
    from one device-resident MYULA chain on the wavelet coefficients.  It is SALSA/SAPG_algorithm_1.m with both of its
    parameters, `tau` being the PSF parameters with the closures of the TV half of this package (include/sbtv.h,
    sbtv_SAPG_wavelet_semiblind, states the loop).  No blur operator is given: the blur is psf_family(kind, psf_size, p).
    kind: "gaussian" (w1, w2), "moffat" (alpha, beta) or "laplace" (b); h, levels: the frame, as for mrdwt_TI2D.
    op (dict or object): everything SAPG_wavelet takes (sigma / sigma2 is sigma2(1), the noise variance itself while
    fix_sigma), and p_init (one or two values, or one row per image of a batch); optional psf_size (7), phi (0), fix_p
    (all free), p_true (p_init), p_min / p_max (required for a free parameter; p_true for a fixed one), c_p (1 each),
    fix_sigma (True), and for a free sigma2: sigma2_min, sigma2_max, c_sigma.
    noise, xw0: as for SAPG_wavelet, the same device-noise validation.
    Returns eb = dict(theta, p, sigma2) (arrays per image for a batch) and results with the keys of SAPG_wavelet plus ps
    (2, samples), sigmas, grads (3, samples: G_p0, G_p1, G_sigma2), mean_ps, tol_ps, p_EB, sigma2_EB, mean_theta.  Then e.g.
    psf_family(kind, psf_size, p_EB) -> SALSA_wavelet / myula_wavelet."""
    ctx = ctx or L.default_context()
    if getattr(ctx, "is_group", False):
        raise NotImplementedError("SAPG_wavelet_semiblind has no sharded variant")
    yi = L.Images(y)
    B, M, N = yi.B, yi.M, yi.N
    nb = max(_bands(levels), 1)
    ha, hp, K = _filter(h)
    get = lambda name, default=None: op.get(name, default) if isinstance(op, dict) else getattr(op, name, default)
    o = L.sbtv_sapg_wavelet_sb_opts()
    o.samples = int(_op(op, "samples"))
    o.warmup = int(_op(op, "warmup", 0))
    o.burnIn = int(_op(op, "burnIn"))
    o.lambda_ = float(_op(op, "lambda"))
    o.gamma = float(_op(op, "gamma"))
    s2 = get("sigma2")
    o.sigma2 = float(s2) if s2 is not None else float(_op(op, "sigma")) ** 2
    o.th_init = float(_op(op, "th_init"))
    o.min_th = float(_op(op, "min_th"))
    o.max_th = float(_op(op, "max_th"))
    o.d_scale = float(_op(op, "d_scale"))
    o.d_exp = float(_op(op, "d_exp"))
    o.seed = int(_op(op, "seed", 1))
    o.chain_offset = int(_op(op, "chain_offset", 0))
    o.kind = _PSF_KIND[kind] if isinstance(kind, str) else int(kind)
    npar = 1 if o.kind == 2 else 2
    o.psf_size = int(_op(op, "psf_size", 7))
    o.phi = float(_op(op, "phi", 0.0))
    pin = np.asarray(_op(op, "p_init"), dtype=np.float64)
    if pin.ndim == 2:
        if pin.shape[0] != B:
            raise ValueError("p_init must have one row per image")
        pstart = np.ascontiguousarray(np.stack([_pair(r, npar) for r in pin]))
    else:
        pstart = np.ascontiguousarray(np.tile(_pair(pin, npar), (B, 1)))
    fix = np.atleast_1d(np.asarray(get("fix_p", [False] * npar))).ravel().astype(bool)
    fix = np.concatenate([fix, np.ones(2 - fix.size, dtype=bool)])
    ptrue = _pair(get("p_true", pstart[0, :npar]), npar)
    c_p = _pair(get("c_p", [1.0] * npar), npar)
    pmin, pmax = get("p_min"), get("p_max")
    if (pmin is None or pmax is None) and not all(fix[:npar]):
        raise KeyError("op.p_min and op.p_max are required for a free PSF parameter")
    pmin = ptrue.copy() if pmin is None else _pair(pmin, npar)
    pmax = ptrue.copy() if pmax is None else _pair(pmax, npar)
    for q in range(2):
        o.fix_p[q] = int(fix[q])
        o.p_init[q], o.p_true[q], o.p_min[q], o.p_max[q], o.c_p[q] = pstart[0, q], ptrue[q], pmin[q], pmax[q], c_p[q]
    o.fix_sigma = int(bool(_op(op, "fix_sigma", True)))
    if o.fix_sigma:
        o.sigma2_min, o.sigma2_max = float(get("sigma2_min", o.sigma2)), float(get("sigma2_max", o.sigma2))
        o.c_sigma = float(get("c_sigma", 0.0))
    else:
        o.sigma2_min, o.sigma2_max = float(_op(op, "sigma2_min")), float(_op(op, "sigma2_max"))
        o.c_sigma = float(_op(op, "c_sigma"))
    S, Wn = o.samples, max(o.warmup, 0)
    if xw0 is None:
        xw0 = get("X0")
    x0i = L.Images(xw0) if xw0 is not None else None
    if x0i is not None:
        if (x0i.B, x0i.M, x0i.N) != (B, M, nb * N):
            raise ValueError("coefficient arrays must be (M, (3 (levels-1) + 1) N) per image")
        if x0i.flags != yi.flags:
            raise ValueError("all image arguments must live in the same memory space")
    nz_keep, nz_ptr = _chain_noise(noise, yi, max(Wn - 1, 0) + S - 1, nb, "max(warmup-1, 0) + samples-1")
    Sn, Mn = max(S, 1), max(S - o.burnIn, 1)
    thetas, sigmas, gx, logpi, tol = (np.zeros((B, Sn)) for _ in range(5))
    ps, tolp, grads = np.zeros((B, 2, Sn)), np.zeros((B, 2, Sn)), np.zeros((B, 3, Sn))
    logpi_wu = np.zeros((B, max(Wn, 1)))
    means, meanp = np.zeros((B, Mn)), np.zeros((B, 2, Mn))
    eb = np.zeros((B, 4))
    xl = _resized(yi, nb * N)
    ctx.check(ctx.lib.sbtv_SAPG_wavelet_semiblind(
        ctx.h, yi.ptr, M, N, B, hp, K, int(levels), C.byref(o), _vp(pstart), x0i.ptr if x0i else None, nz_ptr, _vp(thetas),
        _vp(ps), _vp(sigmas), _vp(gx), _vp(logpi), _vp(logpi_wu), _vp(grads), _vp(means), _vp(tol), _vp(meanp), _vp(tolp),
        _vp(eb), xl.ptr, yi.flags), yi.flags)
    xs = L.images_result(xl, False)
    nm = max(S - o.burnIn, 0)
    results = []
    for b in range(B):
        r = dict(last_samp=S, logPiTraceX=logpi[b], gXTrace=gx[b], mean_theta=float(eb[b, 0]), last_theta=float(thetas[b, -1]),
                 thetas=thetas[b], mean_thetas=means[b, :nm], tol_thetas=tol[b], ps=ps[b], sigmas=sigmas[b], grads=grads[b],
                 mean_ps=meanp[b, :, :nm], tol_ps=tolp[b], p_EB=eb[b, 1:1 + npar].copy(), sigma2_EB=float(eb[b, 3]),
                 options=op, Xlast_sample=xs[b])
        if Wn > 0:
            r["logPiTrace_WU"] = logpi_wu[b, :Wn]
        results.append(r)
    sq = (y.dim() == 2) if yi.torch else yi.squeeze
    if sq:
        return dict(theta=float(eb[0, 0]), p=eb[0, 1:1 + npar].copy(), sigma2=float(eb[0, 3])), results[0]
    return dict(theta=eb[:, 0].copy(), p=eb[:, 1:1 + npar].copy(), sigma2=eb[:, 3].copy()), results
