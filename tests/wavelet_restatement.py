"""NumPy restatement of the redundant wavelet frame and of the wavelet-l1 SALSA iteration (include/sbtv.h,
sbtv_mrdwt_TI2D / sbtv_mirdwt_TI2D / sbtv_SALSA_wavelet).

The reference calls the Rice Wavelet Toolbox MEX through SALSA/mrdwt_TI2D.m and mirdwt_TI2D.m, and that MEX is not shipped
(SALSA/mrdwt.m is a comment block), so the transform is restated here from its definition with np.roll; its 1-D convention
is held against the worked example of that comment block (tests/test_wavelet_cpu.py).  `salsa_wavelet_literal` is
SALSA/SALSA_v2.m:389-494 line for line with Psi = soft, Phi = l1 and the invLS of SALSA/run_deblur_synthesis_L1.m:169-170;
`salsa_wavelet_operator` is the form the library runs.  Nothing here imports the library."""
import math
import time

import numpy as np

SQRT2 = math.sqrt(2.0)


def filters(h):
    """(h0, h1): h0 = h, h1[k] = (-1)^k h[K-1-k]."""
    h = np.asarray(h, dtype=np.float64)
    K = h.size
    return h, np.array([(-1.0) ** k * h[K - 1 - k] for k in range(K)])


def _shift_add(out, a, fk, sh, axis):
    """out += fk * np.roll(a, -sh, axis), without the rolled copy."""
    n = a.shape[axis]
    sh %= n
    if axis == 1:
        out, a = out.T, a.T
    if sh == 0:
        out += fk * a
    else:
        out[:n - sh] += fk * a[sh:]
        out[n - sh:] += fk * a[:sh]


def _filt(a, f, s, axis):
    """sum_k f[k] a[(i + s k) mod n] / sqrt 2 along `axis`."""
    out = np.zeros_like(a)
    for k, fk in enumerate(f):
        _shift_add(out, a, fk, s * k, axis)
    out /= SQRT2
    return out


def _filt_adj(c, f, s, axis):
    """The transpose of _filt: sum_k f[k] c[(i - s k) mod n] / sqrt 2."""
    out = np.zeros_like(c)
    for k, fk in enumerate(f):
        _shift_add(out, c, fk, -s * k, axis)
    out /= SQRT2
    return out


def check_size(shape, K, levels):
    if K % 2 or not 2 <= K <= 8 or levels < 2:
        raise ValueError("bad filter length or levels")
    if (K - 1) * 2 ** (levels - 2) >= min(shape):
        raise ValueError("the image is too small for this depth")


def mrdwt_TI2D(x, h, levels):
    """Analysis W': (M, N) -> (M, (3J+1) N), J = levels - 1: [a_J | LH1 HL1 HH1 | LH2 ...] (first letter: dimension 1)."""
    x = np.asarray(x, dtype=np.float64)
    h0, h1 = filters(h)
    check_size(x.shape, h0.size, levels)
    a, det = x, []
    for j in range(1, levels):
        s = 2 ** (j - 1)
        lo, hi = _filt(a, h0, s, 0), _filt(a, h1, s, 0)
        det += [_filt(lo, h1, s, 1), _filt(hi, h0, s, 1), _filt(hi, h1, s, 1)]
        a = _filt(lo, h0, s, 1)
    return np.hstack([a] + det)


def mirdwt_TI2D(z, h, levels):
    """Synthesis W, the exact adjoint of mrdwt_TI2D: (M, (3J+1) N) -> (M, N)."""
    z = np.asarray(z, dtype=np.float64)
    h0, h1 = filters(h)
    J = levels - 1
    N = z.shape[1] // (3 * J + 1)
    check_size((z.shape[0], N), h0.size, levels)
    band = lambda b: z[:, b * N:(b + 1) * N]
    a = band(0)
    for j in range(J, 0, -1):
        s = 2 ** (j - 1)
        lh, hl, hh = (band(1 + 3 * (j - 1) + q) for q in range(3))
        lo = _filt_adj(a, h0, s, 1) + _filt_adj(lh, h1, s, 1)
        hi = _filt_adj(hl, h0, s, 1) + _filt_adj(hh, h1, s, 1)
        a = _filt_adj(lo, h0, s, 0) + _filt_adj(hi, h1, s, 0)
    return a


def soft(x, T):
    """sign(x) max(|x| - T, 0)."""
    m = np.abs(x)
    m -= T
    np.maximum(m, 0.0, out=m)
    return np.copysign(m, x, out=m)


def daub_closed_form(N):
    """Haar and D4 scaling filters in closed form."""
    if N == 2:
        return np.array([1.0, 1.0]) / SQRT2
    if N == 4:
        r3 = math.sqrt(3.0)
        return np.array([1 + r3, 3 + r3, 3 - r3, 1 - r3]) / (4 * SQRT2)
    raise ValueError(N)


def _sq(a):
    """sum(a .^ 2) in one pass."""
    a = a.ravel()
    return float(np.dot(a, a))


def _traces(objective, distance, times, mses):
    return dict(objective=np.array(objective), distance=np.array(distance), times=np.array(times), mses=np.array(mses))


def _stop(stopcriterion, objective, outer, xw, xprev, tolA):
    if stopcriterion == 1:
        crit = abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]
    elif stopcriterion == 2:
        crit = abs(float(np.linalg.norm((xw - xprev).ravel())) / float(np.linalg.norm(xw.ravel())))
    else:
        crit = objective[outer]
    return crit < tolA


def salsa_wavelet_literal(y, H, h, levels, tau, mu, true_xw=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                          initialization=0):
    """SALSA_v2.m:262-494 with TVINITIALIZATION = 0, Psi = soft, Phi = l1, A = B W, AT = W' B', P = PT = identity and
    invLS(r) = (r - W'(real(ifft2(filter .* fft2(W r))))) / mu, filter = conj(H) H / (|H|^2 + mu).  H: fft2 of the PSF."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")
    y = np.asarray(y, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    B = lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v)))
    BT = lambda v: np.real(np.fft.ifft2(np.conj(H) * np.fft.fft2(v)))
    A = lambda c: B(W(c))
    AT = lambda v: WT(BT(v))
    filt = np.conj(H) / (np.abs(H) ** 2 + mu) * H
    invLS = lambda r: (r - WT(np.real(np.fft.ifft2(filt * np.fft.fft2(W(r)))))) / mu
    numA = numAt = 0
    ATy = AT(y)                                              # :288
    numAt += 1
    if isinstance(initialization, np.ndarray):
        x = np.array(initialization, dtype=np.float64)       # :374-378
    elif initialization == 0:
        x = AT(np.zeros_like(y))                             # :369
    elif initialization == 2:
        x = ATy.copy()                                       # :373
    else:
        raise ValueError("Unknown 'Initialization' option")
    u = x.copy()                                             # :392
    bu = np.zeros_like(u)                                    # :393
    threshold = tau / mu                                     # :394
    resid = y - A(x)                                         # :399
    numA += 1
    objective = [0.5 * _sq(resid) + tau * float(np.sum(np.abs(u)))]     # :401
    times = [0.0]
    mses = [float(np.sum((x - true_xw) ** 2)) / x.size] if true_xw is not None else []    # :414
    distance = []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):                 # :423
        n_outer = outer
        xprev = x
        u = soft(x - bu, threshold)                          # :432
        r = ATy + mu * (u + bu)                              # :434
        x = invLS(r)                                         # :436
        bu = bu + (u - x)                                    # :440
        resid = y - A(x)                                     # :442
        numA += 1
        objective.append(0.5 * _sq(resid) + tau * float(np.sum(np.abs(u))))   # :444
        if true_xw is not None:
            e = x - true_xw
            mses.append(_sq(e) / x.size)       # :446-449
        distance.append(math.sqrt(_sq(x - u)) /
                        math.sqrt(_sq(x) + _sq(u)))           # :451
        times.append(time.perf_counter() - t0)
        if outer > 1 and _stop(stopcriterion, objective, outer, x, xprev, tolA):          # :453-482
            break
    return dict(xw=x, x=W(x), numA=numA, numAt=numAt, n_outer=n_outer, u=u, bu=bu,
                **_traces(objective, distance, times, mses))


def salsa_wavelet_operator(y, H, h, levels, tau, mu, true_xw=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                           initialization=0):
    """The same iteration in the form the library runs (include/sbtv.h, sbtv_SALSA_wavelet): with W W' = I it needs one
    synthesis, one spectral solve in the image domain and one analysis per outer iteration, and no division by mu."""
    y = np.asarray(y, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    Y = np.fft.fft2(y)
    Hc, H2 = np.conj(H), np.abs(H) ** 2
    if isinstance(initialization, np.ndarray):
        xw = np.array(initialization, dtype=np.float64)
    elif initialization == 0:
        xw = WT(np.zeros_like(y))
    elif initialization == 2:
        xw = WT(np.real(np.fft.ifft2(Hc * Y)))
    else:
        raise ValueError("Unknown 'Initialization' option")
    numA, numAt = 1, 1
    u = xw.copy()
    bu = np.zeros_like(xw)
    resid = y - np.real(np.fft.ifft2(H * np.fft.fft2(W(xw))))
    objective = [0.5 * _sq(resid) + tau * float(np.sum(np.abs(u)))]
    times = [0.0]
    mses = [float(np.sum((xw - true_xw) ** 2)) / xw.size] if true_xw is not None else []
    distance = []
    t0 = time.perf_counter()
    n_outer = 0
    xi = None
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = xw
        u = soft(xw - bu, tau / mu)
        s = u + bu
        z = W(s)
        X = (Hc * Y + mu * np.fft.fft2(z)) / (H2 + mu)
        xi = np.real(np.fft.ifft2(X))
        we = WT(xi - z)
        xw = s + we
        bu = -we
        resid = y - np.real(np.fft.ifft2(H * X))
        numA += 1
        objective.append(0.5 * _sq(resid) + tau * float(np.sum(np.abs(u))))
        if true_xw is not None:
            e = xw - true_xw
            mses.append(_sq(e) / xw.size)
        distance.append(math.sqrt(_sq(xw - u)) /
                        math.sqrt(_sq(xw) + _sq(u)))
        times.append(time.perf_counter() - t0)
        if outer > 1 and _stop(stopcriterion, objective, outer, xw, xprev, tolA):
            break
    return dict(xw=xw, x=xi if xi is not None else W(xw), numA=numA, numAt=numAt, n_outer=n_outer, u=u, bu=bu,
                **_traces(objective, distance, times, mses))
