"""NumPy restatement of the masked-observation SALSA iteration (include/sbtv.h, sbtv_SALSA_masked): the ADMM of Almeida &
Figueiredo (IEEE TIP 2013) for  min_x 0.5 sum(m .* (B x - y).^2) + tau TV(x)  with the splits u = x and v = B x, written
line for line as the header states it, on the oracle's chambolle_prox_TV_stop / TVnorm / fft2.  The reference has no such
solver (SALSA/SALSA.m:103-104,308-312,463-464 takes a mask OR a blur), so the tests anchor this restatement on
sbtv_oracle.SALSA_v2 for m = 1 (tests/test_masked_cpu.py) and hold the GPU against it (tests/test_gpu_masked.py)."""
import math
import time

import numpy as np

import sbtv_oracle as o


def spectrum_of_taps(taps, shape):
    """fft2 of the taps embedded top-left (utils/resize.m)."""
    return o.resize(np.atleast_2d(np.asarray(taps, dtype=np.float64)), tuple(shape))


def valid_convolution(x, taps):
    """'valid' part of the LINEAR convolution of x with the taps, as an explicit sum (no FFT): (M-t+1) x (N-t+1)."""
    taps = np.atleast_2d(np.asarray(taps, dtype=np.float64))
    t = taps.shape[0]
    M, N = x.shape
    out = np.zeros((M - t + 1, N - t + 1))
    for a in range(t):
        for b in range(t):
            out += taps[a, b] * x[t - 1 - a:M - a, t - 1 - b:N - b]
    return out


def salsa_masked(y, mask, H, tau, mu1, mu2=0.1, true_x=None, stopcriterion=1, tolA=1e-3, maxiter=10000, TViters=5,
                 initialization=0):
    """Returns dict(x, numA, numAt, objective, distance, times, mses, n_outer).  H: fft2 of the embedded taps."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    Hc = np.conj(H)
    H2 = np.abs(H) ** 2
    B = lambda z: np.real(o.ifft2(H * o.fft2(z)))
    Bt = lambda z: np.real(o.ifft2(Hc * o.fft2(z)))
    numA = numAt = 0
    if isinstance(initialization, np.ndarray):
        x = np.array(initialization, dtype=np.float64)
    elif initialization == 0:
        x = np.zeros_like(y)
    elif initialization == 2:
        x = Bt(m * y)
        numAt += 1
    else:
        raise ValueError("Unknown 'Initialization' option")
    Bx = B(x)
    numA += 1
    u = x.copy()
    v = Bx.copy()
    bu = np.zeros_like(x)
    bv = np.zeros_like(x)
    pux = np.zeros_like(x)
    puy = np.zeros_like(x)
    objective = [0.5 * float(np.sum(m * (Bx - y) ** 2)) + tau * o.TVnorm(u)]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []
    times = [0.0]
    distance = []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = x
        u, pux, puy = o.chambolle_prox_TV_stop(x - bu, lam=tau / mu1, maxiter=TViters, dualvars=(pux, puy))
        v = (m * y + mu2 * (Bx - bv)) / (m + mu2)
        X = (mu1 * o.fft2(u + bu) + mu2 * Hc * o.fft2(v + bv)) / (mu1 + mu2 * H2)
        numAt += 1
        x = np.real(o.ifft2(X))
        Bx = np.real(o.ifft2(H * X))
        numA += 1
        bu = bu + (u - x)
        bv = bv + (v - Bx)
        objective.append(0.5 * float(np.sum(m * (Bx - y) ** 2)) + tau * o.TVnorm(u))
        if true_x is not None:
            e = x - true_x
            mses.append(float(np.sum(e * e)) / x.size)
        distance.append([float(np.linalg.norm((x - u).ravel())) / math.sqrt(float(np.sum(x * x)) + float(np.sum(u * u))),
                         float(np.linalg.norm((Bx - v).ravel())) / math.sqrt(float(np.sum(Bx * Bx)) + float(np.sum(v * v)))])
        times.append(time.perf_counter() - t0)
        if outer > 1:
            if stopcriterion == 1:
                crit = abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]
            elif stopcriterion == 2:
                crit = abs(float(np.linalg.norm((x - xprev).ravel())) / float(np.linalg.norm(x.ravel())))
            else:
                crit = objective[outer]
            if crit < tolA:
                break
    return dict(x=x, numA=numA, numAt=numAt, objective=np.array(objective), distance=np.array(distance).reshape(-1, 2),
                times=np.array(times), mses=np.array(mses), n_outer=n_outer, u=u, v=v, bu=bu, bv=bv)


def psnr_over(mask, x_true, x):
    """PSNR (peak 255, utils/PSNR.m) over the pixels where mask is non-zero."""
    sel = np.asarray(mask) > 0
    return 10.0 * math.log10(255.0 ** 2 / float(np.mean((x_true[sel] - x[sel]) ** 2)))
