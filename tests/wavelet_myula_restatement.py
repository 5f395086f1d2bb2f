"""NumPy restatement of the MYULA chain on the wavelet coefficients at a fixed theta (include/sbtv.h, sbtv_myula_wavelet),
built on the operators of tests/wavelet_sapg_restatement.py.  The chain is the warm-up loop of SALSA/SAPG_algorithm_1.m:131-141
with the closures of SALSA/run_deblur_synthesis_L1.m:135-146 (proxG = soft, g = l1, gradF = W'B'(B W xw - y) / sigma2) at the
caller's theta; every sample is kept, with its image W X(ii), gx(ii) = ||X(ii)||_1 and
logpi(ii) = -||y - B W X(ii)||^2 / (2 sigma2) - theta gx(ii), ii = 1..samples.  Nothing here imports the library."""
import math

import numpy as np

import wavelet_restatement as wr
import wavelet_sapg_restatement as wsr


def myula_wavelet_chain(y, H, h, levels, op, theta, sigma2, noise, xw0=None):
    """op: dict(samples, lambda, gamma); noise: (samples-1, M, (3J+1) N); xw0: X(1) (None: W'y).  Returns dict(samples
    (S, M, (3J+1) N), images (S, M, N), gx (S,), logpi (S,))."""
    y = np.asarray(y, dtype=np.float64)
    W, WT, B, BT = wsr._operators(y, H, h, levels)
    lam, gamma, S = op["lambda"], op["gamma"], int(op["samples"])
    sq2g = math.sqrt(2 * gamma)
    X = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    Xs, images, gx, logpi = [], [], np.zeros(S), np.zeros(S)
    for ii in range(1, S + 1):
        if ii > 1:
            G = WT(BT(B(images[-1]) - y))                                               # gradF sigma2, L1.m:142
            X = ((X + gamma * (wr.soft(X, lam * theta) - X) / lam) - gamma * (G / sigma2)) + sq2g * noise[ii - 2]   # :133
        img = W(X)
        Xs.append(X)
        images.append(img)
        gx[ii - 1] = float(np.sum(np.abs(X)))                                           # L1.m:135
        logpi[ii - 1] = -wr._sq(y - B(img)) / (2 * sigma2) - theta * gx[ii - 1]         # L1.m:146
    return dict(samples=np.stack(Xs), images=np.stack(images), gx=gx, logpi=logpi)


def two_pass(xs):
    xs = np.asarray(xs)
    return xs.mean(axis=0), (xs.var(axis=0, ddof=1) if len(xs) > 1 else np.zeros(xs.shape[1:]))


def welford(xs):
    """The device's update (welford_nocontract) in NumPy: one rounding per operation, so the same bits."""
    mean = m2 = None
    for k, x in enumerate(xs, 1):
        if k == 1:
            mean, m2 = np.array(x, dtype=np.float64), np.zeros_like(x, dtype=np.float64)
            continue
        rk = 1.0 / k
        d = x - mean
        mean = mean + d * rk
        m2 = m2 + d * (x - mean)
    n = len(xs)
    return mean, (m2 / (n - 1.0) if n > 1 else np.zeros_like(mean))
