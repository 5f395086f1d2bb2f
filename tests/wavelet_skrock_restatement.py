"""NumPy restatement of the SK-ROCK chain on the wavelet coefficients at a fixed theta (include/sbtv.h, sbtv_skrock_wavelet),
built on the operators of tests/wavelet_sapg_restatement.py: the coefficient table and the step exactly as the header states
them, every sample kept with its image W X(ii), gx(ii) = ||X(ii)||_1 and logpi(ii) = -||y - B W X(ii)||^2 / (2 sigma2) -
theta gx(ii), ii = 1..samples.  Nothing here imports the library."""
import math

import numpy as np

import wavelet_restatement as wr
import wavelet_sapg_restatement as wsr


def chebyshev(s, w0):
    """T_0..T_s and U_0..U_s at w0 (first / second kind)."""
    T, U = [1.0, w0], [1.0, 2.0 * w0]
    for j in range(2, s + 1):
        T.append(2.0 * w0 * T[j - 1] - T[j - 2])
        U.append(2.0 * w0 * U[j - 1] - U[j - 2])
    return T, U


def coefficients(s, eta=0.05):
    """dict(mu, nu, kappa: arrays of s entries, entry j - 1 for stage j; omega0, omega1, ls, T: T_0..T_s at omega0)."""
    s = int(s)
    assert s >= 2 and eta > 0
    w0 = 1.0 + eta / (float(s) * float(s))
    T, U = chebyshev(s, w0)
    w1 = T[s] / (float(s) * U[s - 1])
    mu, nu, kappa = np.zeros(s), np.zeros(s), np.zeros(s)
    mu[0] = w1 / w0
    nu[0] = float(s) * w1 / 2.0
    kappa[0] = float(s) * w1 / w0
    for j in range(2, s + 1):
        mu[j - 1] = 2.0 * w1 * T[j - 1] / T[j]
        nu[j - 1] = 2.0 * w0 * T[j - 1] / T[j]
        kappa[j - 1] = 1.0 - nu[j - 1]
    ls = (float(s) - 0.5) * (float(s) - 0.5) * (2.0 - 4.0 * eta / 3.0) - 1.5
    return dict(mu=mu, nu=nu, kappa=kappa, omega0=w0, omega1=w1, ls=ls, T=np.array(T))


def max_step(s, eta, sigma2, lam, normB2=1.0):
    return coefficients(s, eta)["ls"] / (normB2 / sigma2 + 1.0 / lam)


def step(X, Z, drift, c, delta):
    """One step from X with the normals Z; drift(K) = D(K).  Works on arrays and on scalars."""
    s = len(c["mu"])
    q = math.sqrt(2 * delta)
    P = X + (c["nu"][0] * q) * Z
    K1 = (X + (c["mu"][0] * delta) * drift(P)) + (c["kappa"][0] * q) * Z
    K0 = X
    for j in range(2, s + 1):
        Kj = ((c["mu"][j - 1] * delta) * drift(K1) + c["nu"][j - 1] * K1) + c["kappa"][j - 1] * K0
        K0, K1 = K1, Kj
    return K1


def skrock_wavelet_chain(y, H, h, levels, op, theta, sigma2, noise, xw0=None):
    """op: dict(samples, stages, lambda, delta, eta (0.05)); noise: (samples-1, M, (3J+1) N); xw0: X(1) (None: W'y).  Returns
    dict(samples (S, M, (3J+1) N), images (S, M, N), gx (S,), logpi (S,))."""
    y = np.asarray(y, dtype=np.float64)
    W, WT, B, BT = wsr._operators(y, H, h, levels)
    lam, delta, S = op["lambda"], op["delta"], int(op["samples"])
    c = coefficients(op["stages"], op.get("eta", 0.05))

    def drift(K):
        G = WT(BT(B(W(K)) - y))
        return (wr.soft(K, lam * theta) - K) / lam - G / sigma2

    X = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    Xs, images, gx, logpi = [], [], np.zeros(S), np.zeros(S)
    for ii in range(1, S + 1):
        if ii > 1:
            X = step(X, noise[ii - 2], drift, c, delta)
        img = W(X)
        Xs.append(X)
        images.append(img)
        gx[ii - 1] = float(np.sum(np.abs(X)))
        logpi[ii - 1] = -wr._sq(y - B(img)) / (2 * sigma2) - theta * gx[ii - 1]
    return dict(samples=np.stack(Xs), images=np.stack(images), gx=gx, logpi=logpi)
