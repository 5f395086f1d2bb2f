"""NumPy restatement of the empirical-Bayes estimate of theta for the wavelet-l1 prior (include/sbtv.h, sbtv_SAPG_wavelet),
built on tests/wavelet_restatement.py.

`sapg_wavelet_literal` is the theta part of SALSA/SAPG_algorithm_1.m:120-231 line for line, with the operators of
SALSA/run_deblur_synthesis_L1.m:116-146 (A = B W, AT = W' B', proxG = soft, g = l1, gradF = AT(A xw - y) / sigma2) and the
normals injected instead of randn.  The `tau` part of that file (op.to_init, op.grad_t, the two-argument gradF) is left out:
the script defines none of it.  `sapg_wavelet_fused` is the form the library runs: the prox is never stored but recomputed
from X and the theta it was formed with, and the residual of a sample is taken from the next iteration's gradient pass.
Both keep the running sum of eta(burnIn..ii) in iteration order, which is what mean(eta(op.burnIn:ii)) is up to the order of
the additions.  Nothing here imports the library."""
import math

import numpy as np

import wavelet_restatement as wr


def _operators(y, H, h, levels):
    W = lambda c: wr.mirdwt_TI2D(c, h, levels)
    WT = lambda v: wr.mrdwt_TI2D(v, h, levels)
    B = lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v)))
    BT = lambda v: np.real(np.fft.ifft2(np.conj(H) * np.fft.fft2(v)))
    return W, WT, B, BT


def _exp_mean(s, n):
    """exp(mean(eta(burnIn:i))) from the running sum; NaN for an empty window, like MATLAB's mean of an empty range."""
    return math.exp(s / n) if n > 0 else float("nan")


def _results(theta, eta_sum, eta_n, logpi, gx, logpi_wu, mean_thetas, tol_thetas, X, op):
    theta_EB = math.exp(eta_sum / eta_n)                                               # :226
    res = dict(last_samp=op["samples"], logPiTraceX=logpi, gXTrace=gx, mean_theta=theta_EB, last_theta=theta[-1],
               thetas=theta, mean_thetas=mean_thetas, tol_thetas=tol_thetas, options=op, Xlast_sample=X)
    if op["warmup"] > 0:
        res["logPiTrace_WU"] = logpi_wu
    return theta_EB, res


def sapg_wavelet_literal(y, H, h, levels, op, noise, xw0=None):
    """op: dict(samples, warmup, burnIn, lambda, gamma, sigma2, th_init, min_th, max_th, d_scale, d_exp); noise:
    (max(warmup-1, 0) + samples-1, M, (3J+1) N), consumed warm-up first; xw0: op.X0 (None: W'y,
    run_deblur_synthesis_L1.m:153).  Returns (theta_EB, results)."""
    y = np.asarray(y, dtype=np.float64)
    W, WT, B, BT = _operators(y, H, h, levels)
    A = lambda c: B(W(c))
    AT = lambda v: WT(BT(v))
    sigma2, lam, gamma = op["sigma2"], op["lambda"], op["gamma"]
    g = lambda c: float(np.sum(np.abs(c)))                                             # L1.m:135
    proxG = lambda c, la, th: wr.soft(c, th * la)                                      # L1.m:137
    f = lambda c: wr._sq(y - A(c)) / (2 * sigma2)                                      # L1.m:141
    gradF = lambda c: AT(A(c) - y) / sigma2                                            # L1.m:142
    logPi = lambda c, th: -f(c) - th * g(c)                                            # L1.m:146
    X0 = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    dimX = X0.size                                                                     # :86
    total_iter, warmup, burnIn = int(op["samples"]), int(op["warmup"]), int(op["burnIn"])
    eta_init, min_eta, max_eta = math.log(op["th_init"]), math.log(op["min_th"]), math.log(op["max_th"])   # :101-103
    delta = lambda i: op["d_scale"] * (i ** (-op["d_exp"]) / dimX)                     # :111
    sq2g = math.sqrt(2 * gamma)
    step = 0
    X_wu = X0                                                                          # :121
    logpi_wu = np.zeros(max(warmup, 0))
    if warmup > 0:                                                                     # :122
        fix_theta = op["th_init"]
        prox = proxG(X_wu, lam, fix_theta)                                             # :129
        for ii in range(2, warmup + 1):                                                # :131
            X_wu = ((X_wu + gamma * (prox - X_wu) / lam) - gamma * gradF(X_wu)) + sq2g * noise[step]       # :133
            step += 1
            prox = proxG(X_wu, lam, fix_theta)                                         # :134
            logpi_wu[ii - 1] = logPi(X_wu, fix_theta)                                  # :136
    theta, eta = np.zeros(total_iter), np.zeros(total_iter)                            # :145-148
    theta[0], eta[0] = op["th_init"], eta_init
    tol_thetas = np.zeros(total_iter)                                                  # :154
    mean_thetas = np.zeros(max(total_iter - burnIn, 0))                                # :159
    logpi, gx = np.zeros(total_iter), np.zeros(total_iter)                             # :162-163
    X = X_wu                                                                           # :165
    logpi[0] = logPi(X, theta[0])                                                      # :166
    prox = proxG(X, lam, theta[0])                                                     # :167
    eta_sum, eta_n = (eta[0], 1) if burnIn == 1 else (0.0, 0)
    for ii in range(2, total_iter + 1):                                                # :171
        Z = noise[step]                                                                # :173
        step += 1
        X = ((X + gamma * (prox - X) / lam) - gamma * gradF(X)) + sq2g * Z             # :174
        prox = proxG(X, lam, theta[ii - 2])                                            # :175
        gX = g(X)
        etaii = eta[ii - 2] + delta(ii) * (dimX / theta[ii - 2] - gX) * math.exp(eta[ii - 2])              # :180
        eta[ii - 1] = min(max(etaii, min_eta), max_eta)                                # :181
        theta[ii - 1] = math.exp(eta[ii - 1])                                          # :182
        logpi[ii - 1] = -f(X) - theta[ii - 2] * gX                                     # :190
        gx[ii - 2] = gX                                                                # :191
        m0 = _exp_mean(eta_sum, eta_n)                                                 # exp(mean(eta(op.burnIn:ii-1)))
        if ii >= burnIn:
            eta_sum, eta_n = eta_sum + eta[ii - 1], eta_n + 1
        m1 = _exp_mean(eta_sum, eta_n)                                                 # exp(mean(eta(op.burnIn:ii)))
        tol_thetas[ii - 1] = abs(m1 - m0) / m0                                         # :199-200
        if ii > burnIn:
            mean_thetas[ii - burnIn - 1] = m1                                          # :209-211
    return _results(theta, eta_sum, eta_n, logpi, gx, logpi_wu, mean_thetas, tol_thetas, X, op)


def sapg_wavelet_fused(y, H, h, levels, op, noise, xw0=None):
    """The same chain as the library runs it: state X only; each iteration computes r = B W X - y once, which gives both the
    gradient W' B' r and ||r||^2 of the sample BEFORE the step, so every log-density is completed one iteration late and the
    last sample takes one extra residual; the soft threshold is recomputed from X and the lagging theta."""
    y = np.asarray(y, dtype=np.float64)
    W, WT, B, BT = _operators(y, H, h, levels)
    sigma2, lam, gamma = op["sigma2"], op["lambda"], op["gamma"]
    X = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    dimX = X.size
    samples, warmup, burnIn = int(op["samples"]), int(op["warmup"]), int(op["burnIn"])
    eta, min_eta, max_eta = math.log(op["th_init"]), math.log(op["min_th"]), math.log(op["max_th"])
    sq2g = math.sqrt(2 * gamma)
    th_prev = th_cur = op["th_init"]
    theta, tol_thetas, logpi, gx = np.zeros(samples), np.zeros(samples), np.zeros(samples), np.zeros(samples)
    theta[0] = th_cur
    mean_thetas = np.zeros(max(samples - burnIn, 0))
    logpi_wu = np.zeros(max(warmup, 0))
    eta_sum, eta_n = (eta, 1) if burnIn == 1 else (0.0, 0)

    def step(X, Z, th):
        r = B(W(X)) - y
        G = WT(BT(r))
        Xn = ((X + gamma * (wr.soft(X, lam * th) - X) / lam) - gamma * (G / sigma2)) + sq2g * Z
        return Xn, wr._sq(r), float(np.sum(np.abs(Xn)))

    s = 0
    g_last = float(np.sum(np.abs(X))) if warmup < 2 else 0.0
    for ii in range(2, warmup + 1):
        X, R, g = step(X, noise[s], th_prev)
        s += 1
        if ii > 2:
            logpi_wu[ii - 2] = -R / (2 * sigma2) - th_prev * g_last
        g_last = g
    for ii in range(2, samples + 1):
        X, R, g = step(X, noise[s], th_prev)
        s += 1
        lp = -R / (2 * sigma2) - th_prev * g_last
        if ii == 2 and warmup >= 2:
            logpi_wu[warmup - 1] = lp
        logpi[ii - 2] = lp
        etaii = eta + op["d_scale"] * (ii ** (-op["d_exp"]) / dimX) * (dimX / th_cur - g) * math.exp(eta)
        eta = min(max(etaii, min_eta), max_eta)
        th = math.exp(eta)
        theta[ii - 1], gx[ii - 2] = th, g
        m0 = _exp_mean(eta_sum, eta_n)
        if ii >= burnIn:
            eta_sum, eta_n = eta_sum + eta, eta_n + 1
        m1 = _exp_mean(eta_sum, eta_n)
        tol_thetas[ii - 1] = abs(m1 - m0) / m0
        if ii > burnIn:
            mean_thetas[ii - burnIn - 1] = m1
        th_prev, th_cur, g_last = th_cur, th, g
    R = wr._sq(B(W(X)) - y)
    logpi[samples - 1] = -R / (2 * sigma2) - th_prev * g_last
    return _results(theta, eta_sum, eta_n, logpi, gx, logpi_wu, mean_thetas, tol_thetas, X, op)
