"""NumPy restatement of the SK-ROCK chain on the TV posterior at fixed parameters (include/sbtv.h, sbtv_skrock): the step and
the coefficient table of tests/wavelet_skrock_restatement.py (the header states ONE step for both samplers) on the drift

    D(K) = (prox(K) - K) / lambda - AT(A K - y) / sigma2,    prox(K) = chambolle_prox_TV_stop(K, lambda theta, maxiter)

with the oracle's prox (cold start, its tol / tau), TVnorm and blur model.  Every sample is kept with gx(ii) = TVnorm(X(ii)) and
logpi(ii) = -||y - A X(ii)||^2 / (2 sigma2) - theta gx(ii), ii = 1..samples, and every prox call leaves its iteration count k
(and its final err).  Nothing here imports the library."""
import numpy as np

import sbtv_oracle as o
import wavelet_skrock_restatement as wkr

coefficients = wkr.coefficients
max_step = wkr.max_step
TOL = 1e-3                        # chambolle_prox_TV_stop.m:77


def skrock_tv_chain(y, model, p, op, theta, sigma2, noise, x0=None, alt_tols=(), perturb=None):
    """y (M, N); model, p: the oracle's BlurModel and its PSF parameters; op: dict(samples, stages, lambda, delta,
    eta (0.05), chambolleit); noise (samples-1, M, N); x0: X(1) (None: y).
    alt_tols: further stop tolerances at which every prox call is run again on the same input, for its k alone.
    perturb: None, or f(prox_output, call_number) -> the prox output the chain goes on with.
    Returns dict(samples (S, M, N), gx (S,), logpi (S,), k [calls], err [calls], k_alt [calls][len(alt_tols)])."""
    y = np.asarray(y, dtype=np.float64)
    lam, delta, S, K = op["lambda"], op["delta"], int(op["samples"]), int(op["chambolleit"])
    c = coefficients(op["stages"], op.get("eta", 0.05))
    ks, errs, k_alt = [], [], []

    def prox(v):
        f, _, _, k, err = o.chambolle_prox_TV_stop(v, lam=lam * theta, maxiter=K, tol=TOL, return_info=True)
        k_alt.append([o.chambolle_prox_TV_stop(v, lam=lam * theta, maxiter=K, tol=t, return_info=True)[3] for t in alt_tols])
        ks.append(k)
        errs.append(err)
        return f if perturb is None else perturb(f, len(ks) - 1)

    def drift(v):
        g = np.real(model.AT(model.A(v, *p) - y, *p))
        return (prox(v) - v) / lam - g / sigma2

    X = y.copy() if x0 is None else np.array(x0, dtype=np.float64)
    Xs, gx, logpi = [], np.zeros(S), np.zeros(S)
    for ii in range(1, S + 1):
        if ii > 1:
            X = wkr.step(X, np.asarray(noise[ii - 2], dtype=np.float64), drift, c, delta)
        Xs.append(X)
        gx[ii - 1] = o.TVnorm(X)
        r = y - np.real(model.A(X, *p))
        logpi[ii - 1] = -float(np.sum(r * r)) / (2 * sigma2) - theta * gx[ii - 1]
    return dict(samples=np.stack(Xs), gx=gx, logpi=logpi, k=np.array(ks), err=np.array(errs), k_alt=np.array(k_alt))
