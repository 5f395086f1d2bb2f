"""NumPy restatement of the SAPG estimation with SK-ROCK as its Markov kernel (include/sbtv.h, sbtv_SAPG_skrock): the loop of the
oracle's SAPG_algorithm with its MYULA move replaced by the step of tests/wavelet_skrock_restatement.py (the header states ONE
step for every SK-ROCK sampler) on the drift

    D(K) = (prox(K) - K) / lambda - AT_p(A_p K - y) / sigma2,    prox(K) = chambolle_prox_TV_stop(K, lambda theta, maxiter)

at the iteration's theta(ii-1), p(ii-1), sigma2(ii-1), with the oracle's prox (cold start, its tol / tau), TVnorm, BlurModel
(A, AT, dA) and demo constants.  No abs() reflection and no lagging prox.  Every prox call leaves its iteration count k and its
final err.  Nothing here imports the library."""
import numpy as np

import sbtv_oracle as o
import wavelet_skrock_restatement as wkr

coefficients = wkr.coefficients
max_step = wkr.max_step
TOL = 1e-3                        # chambolle_prox_TV_stop.m:77


def sapg_skrock_chain(setup, samples, warmup, burnIn, stages, dt, noise, eta=0.05, chambolleit=25, model=None, p_init=None,
                      fix=None, fix_sigma=False, c=None, x0=None, sigma_init=None, iter_offset=0, alt_tols=(), perturb=None):
    """setup: the oracle's demo_setup; model: its BlurModel unless given (another psf_size); noise: (max(warmup-1, 0) +
    samples-1, M, N), warm-up first; p_init, fix, fix_sigma, c = dict(theta, p, sigma), x0, sigma_init, iter_offset: as the
    oracle's SAPG_algorithm takes them.
    alt_tols: further stop tolerances at which every prox call is run again on the same input, for its k alone.
    perturb: None, or f(prox_output, call_number) -> the prox output the chain goes on with.
    Returns dict(thetas, sigmas (S,), ps (npar, S), logpi (S,), logpi_wu (max(warmup, 1),), gx (S,), grads (npar + 2, S),
    theta_EB, p_EB, sigma_EB, samples (S, M, N): X(1..S), k, err [calls], k_alt [calls][len(alt_tols)])."""
    kind = setup["kind"]
    d = o.DEMO[kind]
    model = setup["model"] if model is None else model
    y, dimX, lam = setup["y"], setup["dimX"], setup["lam"]
    npar = len(d["true"])
    p_init = tuple(d["init"] if p_init is None else p_init)
    fixp = tuple(d["fix"] if fix is None else fix)
    c_theta = d["c_theta"] if c is None else c["theta"]
    c_p = d["c_p"] if c is None else c["p"]
    c_sigma = d["c_sigma"] if c is None else c["sigma"]
    p_true = setup["p_true"]
    s_lo, s_hi = min(setup["sigma_min"], setup["sigma_max"]), max(setup["sigma_min"], setup["sigma_max"])
    if sigma_init is None:
        sigma_init = setup["sigma"] ** 2 if fix_sigma else setup["sigma_init"]
    S, K = int(samples), int(chambolleit)
    cf = coefficients(stages, eta)
    ks, errs, k_alt = [], [], []
    nz = iter(np.asarray(noise, dtype=np.float64))

    def prox(v, theta):
        f, _, _, k, err = o.chambolle_prox_TV_stop(v, lam=lam * theta, maxiter=K, tol=TOL, return_info=True)
        k_alt.append([o.chambolle_prox_TV_stop(v, lam=lam * theta, maxiter=K, tol=t, return_info=True)[3] for t in alt_tols])
        ks.append(k)
        errs.append(err)
        return f if perturb is None else perturb(f, len(ks) - 1)

    def skrock_step(X, theta, p, s2):
        def drift(v):
            g = np.real(model.AT(model.A(v, *p) - y, *p))
            return (prox(v, theta) - v) / lam - g / s2
        return wkr.step(X, next(nz), drift, cf, dt)

    def sums(X, p):
        r = model.A(X, *p) - y
        return r, float(np.sum(r * r)), o.TVnorm(X)

    delta = lambda i: setup["d_scale"] * (((i + iter_offset) ** (-setup["d_exp"])) / dimX)
    th0 = setup["th_init"]
    X = y.copy() if x0 is None else np.array(x0, dtype=np.float64)
    logpi_wu = np.zeros(max(warmup, 1))
    for ii in range(2, warmup + 1):
        X = skrock_step(X, th0, p_init, sigma_init)
        _, R, g = sums(X, p_init)
        logpi_wu[ii - 1] = -R / (2 * sigma_init) - th0 * g

    thetas = np.zeros(S); thetas[0] = th0
    sigmas = np.zeros(S); sigmas[0] = sigma_init
    ps = np.zeros((npar, S)); ps[:, 0] = p_init
    logpi, gx, grads = np.zeros(S), np.zeros(S), np.zeros((npar + 2, S))
    _, R, g = sums(X, p_init)
    logpi[0] = -R / (2 * sigma_init) - th0 * g
    Xs = [X]
    for ii in range(2, S + 1):
        i0 = ii - 1
        th, pm, s2 = thetas[i0 - 1], tuple(ps[:, i0 - 1]), sigmas[i0 - 1]
        X = skrock_step(X, th, pm, s2)
        Xs.append(X)
        r, R, g = sums(X, pm)
        G_t = dimX / th - g
        thetas[i0] = min(max(th + c_theta * delta(ii) * G_t, setup["min_th"]), setup["max_th"])
        for q in range(npar):
            G = float(np.sum(model.dA(q, X, *pm) * r) / s2)
            grads[1 + q, i0] = G
            pq = p_true[q] if fixp[q] else ps[q, i0 - 1] - c_p[q] * delta(ii) * G
            ps[q, i0] = min(max(pq, d["pmin"][q]), d["pmax"][q])
        G_s = R / (2 * s2 ** 2) - dimX / (2 * s2)
        s_new = sigma_init if fix_sigma else s2 + c_sigma * delta(ii) * G_s
        sigmas[i0] = min(max(s_new, s_lo), s_hi)
        grads[0, i0] = G_t
        grads[npar + 1, i0] = G_s
        logpi[i0] = -R / (2 * s2) - th * g
        gx[i0 - 1] = g
    b0 = int(burnIn) - 1
    return dict(thetas=thetas, sigmas=sigmas, ps=ps, logpi=logpi, logpi_wu=logpi_wu, gx=gx, grads=grads,
                theta_EB=float(np.mean(thetas[b0:])), p_EB=[float(np.mean(ps[q, b0:])) for q in range(npar)],
                sigma_EB=float(np.mean(sigmas[b0:])), samples=np.stack(Xs), k=np.array(ks), err=np.array(errs),
                k_alt=np.array(k_alt))
