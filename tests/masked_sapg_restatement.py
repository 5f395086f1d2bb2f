"""NumPy restatement of the masked-observation MYULA chain and SAPG estimation on the TV model (include/sbtv.h,
sbtv_myula_masked and sbtv_SAPG_masked), written from the header's statement on the oracle's BlurModel (A, AT, dA),
chambolle_prox_TV_stop and TVnorm.  With m = mask and n_obs = the number of pixels with m > 0:

    R         = sum( m .* (B_p x - y).^2 )
    gradF(x)  = B_p' ( m .* (B_p x - y) ) / s2
    G_theta   = dimX / theta - TVnorm(X)
    G_p(q)    = sum( (dB/dp_q X) .* m .* (B_p X - y) ) / s2
    G_sigma   = R / (2 s2^2) - n_obs / (2 s2)
    logPi     = -R / (2 s2) - theta * TVnorm(X)

and everything else is the loop of the oracle's SAPG_algorithm / myula line for line: the MYULA move (abs() in SAPG, none in
myula), the prox the SAPG move uses (formed at the end of the previous iteration), the order of the updates, the projections,
delta(ii), the burn-in means and the index quirks of the traces.  Every sum is spatial.  Every prox call leaves its iteration
count k and its final err.  Nothing here imports the library."""
import math

import numpy as np

import sbtv_oracle as o

TOL = 1e-3                        # chambolle_prox_TV_stop.m:77


def n_obs(mask):
    return int(np.count_nonzero(np.asarray(mask) > 0))


def residual(model, x, p, y, mask):
    """(r, R): r = m .* (B_p x - y), R = sum(m .* (B_p x - y).^2)."""
    d = model.A(x, *p) - y
    r = mask * d
    return r, float(np.sum(r * d))


def neg_log_likelihood(model, x, p, s2, y, mask):
    """-log p(y | x, p, s2) up to a constant: n_obs/2 log s2 + R / (2 s2)."""
    return 0.5 * n_obs(mask) * math.log(s2) + residual(model, x, p, y, mask)[1] / (2 * s2)


def gradF(model, x, p, s2, y, mask):
    return np.real(model.AT(residual(model, x, p, y, mask)[0], *p)) / s2


def G_p(model, q, x, p, s2, y, mask):
    return float(np.sum(model.dA(q, x, *p) * residual(model, x, p, y, mask)[0]) / s2)


def G_sigma(model, x, p, s2, y, mask):
    return residual(model, x, p, y, mask)[1] / (2 * s2 ** 2) - n_obs(mask) / (2 * s2)


def myula_masked_chain(y, mask, model, p, lam, gam, theta, s2, samples, noise, chambolleit=25, alt_tols=(), perturb=None):
    """SALSA/myula.m:1-22 on the masked likelihood: x = y as given, then ii = 2..samples-1.  noise: (samples-2, M, N).
    alt_tols, perturb: as sapg_masked_chain takes them.
    Returns dict(x: the last sample, samples: X(1..samples-1), k, err [calls], k_alt [calls][len(alt_tols)])."""
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    x = y.copy()
    xs, ks, errs, k_alt = [x], [], [], []
    nz = iter(np.asarray(noise, dtype=np.float64))
    for ii in range(2, int(samples)):
        z = next(nz)
        prox, _, _, k, err = o.chambolle_prox_TV_stop(x, lam=lam * theta, maxiter=chambolleit, tol=TOL, return_info=True)
        k_alt.append([o.chambolle_prox_TV_stop(x, lam=lam * theta, maxiter=chambolleit, tol=t, return_info=True)[3]
                      for t in alt_tols])
        ks.append(k)
        errs.append(err)
        if perturb is not None:
            prox = perturb(prox, len(ks) - 1)
        x = (1 - gam / lam) * x - gam * (gradF(model, x, p, s2, y, m) - prox / lam) + math.sqrt(2 * gam) * z
        xs.append(x)
    return dict(x=x, samples=np.stack(xs), k=np.array(ks), err=np.array(errs), k_alt=np.array(k_alt))


def sapg_masked_chain(setup, mask, samples, warmup, burnIn, noise, chambolleit=25, model=None, p_init=None, fix=None,
                      fix_sigma=False, c=None, x0=None, sigma_init=None, iter_offset=0, y=None, alt_tols=(), perturb=None):
    """setup: the oracle's demo_setup; y: the observation unless setup's; model: its BlurModel unless given (another psf_size);
    noise: (max(warmup-1, 0) + samples-1, M, N), warm-up first; p_init, fix, fix_sigma, c = dict(theta, p, sigma), x0,
    sigma_init, iter_offset: as the oracle's SAPG_algorithm takes them.
    alt_tols: further stop tolerances at which every prox call is run again on the same input, for its k alone.
    perturb: None, or f(prox_output, call_number) -> the prox output the chain goes on with.
    Returns dict(thetas, sigmas (S,), ps (npar, S), logpi (S,), logpi_wu (max(warmup, 1),), gx (S,), grads (npar + 2, S),
    theta_EB, p_EB, sigma_EB, samples (S, M, N): X(1..S), k, err [calls], k_alt [calls][len(alt_tols)])."""
    kind = setup["kind"]
    d = o.DEMO[kind]
    model = setup["model"] if model is None else model
    y = np.asarray(setup["y"] if y is None else y, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    dimX, lamb, gam = setup["dimX"], setup["lam"], setup["gamma"]
    nobs = n_obs(m)
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
    ks, errs, k_alt = [], [], []
    nz = iter(np.asarray(noise, dtype=np.float64))

    def proxG(v, theta):
        f, _, _, k, err = o.chambolle_prox_TV_stop(v, lam=lamb * theta, maxiter=K, tol=TOL, return_info=True)
        k_alt.append([o.chambolle_prox_TV_stop(v, lam=lamb * theta, maxiter=K, tol=t, return_info=True)[3] for t in alt_tols])
        ks.append(k)
        errs.append(err)
        return f if perturb is None else perturb(f, len(ks) - 1)

    def move(X, prox, p, s2):
        r, _ = residual(model, X, p, y, m)
        g = np.real(model.AT(r, *p)) / s2
        return np.abs(X + gam * (prox - X) / lamb - gam * g + math.sqrt(2 * gam) * next(nz))

    def logPi(X, theta, p, s2):
        return -residual(model, X, p, y, m)[1] / (2 * s2) - theta * o.TVnorm(X)

    delta = lambda i: setup["d_scale"] * (((i + iter_offset) ** (-setup["d_exp"])) / dimX)
    th0 = setup["th_init"]

    # ---- warm-up (SAPG_algorithm_Guassian.m:66-93)
    X = y.copy() if x0 is None else np.array(x0, dtype=np.float64)
    logpi_wu = np.zeros(max(warmup, 1))
    if warmup > 0:
        prox = proxG(X, th0)
        for ii in range(2, warmup + 1):
            X = move(X, prox, p_init, sigma_init)
            prox = proxG(X, th0)
            logpi_wu[ii - 1] = logPi(X, th0, p_init, sigma_init)

    # ---- SAPG loop (:98-248)
    thetas = np.zeros(S); thetas[0] = th0
    sigmas = np.zeros(S); sigmas[0] = sigma_init
    ps = np.zeros((npar, S)); ps[:, 0] = p_init
    logpi, gx, grads = np.zeros(S), np.zeros(S), np.zeros((npar + 2, S))
    logpi[0] = logPi(X, th0, p_init, sigma_init)
    prox = proxG(X, th0)
    Xs = [X]
    for ii in range(2, S + 1):
        i0 = ii - 1
        th, pm, s2 = thetas[i0 - 1], tuple(ps[:, i0 - 1]), sigmas[i0 - 1]
        X = move(X, prox, pm, s2)
        Xs.append(X)
        prox = proxG(X, th)
        r, R = residual(model, X, pm, y, m)
        g = o.TVnorm(X)
        G_t = dimX / th - g
        thetas[i0] = min(max(th + c_theta * delta(ii) * G_t, setup["min_th"]), setup["max_th"])
        for q in range(npar):
            G = float(np.sum(model.dA(q, X, *pm) * r) / s2)
            grads[1 + q, i0] = G
            pq = p_true[q] if fixp[q] else ps[q, i0 - 1] - c_p[q] * delta(ii) * G
            ps[q, i0] = min(max(pq, d["pmin"][q]), d["pmax"][q])
        G_s = R / (2 * s2 ** 2) - nobs / (2 * s2)
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
