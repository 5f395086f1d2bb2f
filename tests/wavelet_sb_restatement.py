"""NumPy restatement of the semi-blind empirical-Bayes loop of the wavelet-l1 prior (include/sbtv.h,
sbtv_SAPG_wavelet_semiblind), built on tests/wavelet_restatement.py (the frame, soft) and sbtv_oracle.BlurModel (A, AT, dA of
the three PSF families).

`literal` is SALSA/SAPG_algorithm_1.m:120-242 line for line with BOTH of its parameters: theta on the log scale, and `tau` =
the PSF parameters p with the closures the script run_deblur_synthesis_L1.m never defines: gradF(X, p) = W'B_p'(B_p W X - y)
/ sigma2 and op.grad_t = <dB/dp W X, B_p W X - y> / sigma2, scaled by c_p as SAPG/SAPG_algorithm_laplace.m:172-178, plus the
sigma2 step of SAPG_algorithm_laplace.m:181-186 (its dimension is the PIXEL count).  One deliberate deviation, stated in the
header: logpi(ii) uses p(ii-1), not the unclamped new `to` of :190.  `fused` is the form the library runs: no stored prox, W X
synthesised once per sample and shared by the residual of that sample and the gradient of the next step.  Both keep the
running sums over burnIn..ii in iteration order.  Nothing here imports the library."""
import math

import numpy as np

import wavelet_restatement as wr
from sbtv_oracle import resize

NPAR = {"gaussian": 2, "moffat": 2, "laplace": 1}


def _mean(s, n):
    return s / n if n > 0 else float("nan")


def _exp_mean(s, n):
    return math.exp(s / n) if n > 0 else float("nan")


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


def blur(model, v, p):
    """B_p v, BlurModel.A with the transforms of tests/wavelet_sapg_restatement.py (numpy.fft), so that a chain at fixed
    parameters is that file's chain bit for bit."""
    return np.real(np.fft.ifft2(model.H_FFT(*p) * np.fft.fft2(v)))


def blur_T(model, v, p):
    """B_p' v (BlurModel.AT)."""
    return np.real(np.fft.ifft2(np.conj(model.H_FFT(*p)) * np.fft.fft2(v)))


def blur_d(model, q, v, p):
    """(dB/dp_q)(p) v (BlurModel.dA): the circular convolution with the derivative taps.  Moffat alpha: the reference's
    utils/diff_moffat_alpha.m (BlurModel.dtaps) carries alpha / (2 pi) where the derivative of alpha^2 / (2 pi) gives
    alpha / pi, i.e. it is half the derivative of psf_moffat in every tap; the factor is restored here."""
    d = np.real(np.fft.ifft2(resize(model.dtaps(q, *p), model.im_shape) * np.fft.fft2(v)))
    return 2.0 * d if (model.kind == "moffat" and q == 0) else d


def grad_p(model, y, WX, p, q, sigma2):
    """op.grad_t of parameter q at the image WX = W X: <dB/dp_q WX, B_p WX - y> / sigma2."""
    return float(np.sum(blur_d(model, q, WX, p) * (blur(model, WX, p) - y))) / sigma2


def _traces(op, npar):
    S, burnIn = int(op["samples"]), int(op["burnIn"])
    t = dict(thetas=np.zeros(S), sigmas=np.zeros(S), ps=np.zeros((2, S)), grads=np.zeros((3, S)), logPiTraceX=np.zeros(S),
             gXTrace=np.zeros(S), tol_thetas=np.zeros(S), tol_ps=np.zeros((2, S)), mean_thetas=np.zeros(max(S - burnIn, 0)),
             mean_ps=np.zeros((2, max(S - burnIn, 0))))
    t["thetas"][0], t["sigmas"][0] = op["th_init"], op["sigma2"]
    t["ps"][:npar, 0] = op["p_init"][:npar]
    return t


class _Sums:
    """Running sums of eta, p and sigma2 over burnIn..ii and what :199-213,226,236 make of them."""

    def __init__(self, op, npar, eta0):
        self.npar, self.burnIn = npar, int(op["burnIn"])
        self.n = 1 if self.burnIn == 1 else 0
        self.eta = eta0 if self.n else 0.0
        self.p = [op["p_init"][q] if self.n and q < npar else 0.0 for q in range(2)]
        self.s = op["sigma2"] if self.n else 0.0

    def book(self, t, ii, eta, p, s):
        m0, a0 = _exp_mean(self.eta, self.n), [_mean(self.p[q], self.n) for q in range(self.npar)]
        if ii >= self.burnIn:
            self.eta, self.s, self.n = self.eta + eta, self.s + s, self.n + 1
            for q in range(self.npar):
                self.p[q] += p[q]
        m1, a1 = _exp_mean(self.eta, self.n), [_mean(self.p[q], self.n) for q in range(self.npar)]
        with np.errstate(divide="ignore", invalid="ignore"):
            t["tol_thetas"][ii - 1] = np.float64(abs(m1 - m0)) / np.float64(m0)                     # :199-200
            for q in range(self.npar):
                t["tol_ps"][q, ii - 1] = np.float64(abs(a1[q] - a0[q])) / np.float64(a0[q])         # :204-205
        if ii > self.burnIn:
            t["mean_thetas"][ii - self.burnIn - 1] = m1                                             # :209-211
            for q in range(self.npar):
                t["mean_ps"][q, ii - self.burnIn - 1] = a1[q]                                       # :213

    def results(self, t, op, X, logpi_wu):
        theta_EB = math.exp(self.eta / self.n)                                                      # :226
        p_EB = np.array([self.p[q] / self.n for q in range(self.npar)])                             # :236
        res = dict(t, last_samp=int(op["samples"]), mean_theta=theta_EB, last_theta=t["thetas"][-1], p_EB=p_EB,
                   sigma2_EB=self.s / self.n, options=op, Xlast_sample=X)
        if op["warmup"] > 0:
            res["logPiTrace_WU"] = logpi_wu
        return dict(theta=theta_EB, p=p_EB, sigma2=self.s / self.n), res


def _param_step(op, npar, delta, pm, s, Gp, R, P):
    """:185-186 scaled as SAPG_algorithm_laplace.m:172-178, and the sigma2 step of SAPG_algorithm_laplace.m:181-186."""
    pn = []
    for q in range(npar):
        to = op["p_true"][q] if op["fix_p"][q] else pm[q] - op["c_p"][q] * delta * Gp[q]
        pn.append(_clamp(to, op["p_min"][q], op["p_max"][q]))
    Gs = R / (2 * s * s) - P / (2 * s)
    sn = op["sigma2"] if op["fix_sigma"] else s + op["c_sigma"] * delta * Gs
    return tuple(pn), _clamp(sn, op["sigma2_min"], op["sigma2_max"]), Gs


def literal(y, model, h, levels, op, noise, xw0=None):
    """op: the keys of wavelet_sapg_restatement plus p_init, p_min, p_max, p_true, fix_p, c_p (one entry per PSF parameter),
    fix_sigma, sigma2_min, sigma2_max, c_sigma; sigma2 is sigma2(1).  model: sbtv_oracle.BlurModel.  noise: (max(warmup-1, 0) +
    samples-1, M, (3J+1) N), warm-up first.  Returns (eb, results) in the shape of sbtv.SAPG_wavelet_semiblind."""
    y = np.asarray(y, dtype=np.float64)
    npar = NPAR[model.kind]
    W = lambda c: wr.mirdwt_TI2D(c, h, levels)
    WT = lambda v: wr.mrdwt_TI2D(v, h, levels)
    A = lambda c, p: blur(model, W(c), p)
    AT = lambda v, p: WT(blur_T(model, v, p))
    lam, gamma = op["lambda"], op["gamma"]
    g = lambda c: float(np.sum(np.abs(c)))
    proxG = lambda c, la, th: wr.soft(c, th * la)
    f = lambda c, p, s: wr._sq(y - A(c, p)) / (2 * s)
    gradF = lambda c, p, s: AT(A(c, p) - y, p) / s                                     # the two-argument gradF
    gradF_to = lambda c, p, s, q: float(np.sum(blur_d(model, q, W(c), p) * (A(c, p) - y))) / s              # op.grad_t
    logPi = lambda c, th, p, s: -f(c, p, s) - th * g(c)
    X0 = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    dimX, P = X0.size, y.size                                                          # :86; the dimension of y
    total_iter, warmup = int(op["samples"]), int(op["warmup"])
    eta_init, min_eta, max_eta = math.log(op["th_init"]), math.log(op["min_th"]), math.log(op["max_th"])
    delta = lambda i: op["d_scale"] * (i ** (-op["d_exp"]) / dimX)                     # :111
    sq2g = math.sqrt(2 * gamma)
    p_init, s_init = tuple(op["p_init"][:npar]), op["sigma2"]
    step = 0
    X_wu = X0
    logpi_wu = np.zeros(max(warmup, 0))
    if warmup > 0:
        fix_theta, fix_tau = op["th_init"], p_init                                     # :124-125
        prox = proxG(X_wu, lam, fix_theta)
        for ii in range(2, warmup + 1):
            X_wu = ((X_wu + gamma * (prox - X_wu) / lam) - gamma * gradF(X_wu, fix_tau, s_init)) + sq2g * noise[step]   # :133
            step += 1
            prox = proxG(X_wu, lam, fix_theta)
            logpi_wu[ii - 1] = logPi(X_wu, fix_theta, fix_tau, s_init)                 # :136
    t = _traces(op, npar)
    theta, sig, ps = t["thetas"], t["sigmas"], t["ps"]
    eta = np.zeros(total_iter)
    eta[0] = eta_init
    X = X_wu
    t["logPiTraceX"][0] = logPi(X, theta[0], p_init, sig[0])                           # :166
    prox = proxG(X, lam, theta[0])
    sums = _Sums(op, npar, eta_init)
    for ii in range(2, total_iter + 1):
        pm, s = tuple(ps[:npar, ii - 2]), sig[ii - 2]
        Z = noise[step]
        step += 1
        X = ((X + gamma * (prox - X) / lam) - gamma * gradF(X, pm, s)) + sq2g * Z      # :174
        prox = proxG(X, lam, theta[ii - 2])                                            # :175
        gX = g(X)
        etaii = eta[ii - 2] + delta(ii) * (dimX / theta[ii - 2] - gX) * math.exp(eta[ii - 2])      # :180
        eta[ii - 1] = _clamp(etaii, min_eta, max_eta)
        theta[ii - 1] = math.exp(eta[ii - 1])
        R = wr._sq(A(X, pm) - y)
        Gp = [gradF_to(X, pm, s, q) for q in range(npar)]
        pn, sn, Gs = _param_step(op, npar, delta(ii), pm, s, Gp, R, P)                 # :185-186
        ps[:npar, ii - 1], sig[ii - 1] = pn, sn
        t["grads"][:npar, ii - 1], t["grads"][2, ii - 1] = Gp, Gs
        t["logPiTraceX"][ii - 1] = -R / (2 * s) - theta[ii - 2] * gX                   # :190, at p(ii-1)
        t["gXTrace"][ii - 2] = gX                                                      # :191
        sums.book(t, ii, eta[ii - 1], pn, sn)
    return sums.results(t, op, X, logpi_wu)


def fused(y, model, h, levels, op, noise, xw0=None):
    """The same chain as the library runs it: state X only, the soft threshold recomputed from X and the lagging theta; the
    image W X of a sample is synthesised once and gives the residual / parameter gradients of that sample (with p(ii-1)) and
    the gradient of the next step (with p(ii))."""
    y = np.asarray(y, dtype=np.float64)
    npar = NPAR[model.kind]
    W = lambda c: wr.mirdwt_TI2D(c, h, levels)
    WT = lambda v: wr.mrdwt_TI2D(v, h, levels)
    lam, gamma = op["lambda"], op["gamma"]
    X = WT(y) if xw0 is None else np.array(xw0, dtype=np.float64)
    dimX, P = X.size, y.size
    samples, warmup = int(op["samples"]), int(op["warmup"])
    eta, min_eta, max_eta = math.log(op["th_init"]), math.log(op["min_th"]), math.log(op["max_th"])
    sq2g = math.sqrt(2 * gamma)
    th_prev = th_cur = op["th_init"]
    p, s = tuple(op["p_init"][:npar]), op["sigma2"]
    t = _traces(op, npar)
    logpi_wu = np.zeros(max(warmup, 0))
    sums = _Sums(op, npar, eta)

    def step(X, WX, Z):
        G = WT(blur_T(model, blur(model, WX, p) - y, p))
        Xn = ((X + gamma * (wr.soft(X, lam * th_prev) - X) / lam) - gamma * (G / s)) + sq2g * Z
        WXn = W(Xn)
        r = blur(model, WXn, p) - y
        return Xn, WXn, r, wr._sq(r), float(np.sum(np.abs(Xn)))

    WX = W(X)
    t["logPiTraceX"][0] = -wr._sq(blur(model, WX, p) - y) / (2 * s) - th_cur * float(np.sum(np.abs(X)))
    k = 0
    for ii in range(2, warmup + 1):
        X, WX, r, R, g = step(X, WX, noise[k])
        k += 1
        logpi_wu[ii - 1] = t["logPiTraceX"][0] = -R / (2 * s) - th_cur * g
    for ii in range(2, samples + 1):
        X, WX, r, R, g = step(X, WX, noise[k])
        k += 1
        t["logPiTraceX"][ii - 1], t["gXTrace"][ii - 2] = -R / (2 * s) - th_cur * g, g
        delta = op["d_scale"] * (ii ** (-op["d_exp"]) / dimX)
        etaii = eta + delta * (dimX / th_cur - g) * math.exp(eta)
        eta = _clamp(etaii, min_eta, max_eta)
        th = math.exp(eta)
        Gp = [float(np.sum(blur_d(model, q, WX, p) * r)) / s for q in range(npar)]
        pn, sn, Gs = _param_step(op, npar, delta, p, s, Gp, R, P)
        t["thetas"][ii - 1], t["sigmas"][ii - 1], t["ps"][:npar, ii - 1] = th, sn, pn
        t["grads"][:npar, ii - 1], t["grads"][2, ii - 1] = Gp, Gs
        sums.book(t, ii, eta, pn, sn)
        th_prev, th_cur, p, s = th_cur, th, pn, sn
    return sums.results(t, op, X, logpi_wu)
