"""NumPy restatements of C-SALSA with the wavelet analysis prior (include/sbtv.h, sbtv_CSALSA_wavelet):

    min over the IMAGE x   ||W' x||_1    s.t.   ||B x - y||_2 <= epsilon

`csalsa_wavelet_literal` is SALSA/CSALSA_v2.m:401-561 line for line with general handles A, AT, invLS, P, PT, psi and phi.  The
library's configuration is `wavelet_handles`: A = B, AT = B', invLS(r, mu) = real(ifft2(fft2(r) ./ (|H|^2 + mu))), P = W
(mirdwt_TI2D), PT = W' (mrdwt_TI2D), psi = soft and phi = ||W' .||_1.  The reference records objective = phi(x) with x the image
(:423, 498); phi is a parameter here and the library's cases run with phi = ||W' .||_1, the one stated deviation of the entry
point; the reference's probe phi(PT(ATy)) (:357), which would hand such a phi coefficients, is skipped.  With identity P / PT,
the TV prox as psi (`TVProx`) and phi = TVnorm it is sbtv_oracle.CSALSA_v2 bit for bit (tests/test_csalsa_wavelet_cpu.py).
`csalsa_wavelet_state` is the form the library runs: the coefficient state (s, bu), s = u + bu, and the constraint split either
as the spectrum E of ve with the scalar s_ = min(1, epsilon / ||ve||) (form "spectral") or as the images v, bv (form "image").
The frame and soft are those of tests/wavelet_restatement.py.  Nothing here imports the library."""
import math
import time

import numpy as np

from wavelet_restatement import mirdwt_TI2D, mrdwt_TI2D, soft


def _norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


class TVProx:
    """psi of the TV configuration (:476): chambolle_prox_TV_stop with its warm-started duals as state."""

    def __init__(self, shape, TViters):
        import sbtv_oracle as o
        self._prox = o.chambolle_prox_TV_stop
        self.pux, self.puy, self.TViters = np.zeros(shape), np.zeros(shape), TViters      # :440-441

    def __call__(self, g, lam):
        u, self.pux, self.puy = self._prox(np.real(g), lam=lam, maxiter=self.TViters, dualvars=np.hstack([self.pux, self.puy]))
        return u


def wavelet_handles(H, h, levels):
    """dict(A, AT, invLS, P, PT, psi, phi) of the library's configuration; H: fft2 of the PSF."""
    PT = lambda v: mrdwt_TI2D(v, h, levels)
    return dict(A=lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v))),
                AT=lambda v: np.real(np.fft.ifft2(np.conj(H) * np.fft.fft2(v))),
                invLS=lambda r, mu: np.real(np.fft.ifft2(np.fft.fft2(r) / (np.abs(H) ** 2 + mu))),
                P=lambda c: mirdwt_TI2D(c, h, levels), PT=PT, psi=soft, phi=lambda x: float(np.sum(np.abs(PT(x)))))


def csalsa_wavelet_literal(y, A, AT, invLS, P, PT, psi, phi, mu1, mu2, sigma, true_x=None, stopcriterion=3, tolA=0.001,
                           maxiter=10000, initialization=0, continuationfactor=1.0, epsilon=0.0):
    """Returns x, u, the counters, the traces (entry 0: the state before the loop), n_outer, epsilon, and for the margins of
    the cases `stopvalue` (the number the rule compares with tolA, entry outer - 2) and `n_ve` (||ve|| of every iteration)."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")                   # :258
    y = np.asarray(y, dtype=np.float64)
    numA = numAt = 0
    ATy = AT(y)                                                          # :301
    numAt += 1
    dummy = invLS(ATy, mu1)                                              # :310
    assert dummy.shape == ATy.shape
    if isinstance(initialization, np.ndarray):
        x = np.array(initialization, dtype=np.float64)
    elif initialization == 0:
        x = AT(np.zeros_like(y))                                         # :380
    elif initialization == 2:
        x = ATy.copy()                                                   # :384
        numAt += 1
    else:
        raise ValueError("Unknown 'Initialization' option")
    PTx = PT(x)                                                          # :402
    u = 0 * PTx                                                          # :404
    bu = 0 * u                                                           # :405
    v = 0 * y                                                            # :407
    bv = 0 * y                                                           # :408
    if not epsilon:
        epsilon = math.sqrt(y.size + 8 * math.sqrt(y.size)) * sigma      # :413
    Ax = A(x)                                                            # :416
    numA += 1                                                            # :421
    objective = [phi(x)]                                                 # :423
    times = [0.0]                                                        # :433
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []   # :436
    t0 = time.perf_counter()
    Ax = A(x)                                                            # :444
    numA += 1
    criterion = [_norm(Ax - y)]                                          # :446
    distance1 = [_norm(Ax - y - v)]                                      # :447
    distance2 = [_norm(PTx - u)]                                         # :448
    delta = continuationfactor
    stopvalue, n_ves = [], []
    n_outer = 1
    for outer in range(2, int(maxiter) + 1):                             # :461
        n_outer = outer
        mu1inv = 1 / mu1                                                 # :463
        xprev = x                                                        # :465
        r = mu1 * P(u + bu) + mu2 * AT(y + v + bv)                       # :467
        numAt += 1
        x = invLS(r, mu1)                                                # :471
        PTx = PT(x)                                                      # :473
        u = psi(PTx - bu, mu1inv)                                        # :476 / :478
        Ax = A(x)                                                        # :481
        numA += 1
        ve = Ax - y - bv                                                 # :483
        n_ve = _norm(ve)                                                 # :484
        v = ve if n_ve <= epsilon else ve / n_ve * epsilon               # :485-489
        bv = bv - (Ax - y - v)                                           # :491
        bu = bu - (PTx - u)                                              # :492
        criterion.append(_norm(Ax - y))                                  # :494
        distance1.append(_norm(Ax - y - v))                              # :495
        distance2.append(_norm(PTx - u))                                 # :497
        objective.append(phi(x))                                         # :498
        if true_x is not None:
            mses.append(_norm(x - true_x) ** 2 / true_x.size)            # :501
        times.append(time.perf_counter() - t0)                           # :504
        n_ves.append(n_ve)
        mu1 = mu1 * delta                                                # :517-518
        mu2 = mu2 * delta
        k = outer - 1                                                    # 0-based position of `outer`
        if stopcriterion == 1:
            sc = abs(objective[k] - objective[k - 1]) / objective[k]     # :527
        elif stopcriterion == 2:
            sc = abs(_norm(x - xprev) / _norm(x))                        # :534
        else:
            sc = abs(criterion[k] - criterion[k - 1]) / criterion[k]     # :539
        stopvalue.append(sc)
        if sc < tolA and criterion[k] <= epsilon:                        # :529,535,541
            break
    return dict(x=x, u=u, numA=numA, numAt=numAt, objective=np.array(objective), distance1=np.array(distance1),
                distance2=np.array(distance2), criterion=np.array(criterion), times=np.array(times), mses=np.array(mses),
                n_outer=n_outer, epsilon=epsilon, stopvalue=np.array(stopvalue), n_ve=np.array(n_ves), v=v)


def csalsa_wavelet_state(y, H, h, levels, mu1, mu2, sigma, true_x=None, stopcriterion=3, tolA=0.001, maxiter=10000,
                         initialization=0, continuationfactor=1.0, epsilon=0.0, form="spectral"):
    """The same iteration as the library runs it.  The coefficient pass is one and the same in both forms:
        u = soft(w - bu, 1/mu1) ; bu' = bu - (w - u) ; s' = u + bu' ; the sums |w| and (w - u)^2
    form "spectral": the split (v, bv) is the spectrum E of ve and the scalar s_ of the previous iteration; one spectral pass
    forms W = mu2 (Y + (2 s_ - 1) E), X = (conj(H) W + mu1 fft2(W s)) / (|H|^2 + mu1), T = H X - Y, E' = T + (1 - s_) E and the
    Parseval sums ||Ax-y||^2, ||ve||^2, ||E' - E||^2 (needs a fixed mu1 / mu2).  form "image": v and bv are images."""
    y = np.asarray(y, dtype=np.float64)
    if form == "spectral" and continuationfactor != 1.0:
        raise ValueError("the spectral form needs fixed mu1 / mu2")
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    Y = np.fft.fft2(y)
    Hc, H2 = np.conj(H), np.abs(H) ** 2
    n = y.size
    B = lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v)))
    BT = lambda v: np.real(np.fft.ifft2(Hc * np.fft.fft2(v)))
    numA, numAt = 2, 1
    if isinstance(initialization, np.ndarray):
        x = np.array(initialization, dtype=np.float64)
    elif initialization == 0:
        x = np.zeros_like(y)
    elif initialization == 2:
        x = BT(y)
        numAt += 1
    else:
        raise ValueError("Unknown 'Initialization' option")
    if not epsilon:
        epsilon = math.sqrt(n + 8 * math.sqrt(n)) * sigma
    w = WT(x)
    s = np.zeros_like(w)
    bu = np.zeros_like(w)
    r0 = math.sqrt(float(np.sum(np.abs(H * np.fft.fft2(x) - Y) ** 2)) / n)
    criterion, distance1, distance2 = [r0], [r0], [math.sqrt(float(np.sum((w - s) ** 2)))]
    objective = [float(np.sum(np.abs(w)))]
    times = [0.0]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []
    E, sm, A1p = np.zeros_like(Y), 1.0, 0.0                              # v = bv = 0: E = 0, s_ = 1
    v, bv = np.zeros_like(y), np.zeros_like(y)
    delta = continuationfactor
    t0 = time.perf_counter()
    n_outer = 1
    for outer in range(2, int(maxiter) + 1):
        n_outer = outer
        T = 1.0 / mu1
        xprev = x
        z = W(s)
        if form == "spectral":
            Wsp = mu2 * (Y + (2.0 * sm - 1.0) * E)
            X = (Hc * Wsp + mu1 * np.fft.fft2(z)) / (H2 + mu1)
            Tt = H * X - Y
            En = Tt + (1.0 - sm) * E
            A0, A1, A2 = (float(np.sum(np.abs(q) ** 2)) / n for q in (Tt, En, En - E))
            x = np.real(np.fft.ifft2(X))
            n_ve = math.sqrt(A1)
            sfac = 1.0 if n_ve <= epsilon else epsilon / n_ve
            a, c = 1.0 - sfac, 1.0 - sm
            d1 = (a - c) * (a * A1 - c * A1p) + a * c * A2
            crit, dist1 = math.sqrt(A0), math.sqrt(max(d1, 0.0))
            E, sm, A1p = En, sfac, A1
        else:
            Wsp = np.fft.fft2(mu2 * ((y + v) + bv))
            X = (Hc * Wsp + mu1 * np.fft.fft2(z)) / (H2 + mu1)
            x = np.real(np.fft.ifft2(X))
        w = WT(x)
        u = soft(w - bu, T)                                              # the coefficient pass
        d = w - u
        bu = bu - d
        s = u + bu
        if form != "spectral":
            Ax = B(x)
            t = Ax - y
            ve = t - bv
            n_ve = _norm(ve)
            v = ve if n_ve <= epsilon else ve / n_ve * epsilon
            rr = t - v
            bv = bv - rr
            crit, dist1 = _norm(t), _norm(rr)
        numAt += 1
        numA += 1
        criterion.append(crit)
        distance1.append(dist1)
        distance2.append(math.sqrt(float(np.sum(d * d))))
        objective.append(float(np.sum(np.abs(w))))
        if true_x is not None:
            mses.append(float(np.sum((x - true_x) ** 2)) / x.size)
        times.append(time.perf_counter() - t0)
        mu1 = mu1 * delta
        mu2 = mu2 * delta
        k = outer - 1
        if stopcriterion == 1:
            sc = abs(objective[k] - objective[k - 1]) / objective[k]
        elif stopcriterion == 2:
            sc = abs(math.sqrt(float(np.sum((x - xprev) ** 2))) / math.sqrt(float(np.sum(x * x))))
        else:
            sc = abs(criterion[k] - criterion[k - 1]) / criterion[k]
        if sc < tolA and criterion[k] <= epsilon:
            break
    return dict(x=x, numA=numA, numAt=numAt, objective=np.array(objective), distance1=np.array(distance1),
                distance2=np.array(distance2), criterion=np.array(criterion), times=np.array(times), mses=np.array(mses),
                n_outer=n_outer, epsilon=epsilon)
