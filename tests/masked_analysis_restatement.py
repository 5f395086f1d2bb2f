"""NumPy restatement of the masked-observation SALSA with an analysis prior (include/sbtv.h, sbtv_SALSA_masked_analysis):

    min over the IMAGE x   0.5 sum(m .* (B x - y).^2) + tau phi(PT x)

the mask-decoupling ADMM of Almeida & Figueiredo (IEEE TIP 2013) with the splits u = PT x and v = B x, written line for line as
the header states it.  `salsa_masked_literal` takes the handles P, PT, psi, phi: with identity handles, the oracle's
chambolle_prox_TV_stop (warm duals) as psi and TVnorm as phi it IS tests/masked_restatement.py's salsa_masked, bit for bit
(tests/test_masked_analysis_cpu.py asserts it), and with P = W = mirdwt_TI2D, PT = W' = mrdwt_TI2D, psi = soft, phi = l1 it is the
reference of the GPU tests (`salsa_masked_analysis_literal`).  `salsa_masked_analysis_state` is the form the library runs, in
the device's order of operations: the coefficient state (s, bu) with s = u + bu, the pixel state x, Bx, v, bv, the spectral
solve with r = mu1 / mu2.  The reference has no such solver.  Nothing here imports the library."""
import math
import time

import numpy as np

import sbtv_oracle as o

from wavelet_restatement import _sq, mirdwt_TI2D, mrdwt_TI2D, soft


class WarmChambolle:
    """psi(g, lam) = chambolle_prox_TV_stop(g, lam, maxiter = TViters) with the duals of the call before (zero at first)."""

    def __init__(self, shape, TViters):
        self.pux, self.puy, self.K = np.zeros(shape), np.zeros(shape), TViters

    def __call__(self, g, lam):
        u, self.pux, self.puy = o.chambolle_prox_TV_stop(g, lam=lam, maxiter=self.K, dualvars=(self.pux, self.puy))
        return u


def _start(initialization, y, m, Bt):
    """(x, applications of B') of the start."""
    if isinstance(initialization, np.ndarray):
        return np.array(initialization, dtype=np.float64), 0
    if initialization == 0:
        return np.zeros_like(y), 0
    if initialization == 2:
        return Bt(m * y), 1
    raise ValueError("Unknown 'Initialization' option")


def _criterion(stopcriterion, objective, outer, x, xprev):
    """The number the stop rule compares with tolA (SALSA_v2.m:456-466)."""
    if stopcriterion == 1:
        return abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]
    if stopcriterion == 2:
        return abs(float(np.linalg.norm((x - xprev).ravel())) / float(np.linalg.norm(x.ravel())))
    return objective[outer]


def salsa_masked_literal(y, mask, H, tau, mu1, mu2, P, PT, psi, phi, true_x=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                         initialization=0):
    """The iteration of the header with general handles.  H: fft2 of the embedded taps; psi(g, threshold) the prox of
    threshold * phi.  Returns dict(x, u, v, bu, bv, numA, numAt, objective, distance, times, mses, n_outer, criterion);
    `criterion` holds the stop criterion of every iteration from the second on (entry outer - 2)."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    Hc = np.conj(H)
    H2 = np.abs(H) ** 2
    B = lambda z: np.real(o.ifft2(H * o.fft2(z)))
    Bt = lambda z: np.real(o.ifft2(Hc * o.fft2(z)))
    numA = numAt = 0
    x, numAt = _start(initialization, y, m, Bt)
    Bx = B(x)
    numA += 1
    PTx = PT(x)
    u = PTx.copy()
    v = Bx.copy()
    bu = np.zeros_like(u)
    bv = np.zeros_like(x)
    objective = [0.5 * float(np.sum(m * (Bx - y) ** 2)) + tau * phi(u)]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []
    times = [0.0]
    distance, criterion = [], []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = x
        u = psi(PTx - bu, tau / mu1)
        v = (m * y + mu2 * (Bx - bv)) / (m + mu2)
        X = (mu1 * o.fft2(P(u + bu)) + mu2 * Hc * o.fft2(v + bv)) / (mu1 + mu2 * H2)
        numAt += 1
        x = np.real(o.ifft2(X))
        Bx = np.real(o.ifft2(H * X))
        numA += 1
        PTx = PT(x)
        bu = bu + (u - PTx)
        bv = bv + (v - Bx)
        objective.append(0.5 * float(np.sum(m * (Bx - y) ** 2)) + tau * phi(u))
        if true_x is not None:
            e = x - true_x
            mses.append(float(np.sum(e * e)) / x.size)
        distance.append([float(np.linalg.norm((PTx - u).ravel())) / math.sqrt(float(np.sum(PTx * PTx)) + float(np.sum(u * u))),
                         float(np.linalg.norm((Bx - v).ravel())) / math.sqrt(float(np.sum(Bx * Bx)) + float(np.sum(v * v)))])
        times.append(time.perf_counter() - t0)
        if outer > 1:
            crit = _criterion(stopcriterion, objective, outer, x, xprev)
            criterion.append(crit)
            if crit < tolA:
                break
    return dict(x=x, numA=numA, numAt=numAt, objective=np.array(objective), distance=np.array(distance).reshape(-1, 2),
                times=np.array(times), mses=np.array(mses), n_outer=n_outer, u=u, v=v, bu=bu, bv=bv,
                criterion=np.array(criterion))


def salsa_masked_analysis_literal(y, mask, H, h, levels, tau, mu1, mu2, **kw):
    """The literal iteration with the wavelet frame: P = W, PT = W', psi = soft, phi = l1."""
    return salsa_masked_literal(y, mask, H, tau, mu1, mu2, lambda c: mirdwt_TI2D(c, h, levels), lambda z: mrdwt_TI2D(z, h, levels),
                                soft, lambda c: float(np.sum(np.abs(c))), **kw)


def salsa_masked_analysis_state(y, mask, H, h, levels, tau, mu1, mu2, true_x=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                                initialization=0):
    """The same iteration as the library runs it.  Coefficients: the state is (s, bu), s = u + bu, and one pass per iteration
    recovers u = s - bu, takes its sums, updates bu and forms the next s (analysis_restatement.salsa_analysis_operator).  Pixels:
    one pass per iteration on (Bx, v, bv) forms bv' = bv + (v - Bx) and the next v = (m y + mu2 (Bx - bv')) / (m + mu2) and
    takes the sums with the v the iteration solved with.  The solve is X = (conj(H) fft2(v + bv) + r fft2(W s)) / (|H|^2 + r),
    r = mu1 / mu2."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda z: mrdwt_TI2D(z, h, levels)
    Hc, H2 = np.conj(H), np.abs(H) ** 2
    T, r = tau / mu1, mu1 / mu2
    Bt = lambda z: np.real(np.fft.ifft2(Hc * np.fft.fft2(z)))
    x, numAt = _start(initialization, y, m, Bt)
    numA = 1

    def step(s, bu, w):
        """The coefficient pass: (|u|, u^2, (w-u)^2, w^2), the new bu, the next s, and u."""
        u = s - bu
        sums = (float(np.sum(np.abs(u))), _sq(u), _sq(w - u), _sq(w))
        bu = bu + (u - w)
        return sums, bu, soft(w - bu, T) + bu, u

    def pixel(Bx, v, bv):
        """The pixel pass: (m (Bx-y)^2, (Bx-v)^2, Bx^2, v^2), the new bv, the next v."""
        e = Bx - y
        sums = (float(np.sum(m * (e * e))), _sq(Bx - v), _sq(Bx), _sq(v))
        bv = bv + (v - Bx)
        return sums, bv, (m * y + mu2 * (Bx - bv)) / (m + mu2)

    Bx = np.real(np.fft.ifft2(H * np.fft.fft2(x)))
    w = WT(x)
    cs, bu, s, u = step(w, np.zeros_like(w), w)              # the start: s = w_0, bu = 0 gives u_0 = w_0, bu_0 = 0
    ps, bv, v = pixel(Bx, Bx, np.zeros_like(Bx))             # v = Bx_0, bv = 0 gives bv_0 = 0 and the first v
    objective = [0.5 * ps[0] + tau * cs[0]]
    times = [0.0]
    mses = [_sq(x - true_x) / x.size] if true_x is not None else []
    distance = []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = x
        z = W(s)
        X = (Hc * np.fft.fft2(v + bv) + r * np.fft.fft2(z)) / (H2 + r)
        numAt += 1
        x = np.real(np.fft.ifft2(X))
        Bx = np.real(np.fft.ifft2(H * X))
        numA += 1
        w = WT(x)
        cs, bu, s, u = step(s, bu, w)
        ps, bv, v = pixel(Bx, v, bv)
        objective.append(0.5 * ps[0] + tau * cs[0])
        if true_x is not None:
            mses.append(_sq(x - true_x) / x.size)
        distance.append([math.sqrt(cs[2]) / math.sqrt(cs[3] + cs[1]), math.sqrt(ps[1]) / math.sqrt(ps[2] + ps[3])])
        times.append(time.perf_counter() - t0)
        if outer > 1:
            if stopcriterion == 1:
                crit = abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]
            elif stopcriterion == 2:
                crit = abs(math.sqrt(_sq(x - xprev)) / math.sqrt(_sq(x)))
            else:
                crit = objective[outer]
            if crit < tolA:
                break
    return dict(x=x, numA=numA, numAt=numAt, objective=np.array(objective), distance=np.array(distance).reshape(-1, 2),
                times=np.array(times), mses=np.array(mses), n_outer=n_outer, u=u, bu=bu, bv=bv)


def calls(p, n_outer):
    """What the call counter advances by, as sbtv_SALSA_masked advances it: B' for the start 2, the start's B x, then the solve
    and H .* X per outer iteration (P and PT are not counted)."""
    start2 = not isinstance(p["init"], np.ndarray) and p["init"] == 2
    return 1 + (1 if start2 else 0) + 2 * n_outer
