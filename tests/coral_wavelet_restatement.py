"""NumPy restatement of CoRAL with a compound regulariser (include/sbtv.h, sbtv_CoRAL_wavelet):

    min over the IMAGE x   0.5 ||y - B x||^2 + tau1 phi1(P1' x) + tau2 phi2(P2' x)

`coral_literal` is SALSA/CoRAL_v2.m:349-476 line for line with general P1 / P1' / P2 / P2' handles; each term is either the
warm-started TV prox (chambolle_prox_TV_stop, phi = TVnorm: the reference's 'TVINITIALIZATION' = 1) or psi = soft with phi =
l1.  With P1 = P2 = identity and TV on both terms it is sbtv_oracle.CoRAL_v2 bit for bit (tests/test_coral_wavelet_cpu.py).
`coral_wavelet` is the configuration the library runs: P1 = identity with TV, P2 = W (mirdwt_TI2D), P2' = W' (mrdwt_TI2D) with
soft.  `coral_wavelet_operator` is that iteration in the state form of the device: pixel state x, u, bu, g1 = x - bu and
coefficient state (sv, bv), sv = v + bv.  The frame, soft and the stop rule are those of tests/wavelet_restatement.py, the TV
prox and TVnorm those of oracle/sbtv_oracle.py.  Nothing here imports the library."""
import math
import time

import numpy as np

import sbtv_oracle as o
from wavelet_restatement import _sq, mirdwt_TI2D, mrdwt_TI2D, soft

CHAMBOLLE_TOL = 1e-3                                         # chambolle_prox_TV_stop.m:77


def _start(initialization, y, ATy, AT):
    if isinstance(initialization, np.ndarray):
        return np.array(initialization, dtype=np.float64)
    if initialization == 0:
        return AT(np.zeros_like(y))                          # :329
    if initialization == 2:
        return ATy.copy()                                    # :333
    raise ValueError("Unknown 'Initialization' option")


def _l1(v):
    return float(np.sum(np.abs(v)))


class _Term:
    """One regulariser term: ('tv', TViters) or ('soft',).  prox(g, threshold) -> the minimiser; TV keeps its duals and records
    (k, err) of every call in `info`."""

    def __init__(self, spec):
        self.tv = spec[0] == "tv"
        self.iters = int(spec[1]) if self.tv else 0
        self.phi = o.TVnorm if self.tv else _l1
        self.duals = None
        self.info = []
        self.steps = []                                      # per call: the err of each of its k steps

    def arm(self, u):
        if self.tv:
            self.duals = (0 * u, 0 * u)                      # :385-386, 390-391

    def prox(self, g, threshold):
        if not self.tv:
            return soft(g, threshold)                        # :403, 408
        f, px, py, k, err = o.chambolle_prox_TV_stop(np.real(g), lam=threshold, maxiter=self.iters, dualvars=self.duals,
                                                     return_info=True)      # :401, 406
        self.steps.append(step_errors(np.real(g), threshold, k, self.duals, (px, py), err))
        self.duals = (px, py)
        self.info.append((k, err))
        return f


def step_errors(g, lam, k, duals, duals_after, err_after):
    """The `err` of each of the k steps of one prox call (return_info gives the last only): the same call one step at a time,
    which is the same arithmetic; held against the duals and the err of the call itself."""
    errs = []
    for _ in range(k):
        _, px, py, _, e = o.chambolle_prox_TV_stop(g, lam=lam, maxiter=1, dualvars=duals, return_info=True)
        duals = (px, py)
        errs.append(e)
    assert errs[-1] == err_after and np.array_equal(duals[0], duals_after[0]) and np.array_equal(duals[1], duals_after[1])
    return errs


def _criterion(stopcriterion, objective, outer, x, xprev):
    if stopcriterion == 1:
        return abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]          # :441
    if stopcriterion == 2:
        return abs(float(np.linalg.norm((x - xprev).ravel())) / float(np.linalg.norm(x.ravel())))   # :445
    return objective[outer]                                  # :448


def _rel_distance(PTx, u):
    return float(np.linalg.norm((PTx - u).ravel())) / math.sqrt(float(np.sum(PTx * PTx)) + float(np.sum(u * u)))


def coral_literal(y, A, AT, invLS, tau1, tau2, mu1, mu2, term1, term2, P1=None, P1T=None, P2=None, P2T=None, true_x=None,
                  stopcriterion=1, tolA=1e-3, maxiter=10000, initialization=0):
    """CoRAL_v2.m:182-476.  term1 / term2: ('tv', TViters) or ('soft',).  Returns x, u, v, bu, bv, the counters, the traces,
    `criterion` (entry outer - 1, entry 0 is 1 as in the reference) and, per TV term, `prox1` / `prox2`: the (k, err) of each
    prox call."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")       # :133
    ident = lambda a: a
    P1, P1T, P2, P2T = (f or ident for f in (P1, P1T, P2, P2T))
    t1, t2 = _Term(term1), _Term(term2)
    numA = numAt = 0
    ATy = AT(y)                                              # :189
    numAt += 1
    dummy = invLS(ATy)                                       # :199
    if dummy.shape != ATy.shape:
        raise ValueError("Specified function handle for solving the LS step does not seem compatible")
    ATy = AT(y)                                              # :219
    numAt += 1
    x = _start(initialization, y, ATy, AT)
    P1Tx = P1T(x)                                            # :349
    P2Tx = P2T(x)
    u = P1Tx.copy()                                          # :353-356
    bu = u.copy()
    threshold1 = tau1 / mu1
    v = P2Tx.copy()                                          # :358-361
    bv = v.copy()
    threshold2 = tau2 / mu2
    resid = y - A(x)                                         # :366
    numA += 1
    objective = [0.5 * float(np.sum(resid * resid)) + tau1 * t1.phi(u) + tau2 * t2.phi(v)]   # :368
    times = [0.0]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []        # :381
    t1.arm(u)
    t2.arm(v)
    distance = []
    criterion = [1.0]
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):                 # :394
        n_outer = outer
        xprev = x
        u = t1.prox(P1Tx - bu, threshold1)                   # :401-404
        v = t2.prox(P2Tx - bv, threshold2)                   # :406-409
        r = ATy + mu1 * P1(u + bu) + mu2 * P2(v + bv)        # :411
        x = invLS(r)                                         # :413
        P1Tx = P1T(x)                                        # :417-418
        P2Tx = P2T(x)
        bu = bu + (u - P1Tx)                                 # :420-421
        bv = bv + (v - P2Tx)
        resid = y - A(x)                                     # :423
        numA += 1
        objective.append(0.5 * float(np.sum(resid * resid)) + tau1 * t1.phi(u) + tau2 * t2.phi(v))   # :425
        if true_x is not None:
            e = x - true_x
            mses.append(float(np.sum(e * e)) / x.size)       # :428-429
        distance.append((_rel_distance(P1Tx, u), _rel_distance(P2Tx, v)))                   # :432-433
        times.append(time.perf_counter() - t0)
        if outer > 1:                                        # :435
            criterion.append(_criterion(stopcriterion, objective, outer, x, xprev))
            if criterion[-1] < tolA:                         # :453
                break
    return dict(x=x, u=u, v=v, bu=bu, bv=bv, numA=numA, numAt=numAt, n_outer=n_outer, objective=np.array(objective),
                distance=np.array(distance), times=np.array(times), mses=np.array(mses), criterion=np.array(criterion),
                prox1=t1.info, prox2=t2.info, steps1=t1.steps, steps2=t2.steps)


def blur_handles(H, mu):
    """A, AT and invLS of the circular blur with spectrum H (fft2 of the PSF)."""
    A = lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v)))
    AT = lambda v: np.real(np.fft.ifft2(np.conj(H) * np.fft.fft2(v)))
    invLS = lambda r: np.real(np.fft.ifft2(np.fft.fft2(r) / (np.abs(H) ** 2 + mu)))
    return A, AT, invLS


def coral_wavelet(y, H, h, levels, tau1, tau2, mu1, mu2, TViters=5, **kw):
    """coral_literal in the configuration of sbtv_CoRAL_wavelet: TV on the image, soft on W'x, invLS with mu1 + mu2."""
    y = np.asarray(y, dtype=np.float64)
    A, AT, invLS = blur_handles(H, mu1 + mu2)                # :137
    return coral_literal(y, A, AT, invLS, tau1, tau2, mu1, mu2, ("tv", TViters), ("soft",),
                         P2=lambda c: mirdwt_TI2D(c, h, levels), P2T=lambda a: mrdwt_TI2D(a, h, levels), **kw)


def coral_wavelet_operator(y, H, h, levels, tau1, tau2, mu1, mu2, TViters=5, true_x=None, stopcriterion=1, tolA=1e-3,
                           maxiter=10000, initialization=0):
    """The same iteration as the library runs it.  Pixel state x, u, bu and g1 = x - bu (the next prox input); coefficient state
    (sv, bv) with sv = v + bv.  The start is sv = bv = W'x: the first soft argument is exactly zero.  The spectral solve takes
    fft2(y) and s = (mu1 (u + bu) + mu2 W sv) / mu, the residual comes from the spectrum of x, one coefficient pass recovers
    v = sv - bv, takes its sums, updates bv and forms the next sv, one pixel pass updates bu and forms g1."""
    y = np.asarray(y, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda a: mrdwt_TI2D(a, h, levels)
    Y = np.fft.fft2(y)
    Hc, H2 = np.conj(H), np.abs(H) ** 2
    mu = mu1 + mu2
    T1, T2 = tau1 / mu1, tau2 / mu2
    BT = lambda a: np.real(np.fft.ifft2(Hc * np.fft.fft2(a)))
    x = _start(initialization, y, BT(y), BT)
    numA, numAt = 1, 2
    u, bu, g1 = x.copy(), x.copy(), np.zeros_like(x)
    sv = WT(x)
    bv = sv.copy()
    duals = (np.zeros_like(x), np.zeros_like(x))
    resid = y - np.real(np.fft.ifft2(H * np.fft.fft2(x)))
    objective = [0.5 * _sq(resid) + tau1 * o.TVnorm(u) + tau2 * _l1(sv)]
    times = [0.0]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []
    distance, prox = [], []
    t0 = time.perf_counter()
    n_outer = 0
    v = sv
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = x
        u, px, py, k, err = o.chambolle_prox_TV_stop(g1, lam=T1, maxiter=TViters, dualvars=duals, return_info=True)
        duals = (px, py)
        prox.append((k, err))
        z = W(sv)
        s = (mu1 * (u + bu) + mu2 * z) / mu                  # the s pass
        X = (Hc * Y + mu * np.fft.fft2(s)) / (H2 + mu)
        x = np.real(np.fft.ifft2(X))
        resid = y - np.real(np.fft.ifft2(H * X))
        w = WT(x)
        v = sv - bv                                          # the step pass
        cs = (_l1(v), _sq(v), _sq(w - v), _sq(w))
        bv = bv + (v - w)
        sv = soft(w - bv, T2) + bv
        bu = bu + (u - x)                                    # the post pass
        g1 = x - bu
        numA += 1
        objective.append(0.5 * _sq(resid) + tau1 * o.TVnorm(u) + tau2 * cs[0])
        if true_x is not None:
            mses.append(_sq(x - true_x) / x.size)
        distance.append((math.sqrt(_sq(x - u)) / math.sqrt(_sq(x) + _sq(u)), math.sqrt(cs[2]) / math.sqrt(cs[3] + cs[1])))
        times.append(time.perf_counter() - t0)
        if outer > 1 and _criterion(stopcriterion, objective, outer, x, xprev) < tolA:
            break
    return dict(x=x, u=u, v=v, bu=bu, bv=bv, numA=numA, numAt=numAt, n_outer=n_outer, objective=np.array(objective),
                distance=np.array(distance), times=np.array(times), mses=np.array(mses), prox1=prox)
