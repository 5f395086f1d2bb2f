"""NumPy restatement of the analysis-prior wavelet SALSA (include/sbtv.h, sbtv_SALSA_analysis):

    min over the IMAGE x   0.5 ||y - B x||^2 + tau ||W' x||_1

`salsa_analysis_literal` is SALSA/SALSA_v2.m:262-494 line for line with TVINITIALIZATION = 0, Psi = soft, Phi = l1, A = B,
AT = B', PT = W' (mrdwt_TI2D), P = W (mirdwt_TI2D) and invLS(r) = real(ifft2(fft2(r) ./ (|H|^2 + mu))), the exact x-minimiser
because W W' = I.  `salsa_analysis_operator` is the form the library runs, on the coefficient state (s, bu), s = u + bu.  The
frame, soft and the stop rule are those of tests/wavelet_restatement.py.  Nothing here imports the library."""
import math
import time

import numpy as np

from wavelet_restatement import _sq, _stop, _traces, mirdwt_TI2D, mrdwt_TI2D, soft


def _start(initialization, y, ATy, AT):
    if isinstance(initialization, np.ndarray):
        return np.array(initialization, dtype=np.float64)    # :374-378
    if initialization == 0:
        return AT(np.zeros_like(y))                          # :369
    if initialization == 2:
        return ATy.copy()                                    # :373
    raise ValueError("Unknown 'Initialization' option")


def salsa_analysis_literal(y, H, h, levels, tau, mu, true_x=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                           initialization=0):
    """H: fft2 of the PSF.  Returns x, u, bu, the counters and the traces; `criterion` holds the stop criterion of every
    iteration from the second on (entry outer - 2), whichever rule is in force."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Unknown stopping criterion")
    y = np.asarray(y, dtype=np.float64)
    P = lambda c: mirdwt_TI2D(c, h, levels)
    PT = lambda v: mrdwt_TI2D(v, h, levels)
    A = lambda v: np.real(np.fft.ifft2(H * np.fft.fft2(v)))
    AT = lambda v: np.real(np.fft.ifft2(np.conj(H) * np.fft.fft2(v)))
    invLS = lambda r: np.real(np.fft.ifft2(np.fft.fft2(r) / (np.abs(H) ** 2 + mu)))
    numA = numAt = 0
    ATy = AT(y)                                              # :288
    numAt += 1
    x = _start(initialization, y, ATy, AT)
    PTx = PT(x)                                              # :389
    u = PTx                                                  # :392
    bu = 0 * u                                               # :393
    threshold = tau / mu                                     # :394
    resid = y - A(x)                                         # :399
    numA += 1
    objective = [0.5 * _sq(resid) + tau * float(np.sum(np.abs(u)))]     # :401
    times = [0.0]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []      # :415
    distance, criterion = [], []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):                 # :423
        n_outer = outer
        xprev = x                                            # :425
        u = soft(PTx - bu, threshold)                        # :431
        r = ATy + mu * P(u + bu)                             # :434
        x = invLS(r)                                         # :436
        PTx = PT(x)                                          # :438
        bu = bu + (u - PTx)                                  # :440
        resid = y - A(x)                                     # :442
        numA += 1
        objective.append(0.5 * _sq(resid) + tau * float(np.sum(np.abs(u))))   # :444
        if true_x is not None:
            err = x - true_x
            mses.append(_sq(err) / x.size)                   # :446-449
        distance.append(math.sqrt(_sq(PTx - u)) / math.sqrt(_sq(PTx) + _sq(u)))           # :451
        times.append(time.perf_counter() - t0)
        if outer > 1:                                        # :453-482
            criterion.append(_criterion(stopcriterion, objective, outer, x, xprev))
            if _stop(stopcriterion, objective, outer, x, xprev, tolA):
                break
    return dict(x=x, u=u, bu=bu, numA=numA, numAt=numAt, n_outer=n_outer, criterion=np.array(criterion),
                **_traces(objective, distance, times, mses))


def _criterion(stopcriterion, objective, outer, x, xprev):
    """The number _stop compares with tolA (SALSA_v2.m:456-466)."""
    if stopcriterion == 1:
        return abs(objective[outer] - objective[outer - 1]) / objective[outer - 1]
    if stopcriterion == 2:
        return abs(float(np.linalg.norm((x - xprev).ravel())) / float(np.linalg.norm(x.ravel())))
    return objective[outer]


def salsa_analysis_operator(y, H, h, levels, tau, mu, true_x=None, stopcriterion=1, tolA=1e-3, maxiter=10000,
                            initialization=0):
    """The same iteration as the library runs it: the coefficient state is (s, bu) with s = u + bu, the spectral solve takes
    fft2(y) and z = W s, the residual comes from the spectrum of x, and one coefficient pass per iteration recovers u = s - bu,
    takes the sums, updates bu and forms the next s (where u was thresholded to zero, s == bu bit for bit)."""
    y = np.asarray(y, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    Y = np.fft.fft2(y)
    Hc, H2 = np.conj(H), np.abs(H) ** 2
    T = tau / mu
    BT = lambda v: np.real(np.fft.ifft2(Hc * np.fft.fft2(v)))
    x = _start(initialization, y, BT(y), BT)
    numA, numAt = 1, 1

    def step(s, bu, w):
        """The coefficient pass: (|u|, u^2, (w-u)^2, w^2), the new bu, the next s, and u."""
        u = s - bu
        sums = (float(np.sum(np.abs(u))), _sq(u), _sq(w - u), _sq(w))
        bu = bu + (u - w)
        return sums, bu, soft(w - bu, T) + bu, u

    w = WT(x)
    sums, bu, s, u = step(w, np.zeros_like(w), w)            # the start: s = w_0, bu = 0 gives u_0 = w_0, bu_0 = 0
    resid = y - np.real(np.fft.ifft2(H * np.fft.fft2(x)))
    objective = [0.5 * _sq(resid) + tau * sums[0]]
    times = [0.0]
    mses = [float(np.sum((x - true_x) ** 2)) / x.size] if true_x is not None else []
    distance = []
    t0 = time.perf_counter()
    n_outer = 0
    for outer in range(1, int(maxiter) + 1):
        n_outer = outer
        xprev = x
        z = W(s)
        X = (Hc * Y + mu * np.fft.fft2(z)) / (H2 + mu)
        x = np.real(np.fft.ifft2(X))
        resid = y - np.real(np.fft.ifft2(H * X))
        w = WT(x)
        sums, bu, s, u = step(s, bu, w)
        numA += 1
        objective.append(0.5 * _sq(resid) + tau * sums[0])
        if true_x is not None:
            mses.append(_sq(x - true_x) / x.size)
        distance.append(math.sqrt(sums[2]) / math.sqrt(sums[3] + sums[1]))
        times.append(time.perf_counter() - t0)
        if outer > 1 and _stop(stopcriterion, objective, outer, x, xprev, tolA):
            break
    return dict(x=x, u=u, bu=bu, numA=numA, numAt=numAt, n_outer=n_outer, **_traces(objective, distance, times, mses))
