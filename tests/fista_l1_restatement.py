"""NumPy restatement of the wavelet-l1 FISTA (include/sbtv.h, sbtv_fista_l1) on the frame of tests/wavelet_restatement.py.

`fista_l1_literal` is SALSA/my_fista_l1.m:5-68 line for line (with L, a start other than zero and an optional `true` as its
only extensions); `fista_l1_operator` is the one-synthesis form the library runs: the momentum point y is never stored, its
image W y is formed from the images of the last two iterates.  Nothing here imports the library."""
import math
import time

import numpy as np

from wavelet_restatement import _sq, mirdwt_TI2D, mrdwt_TI2D, soft


def _criterion(stopcriterion, objective, x, x_old):
    """my_fista_l1.m:49-58 with IEEE semantics: rule 2 at x = 0 is 0 / 0 = NaN."""
    if stopcriterion == 1:
        return abs(objective[-1] - objective[-2]) / objective[-1]
    if stopcriterion == 2:
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(math.sqrt(_sq(x - x_old))) / np.float64(math.sqrt(_sq(x))))
    if stopcriterion == 3:
        return objective[-1]
    raise ValueError("Invalid stopping criterion!")


def _result(x, Wx, objective, times, mses, criteria, calls):
    return dict(xw=x, x=Wx, objective=np.array(objective), times=np.array(times), mses=np.array(mses),
                criteria=np.array(criteria), n_iter=len(objective), calls=calls)


def fista_l1_literal(b, H, h, levels, tau, stopcriterion, tolerance, maxiters, true_xw=None, L=1.0, xw_init=None):
    """my_fista_l1.m.  H: fft2 of the full-size kernel.  `criteria[k-2]` is the criterion of iteration k."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Invalid stopping criterion!")
    b = np.asarray(b, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    HC = np.conj(H)
    calls = [0]

    def A(x):                                                            # :12,17
        calls[0] += 1
        return np.real(np.fft.ifft2(H * np.fft.fft2(W(x))))

    def AT(x):                                                           # :13,18
        calls[0] += 1
        return WT(np.real(np.fft.ifft2(HC * np.fft.fft2(x))))

    x = np.zeros_like(AT(b))                                             # :20
    if xw_init is not None:
        x = np.array(xw_init, dtype=np.float64)
    y = x.copy()                                                         # :21
    t = 1.0                                                              # :22
    times = [0.0]                                                        # :24
    t0 = time.perf_counter()
    Wx = W(x)                                                            # :27
    objective = [0.5 * _sq(A(x) - b) + tau * float(np.sum(np.abs(x)))]   # :28
    mses = [_sq(x - true_xw) / x.size] if true_xw is not None else []    # :29
    criteria = []
    for k in range(2, int(maxiters) + 1):                                # :34
        x_old = x                                                        # :35
        t_old = t                                                        # :36
        y = y - (1.0 / L) * AT(A(y) - b)                                 # :38
        x = soft(y, tau / L)                                             # :39
        t = 0.5 * (1 + math.sqrt(1 + 4 * t_old ** 2))                    # :41
        y = x + ((t_old - 1) / t) * (x - x_old)                          # :42
        Wx = W(x)                                                        # :43
        objective.append(0.5 * _sq(A(x) - b) + tau * float(np.sum(np.abs(x))))   # :44
        if true_xw is not None:
            mses.append(_sq(x - true_xw) / x.size)                       # :45
        times.append(time.perf_counter() - t0)                           # :47
        criteria.append(_criterion(stopcriterion, objective, x, x_old))  # :49-58
        if criteria[-1] < tolerance:                                     # :64
            break
    return _result(x, Wx, objective, times, mses, criteria, calls[0])


def fista_l1_operator(b, H, h, levels, tau, stopcriterion, tolerance, maxiters, true_xw=None, L=1.0, xw_init=None):
    """The form the library runs: x_{k-1}, x_{k-2} and their images zx = W x; with c the momentum factor of the iteration
    before (0 for k = 2)
        zy = zx_{k-1} + c (zx_{k-1} - zx_{k-2}) ; g = W' B'(B zy - b)
        x_k = soft((x_{k-1} + c (x_{k-1} - x_{k-2})) - (1/L) g, tau/L) ; zx_k = W x_k ; objective from B zx_k - b
    one synthesis per iteration.  `calls` is what the reference would count, 2 + 3 (n_iter - 1)."""
    if stopcriterion not in (1, 2, 3):
        raise ValueError("Invalid stopping criterion!")
    b = np.asarray(b, dtype=np.float64)
    W = lambda c: mirdwt_TI2D(c, h, levels)
    WT = lambda v: mrdwt_TI2D(v, h, levels)
    HC = np.conj(H)
    Bf = np.fft.fft2(b)
    nbands = 3 * (levels - 1) + 1
    if xw_init is not None:
        x = np.array(xw_init, dtype=np.float64)
    else:
        x = np.zeros((b.shape[0], nbands * b.shape[1]))
    x_old = x
    zx = W(x)
    zx_old = zx
    resid2 = lambda z: _sq(np.real(np.fft.ifft2(H * np.fft.fft2(z) - Bf)))
    objective = [0.5 * resid2(zx) + tau * float(np.sum(np.abs(x)))]
    mses = [_sq(x - true_xw) / x.size] if true_xw is not None else []
    times, criteria = [0.0], []
    t0 = time.perf_counter()
    t, c = 1.0, 0.0
    calls = 2
    for k in range(2, int(maxiters) + 1):
        zy = zx + c * (zx - zx_old)
        g = WT(np.real(np.fft.ifft2(HC * (H * np.fft.fft2(zy) - Bf))))
        xn = soft((x + c * (x - x_old)) - (1.0 / L) * g, tau / L)
        x_old, x = x, xn
        zx_old, zx = zx, W(x)
        t_old = t
        t = 0.5 * (1 + math.sqrt(1 + 4 * t_old ** 2))
        c = (t_old - 1) / t
        calls += 3
        objective.append(0.5 * resid2(zx) + tau * float(np.sum(np.abs(x))))
        if true_xw is not None:
            mses.append(_sq(x - true_xw) / x.size)
        times.append(time.perf_counter() - t0)
        criteria.append(_criterion(stopcriterion, objective, x, x_old))
        if criteria[-1] < tolerance:
            break
    return _result(x, zx, objective, times, mses, criteria, calls)
