"""CPU: the dtype-generic evaluator of the wavelet frame (tests/wavelet_longdouble.py) gives the bits of
tests/wavelet_restatement.py in float64, is a Parseval frame to long-double precision in np.longdouble, and sizes the bar of
tests/test_gpu_wavelet_sweep.py far below the 1e-12 max|x| of tests/test_gpu_wavelet.py."""
import numpy as np
import pytest

import wavelet_longdouble as wl
import wavelet_restatement as wr

EPS = float(np.finfo(np.float64).eps)
CASES = [((2, 2), 2, 2), ((13, 13), 4, 4), ((65, 33), 8, 4), ((150, 131), 8, 5), ((96, 160), 2, 7), ((257, 129), 6, 6)]


def _h(K):
    import sbtv
    return sbtv.daubcqf(K)


@pytest.mark.parametrize("shape,K,levels", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_float64_bits_and_long_double_error(shape, K, levels):
    h = _h(K)
    rng = np.random.default_rng(shape[0] + K)
    x = rng.standard_normal((2,) + shape) * 100.0
    z64 = wl.analysis(x, h, levels, np.float64)
    np.testing.assert_array_equal(z64, np.stack([wr.mrdwt_TI2D(x[b], h, levels) for b in range(2)]))
    c = rng.standard_normal(z64.shape) * 100.0
    s64 = wl.synthesis(c, h, levels, np.float64)
    np.testing.assert_array_equal(s64, np.stack([wr.mirdwt_TI2D(c[b], h, levels) for b in range(2)]))
    zl, sl = wl.analysis(x, h, levels), wl.synthesis(c, h, levels)
    assert zl.dtype == wl.LD and sl.dtype == wl.LD
    scale = float(np.max(np.abs(x)))
    own_a = float(np.max(np.abs(z64.astype(wl.LD) - zl))) / scale
    own_s = float(np.max(np.abs(s64.astype(wl.LD) - sl))) / float(np.max(np.abs(c)))
    print(f"{shape} K={K} levels={levels}: float64 against long double, analysis {own_a / EPS:.2f} eps, synthesis "
          f"{own_s / EPS:.2f} eps of the largest input")
    # a few roundings per level, relative to values of the input's size: the bar of the sweep, 16 x this, stays two orders
    # of magnitude under 1e-12
    assert 0 < own_a <= 8 * EPS and 0 < own_s <= 8 * EPS
    # the long-double evaluation is itself a Parseval frame and an adjoint pair to its own precision (h is float64 data,
    # orthonormal to about 1e-16 only: the identities are checked on the reconstruction through the SAME filters' error)
    back = wl.synthesis(zl, h, levels)
    lhs, rhs = np.sum(zl * c.astype(wl.LD)), np.sum(x.astype(wl.LD) * sl)
    assert abs(lhs - rhs) <= 1e-17 * float(np.linalg.norm(zl.astype(np.float64)) * np.linalg.norm(c))
    assert float(np.max(np.abs(back - x))) <= 64 * EPS * scale       # limited by the filter's own orthonormality


def test_structural_support_of_a_delta():
    """All-ones filters: positive where the definition puts a contribution, 0.0 elsewhere; the real filters vanish off it."""
    M, N, K, levels = 23, 19, 4, 4
    h = _h(K)
    x = np.zeros((M, N))
    x[5, 17] = 3.0
    pat = wl.analysis(x, None, levels, np.float64, wl.ones_filters(K))
    z = wl.analysis(x, h, levels)
    assert np.all(pat >= 0) and np.all(z[pat == 0] == 0)
    lh1 = pat[:, N:2 * N]                                                  # level 1: taps reach back K - 1 along each dimension
    rows, cols = np.nonzero(lh1)
    assert sorted(set(rows)) == [2, 3, 4, 5] and sorted(set(cols)) == [14, 15, 16, 17]
    a3 = pat[:, :N]                                                       # a_J: reach (K - 1)(1 + 2 + 4) = 21 back, modulo n
    assert np.count_nonzero(a3[:, 17]) == 22 and a3[6, 17] == 0
    # the transpose: one coefficient of the deepest approximation spreads forward by the same reach
    c = np.zeros_like(pat)
    c[5, 17] = 1.0
    ps = wl.synthesis(c, None, levels, np.float64, wl.ones_filters(K))
    assert np.count_nonzero(ps[:, 17]) == 22 and ps[4, 17] == 0 and ps[5, 17] > 0


@pytest.mark.parametrize("dtype", [np.float64, wl.LD], ids=["float64", "longdouble"])
def test_the_evaluator_commutes_with_circular_shifts_bit_for_bit(dtype):
    """Every output sample runs the same operations in the same order whatever its position, so the transform of a shifted
    input is the shifted transform to the last bit: tests/test_gpu_wavelet_sweep.py computes one impulse response per band
    and moves it to every impulse position."""
    M, N, K, levels = 21, 17, 6, 3
    nb = 3 * (levels - 1) + 1
    h = _h(K)
    x = np.random.default_rng(5).standard_normal((M, N))
    z = wl.analysis(x, h, levels, dtype)
    zs = wl.analysis(np.roll(x, (4, 15), axis=(0, 1)), h, levels, dtype)
    np.testing.assert_array_equal(zs, np.roll(z.reshape(M, nb, N), (4, 15), axis=(0, 2)).reshape(M, nb * N))
    c = np.random.default_rng(6).standard_normal((M, nb * N))
    w = wl.synthesis(c, h, levels, dtype)
    ws = wl.synthesis(np.roll(c.reshape(M, nb, N), (20, 1), axis=(0, 2)).reshape(M, nb * N), h, levels, dtype)
    np.testing.assert_array_equal(ws, np.roll(w, (20, 1), axis=(0, 1)))
