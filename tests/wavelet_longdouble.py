"""The redundant wavelet frame of include/sbtv.h evaluated from its definition in any floating-point type, for stacks of
images: the long-double reference of tests/test_gpu_wavelet_sweep.py.

Same formulas and the same order of operations as tests/wavelet_restatement.py (`_filt`, `_filt_adj`, `mrdwt_TI2D`,
`mirdwt_TI2D`), so in float64 it gives that module's bits (tests/test_wavelet_longdouble_cpu.py); in np.longdouble the taps h
(float64 data, exact in the wider type) are applied with a long-double 1/sqrt 2 and long-double sums.  Arrays are
(..., M, N) images and (..., M, (3J+1) N) coefficients.  `filters=(f0, f1)` replaces the pair derived from h: with all-ones
filters a delta's transform is positive exactly where the index arithmetic of the definition puts a contribution and 0.0
elsewhere (the STRUCTURAL support: no cancellation between taps can hide or fake an entry).  Nothing here imports the
library."""
import numpy as np

LD = np.longdouble
# a platform whose long double is the 64-bit double would compare float64 with itself
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an 80-bit (or wider) type on this platform"


def filter_pair(h, dtype):
    """(h0, h1) in `dtype`: h0 = h, h1[k] = (-1)^k h[K-1-k]."""
    h = np.asarray(h, dtype=np.float64).astype(dtype)
    K = h.size
    return h, np.array([(-1.0) ** k * h[K - 1 - k] for k in range(K)], dtype=dtype)


def _shift_add(out, a, fk, sh, axis):
    """out += fk * roll(a, -sh, axis) without the rolled copy; axis -2 or -1."""
    n = a.shape[axis]
    sh %= n
    o, v = np.moveaxis(out, axis, 0), np.moveaxis(a, axis, 0)
    if sh == 0:
        o += fk * v
    else:
        o[:n - sh] += fk * v[sh:]
        o[n - sh:] += fk * v[:sh]


def filt(a, f, s, axis, adjoint=False):
    """sum_k f[k] a[(i + s k) mod n] / sqrt 2 along `axis` (-2: dimension 1, -1: dimension 2); adjoint: index i - s k."""
    out = np.zeros_like(a)
    for k, fk in enumerate(f):
        _shift_add(out, a, fk, -s * k if adjoint else s * k, axis)
    out /= np.sqrt(a.dtype.type(2))
    return out


def analysis(x, h, levels, dtype=LD, filters=None):
    """W': (..., M, N) -> (..., M, (3J+1) N), [a_J | LH1 HL1 HH1 | LH2 ...]."""
    a = np.asarray(x).astype(dtype)
    h0, h1 = filters if filters is not None else filter_pair(h, dtype)
    det = []
    for j in range(1, levels):
        s = 2 ** (j - 1)
        lo, hi = filt(a, h0, s, -2), filt(a, h1, s, -2)
        det += [filt(lo, h1, s, -1), filt(hi, h0, s, -1), filt(hi, h1, s, -1)]
        a = filt(lo, h0, s, -1)
    return np.concatenate([a] + det, axis=-1)


def synthesis(z, h, levels, dtype=LD, filters=None):
    """W, the exact adjoint of `analysis`: (..., M, (3J+1) N) -> (..., M, N)."""
    z = np.asarray(z).astype(dtype)
    h0, h1 = filters if filters is not None else filter_pair(h, dtype)
    J = levels - 1
    N = z.shape[-1] // (3 * J + 1)
    band = lambda b: z[..., b * N:(b + 1) * N]
    a = band(0)
    for j in range(J, 0, -1):
        s = 2 ** (j - 1)
        lh, hl, hh = (band(1 + 3 * (j - 1) + q) for q in range(3))
        lo = filt(a, h0, s, -1, True) + filt(lh, h1, s, -1, True)
        hi = filt(hl, h0, s, -1, True) + filt(hh, h1, s, -1, True)
        a = filt(lo, h0, s, -2, True) + filt(hi, h1, s, -2, True)
    return a


def ones_filters(K):
    f = np.ones(K)
    return f, f
