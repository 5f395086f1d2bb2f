"""GPU sweep of the wavelet frame kernels (wav_analysis_kernel<K>, wav_synthesis_kernel<K>, K = 2, 4, 6, 8, csrc/wavelet.hip)
and of sbtv_soft over every tile-geometry class.

Sizes come from tests/wavelet_geometry_cases.py, whose CPU test proves that they reach every class.  Before anything is
launched the geometry the library REPORTS (`Context.wavelet_geometry`, every level of every case) is compared with the
model of that module, and the classes are derived a second time from the reports.  Everything a kernel is compared with is
the transform evaluated from its definition in np.longdouble (tests/wavelet_longdouble.py); the float64 restatement of the
same formulas is computed alongside only to size the bar.

Bar.  err(.) = largest absolute difference from the long-double reference, own = err(float64 restatement):
    bar = max(16 own, 16 eps max|reference|),
per band for the analysis.  The device multiplies by taps pre-scaled by 1/sqrt 2 (one more rounding per tap; the restatement
divides each sum by sqrt 2 instead) and sums in tap order inside LDS tiles: a few roundings per level either way.  Both carry a
systematic part of about 0.3 eps per 1-D filter from their rounded constant, so both grow alike with the depth.  Every bar
is asserted to lie below the 1e-12 max|x| of tests/test_gpu_wavelet.py (it is about 1e-14 max|x| at the deepest cases).
The adjoint and Parseval identities on the device's own outputs keep their 1e-11.

Impulses.  For the marked cases a delta is put at every position of `impulse_points` (index 0, the last sample, both sides
of the first tile seam of every level and pass, the first sample of the second run of a comb level; along each dimension).
The analysis must be EXACTLY 0.0 outside the structural support (the transform of the delta through all-ones filters) and
within the bar on it.  The transpose: one non-zero coefficient at the same positions in the four bands of the deepest
level (a_J and its three details) and the three detail bands of level 1 (a_1 is not an input unless J = 1), exactly zero
off the support and within the bar on it.  A random field averages an index error into a maximum; an impulse shows it at its
position.

Largest device error / own error over the module (one MI355X): analysis 2.42 (K = 4, 129x5, levels 2), synthesis 1.80 (K = 8,
15x16, levels 3), W W'x 2.00 (K = 2, 9x9, levels 5), impulses 2.93 (K = 4); per K in DESIGN.md 3.8.  No kernel bug was found.

Mutants of csrc/wavelet.hip, one at a time on a scratch copy (never committed), against this module and the twelve
TRANSFORM_CASES of tests/test_gpu_wavelet.py (F = fails, . = passes):
                                                                          this  test_gpu_wavelet
  1 wav_cap2 returns 4 for K = 6 (the LDS arrays follow it)                 F         .
  2 WS_T2 where WA_T2 belongs in the analysis grid                         F         .
  3 f1[3] * (1 + 1e-13) for K = 8                                          F         .
  4 wav_wrap maps an index >= 2n to n - 1 instead of i % n                 .         .
  5 wav_base sends every run above the first to run 1 (s >= 4 cap only)    F         F
1 and 2 compute correct images (2 launches tiles that store nothing): only the model-against-library assertion shows them.
3 gives 4.1e-12 against a bar of 1.6e-12 at 114x113 (and 2.5e-13 against 5.1e-14 on the impulses).  4 is equivalent as far as
values go: an index >= 2n only feeds outputs beyond the image, which are not stored (tests/wavelet_geometry_cases.py, "wrap").

sbtv_soft.  One lane's second trip through the grid-stride loop needs P = 2048 * 256 + 2 per image; 1024 x 513 (the shape
named beside it) is P = 2048 * 256 + 1024, 1024 lanes' second trip: both run, each as a batch of two with two thresholds.
x = +-inf is kept out of the image whose threshold is inf: inf - inf has no value to pin (fmax drops the NaN on the
device, NumPy's maximum keeps it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import wavelet_geometry_cases as wg
import wavelet_longdouble as wl
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = wl.LD
EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
RATIOS = {}                                # (K, quantity) -> (largest device error / own error, device error, own, bar, case)


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    for key in sorted(RATIOS):
        r, e, own, bar, case = RATIOS[key]
        print("WAVELET SWEEP K=%d %-22s worst device / own error %6.2f  (error %.3e, own %.3e, bar %.3e) at %s"
              % (key[0], key[1], r, e, own, bar, case))


def new_bar(ref_ld, ref_f64):
    """(bar, own): 16 x the float64 restatement's own error, floored at 16 eps relative to the largest reference value."""
    scale = float(np.max(np.abs(ref_ld)))
    own = float(np.max(np.abs(np.asarray(ref_f64).astype(LD) - ref_ld)))
    return max(MARGIN * own, MARGIN * EPS * scale), own


def err(got, ref_ld):
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref_ld)))


def check(K, quantity, got, ref_ld, ref_f64, old_scale, case):
    """Record device error / own error, assert the bar below the old one, then the error below the bar."""
    bar, own = new_bar(ref_ld, ref_f64)
    e = err(got, ref_ld)
    r = e / own if own > 0 else (0.0 if e == 0 else np.inf)
    key = (K, quantity)
    if key not in RATIOS or r > RATIOS[key][0]:
        RATIOS[key] = (r, e, own, bar, case)
    assert bar < 1e-12 * old_scale, "%s at %s: the bar %.3e is not below 1e-12 max|x| = %.3e" % (quantity, case, bar, 1e-12 * old_scale)
    assert e <= bar, "%s at %s: error %.3e against the long-double reference, bar %.3e (float64 restatement: %.3e)" % (
        quantity, case, e, bar, own)


def reported(ctx, M, N, K, levels):
    """The library's geometry of every level, checked against the model before any launch."""
    rep = [ctx.wavelet_geometry(M, N, K, levels, j) for j in range(1, levels)]
    assert rep == wg.model_report(M, N, K, levels), ("the library's wavelet geometry differs from the model", M, N, K, levels, rep)
    return rep


def bands(levels):
    return 3 * (levels - 1) + 1


def analysis_dev(ctx, x, h, levels):
    """(B, M, N) -> (B, M, nb N) through sbtv_mrdwt_TI2D, host pointers."""
    import sbtv
    return np.asarray(sbtv.mrdwt_TI2D(x, h, levels, ctx=ctx)).reshape(x.shape[0], x.shape[1], -1)


def synthesis_dev(ctx, z, h, levels):
    import sbtv
    return np.asarray(sbtv.mirdwt_TI2D(z, h, levels, ctx=ctx)).reshape(z.shape[0], z.shape[1], -1)


# ---------------------------------------------------------------------------------------------------------------------
# 0. the geometry the library reports: the model's, and the list reaches every class through it
# ---------------------------------------------------------------------------------------------------------------------
def test_reported_geometry_reaches_every_class(ctx):
    import sbtv
    rep = lambda M, N, K, levels: reported(ctx, M, N, K, levels)
    cov = wg.assert_coverage(wg.CASES, wg.REQUIRED, rep)
    assert cov == wg.coverage(wg.CASES)
    for (M, N), K, levels, batch in ((c[0], c[1], c[2], c[3]) for c in wg.CASES):
        assert wg.classes(M, N, K, levels, batch, rep(M, N, K, levels)) == wg.classes(M, N, K, levels, batch)
    # the static LDS is what the loaded kernels state, not a formula of the library's
    for K in wg.KS:
        g = ctx.wavelet_geometry(64, 64, K, 2, 1)
        assert (g["lds_analysis"], g["lds_synthesis"]) == wg.lds_bytes(K)
    # refused as the transforms refuse, with their codes; a level outside 1..J
    for args, code in (((32, 32, 3, 3, 1), -1), ((32, 32, 10, 2, 1), -1), ((32, 32, 4, 1, 1), -1), ((12, 12, 4, 4, 1), -2),
                       ((40, 12, 4, 4, 1), -2), ((0, 12, 4, 2, 1), -2), ((32, 32, 4, 80, 1), -2), ((32, 32, 4, 3, 0), -1),
                       ((32, 32, 4, 3, 3), -1)):
        with pytest.raises(sbtv.SbtvError) as e:
            ctx.wavelet_geometry(*args)
        assert e.value.code == code, (args, e.value.code)
    assert ctx.wavelet_geometry(13, 13, 4, 4, 3)["s"] == 4                     # reach 12 < 13 is accepted


# ---------------------------------------------------------------------------------------------------------------------
# 1. every case: random fields against the long-double reference, the identities, the batch
# ---------------------------------------------------------------------------------------------------------------------
def run_case(ctx, case):
    import sbtv
    (M, N), K, levels, batch, marks = case
    where = "%dx%d K=%d levels=%d batch=%d" % (M, N, K, levels, batch)
    reported(ctx, M, N, K, levels)
    h = sbtv.daubcqf(K)
    nb = bands(levels)
    rng = np.random.default_rng([M, N, K, levels, batch])                     # an input of the case's own
    x = rng.standard_normal((batch, M, N)) * 100.0
    c = rng.standard_normal((batch, M, nb * N)) * 100.0
    xs, cs = float(np.max(np.abs(x))), float(np.max(np.abs(c)))
    # analysis, every band
    z = analysis_dev(ctx, x, h, levels)
    z_ld = wl.analysis(x, h, levels)
    z_64 = np.stack([wr.mrdwt_TI2D(x[b], h, levels) for b in range(batch)])
    for b in range(nb):
        sl = slice(b * N, (b + 1) * N)
        check(K, "analysis", z[..., sl], z_ld[..., sl], z_64[..., sl], xs, where + " band %d" % b)
    # synthesis of random coefficients
    w = synthesis_dev(ctx, c, h, levels)
    check(K, "synthesis", w, wl.synthesis(c, h, levels), np.stack([wr.mirdwt_TI2D(c[b], h, levels) for b in range(batch)]),
          cs, where)
    # W W'x = x: the device's round trip against x, sized by the restatement's round trip
    back = synthesis_dev(ctx, z, h, levels)
    check(K, "W W'x - x", back, x.astype(LD), np.stack([wr.mirdwt_TI2D(z_64[b], h, levels) for b in range(batch)]), xs, where)
    # the identities on the device's own outputs
    for b in range(batch):
        lhs, rhs = float(np.vdot(z[b], c[b])), float(np.vdot(x[b], w[b]))
        adj = abs(lhs - rhs) / (np.linalg.norm(z[b]) * np.linalg.norm(c[b]))
        pars = abs(np.linalg.norm(z[b]) / np.linalg.norm(x[b]) - 1.0)
        assert adj <= 1e-11 and pars <= 1e-11, (where, b, adj, pars)
    # image b of the batched call is the single call on image b, bit for bit
    if batch > 1:
        for b in range(batch):
            np.testing.assert_array_equal(analysis_dev(ctx, x[b:b + 1], h, levels)[0], z[b], err_msg=where)
            np.testing.assert_array_equal(synthesis_dev(ctx, c[b:b + 1], h, levels)[0], w[b], err_msg=where)
    # device tensors in and out: the bits of the host-pointer call
    if "d" in marks:
        zd = sbtv.mrdwt_TI2D(sbtv.to_device(x), h, levels, ctx=ctx)
        np.testing.assert_array_equal(np.asarray(sbtv.to_host(zd)).reshape(z.shape), z, err_msg=where)
        wd = sbtv.mirdwt_TI2D(sbtv.to_device(c), h, levels, ctx=ctx)
        np.testing.assert_array_equal(np.asarray(sbtv.to_host(wd)).reshape(w.shape), w, err_msg=where)


@pytest.mark.parametrize("K", wg.KS)
def test_sweep(ctx, K):
    cases = wg.cases_of(K)
    assert cases and len(wg.marked("d", K)) == 1
    for case in cases:
        run_case(ctx, case)
    for q in ("analysis", "synthesis", "W W'x - x"):
        r, e, own, bar, at = RATIOS[(K, q)]
        print("K=%d %-10s worst device error / float64 restatement's error %.2f (margin %.0f) at %s" % (K, q, r, MARGIN, at))


# ---------------------------------------------------------------------------------------------------------------------
# 2. impulses
# ---------------------------------------------------------------------------------------------------------------------
AMPLITUDE = 37.5


def impulse_bands(levels):
    J = levels - 1
    deepest = [0] + [1 + 3 * (J - 1) + q for q in range(3)]
    return sorted(set(deepest + [1, 2, 3]))


def shifted(a, r, c, nb=1):
    """A transform of the impulse at (0, 0), (M, nb N), moved to the impulse at (r, c): the frame commutes with circular
    shifts, and the evaluator does so bit for bit (tests/test_wavelet_longdouble_cpu.py), so ONE reference per band serves
    every position."""
    M = a.shape[0]
    return np.roll(a.reshape(M, nb, -1), (r, c), axis=(0, 2)).reshape(M, -1)


def references(fn, unit, h, levels, K):
    """(long double, float64, structural support) of fn on the unit impulse."""
    return (fn(unit, h, levels), fn(unit, h, levels, np.float64), fn(unit, None, levels, np.float64, wl.ones_filters(K)) != 0)


def run_impulses(ctx, case):
    import sbtv
    (M, N), K, levels, _, _ = case
    where = "%dx%d K=%d levels=%d" % (M, N, K, levels)
    rep = reported(ctx, M, N, K, levels)
    pts = wg.impulse_points(M, N, K, levels, rep)
    assert pts == wg.impulse_points(M, N, K, levels) and len(pts) >= 2
    h = sbtv.daubcqf(K)
    nb = bands(levels)

    def compare(quantity, got, refs, nbands, tag):
        ld, f64, sup = (np.stack([shifted(a, r, c, nbands) for r, c in pts]) for a in refs)
        bad = ~sup & (got != 0)
        assert not np.any(bad), "%s: %s%s is not exactly 0 at %d positions off its support, first (impulse, row, column) %s, " \
            "impulse at %s" % (where, quantity, tag, np.count_nonzero(bad), tuple(np.argwhere(bad)[0]), pts[np.argwhere(bad)[0][0]])
        check(K, quantity, got, ld, f64, AMPLITUDE, where + tag)

    # a delta in
    unit = np.zeros((M, N))
    unit[0, 0] = AMPLITUDE
    x = np.stack([shifted(unit, r, c) for r, c in pts])
    refs = references(wl.analysis, unit, h, levels, K)
    if min(M, N) > K:
        assert not np.all(refs[2][:, N:4 * N])                                  # level 1 leaves zeros: n > K
    compare("delta in", analysis_dev(ctx, x, h, levels), refs, nb, "")
    # the transpose: one coefficient in
    for b in impulse_bands(levels):
        unit = np.zeros((M, nb * N))
        unit[0, b * N] = AMPLITUDE
        c = np.stack([shifted(unit, r, col, nb) for r, col in pts])
        compare("coefficient in", synthesis_dev(ctx, c, h, levels), references(wl.synthesis, unit, h, levels, K), 1, " band %d" % b)


@pytest.mark.parametrize("K", wg.KS)
def test_impulses(ctx, K):
    cases = wg.marked("i", K)
    assert cases
    for case in cases:
        run_impulses(ctx, case)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sbtv_soft
# ---------------------------------------------------------------------------------------------------------------------
SUBNORMAL = 5e-324 * 1000
SPECIALS = [0.0, -0.0, 1.5, -1.5, np.nextafter(1.5, 2.0), -np.nextafter(1.5, 2.0), np.nextafter(1.5, 0.0), SUBNORMAL, -SUBNORMAL,
            1e308, -1e308, np.inf, -np.inf]


def assert_soft(got, x, T):
    ref = np.stack([wr.soft(x[b], T[b]) for b in range(x.shape[0])])
    assert not np.any(np.isnan(ref))
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin], ref[~fin])
    assert np.all(np.abs(got[fin] - ref[fin]) <= np.spacing(np.abs(ref[fin])))          # 1 ulp
    zero = ref == 0
    np.testing.assert_array_equal(got[zero], ref[zero])
    np.testing.assert_array_equal(np.signbit(got[zero]), np.signbit(ref[zero]))         # the sign of a zero result


# 2048 workgroups of 256 lanes: P = 2048 * 256 + 2 sends lanes 0 and 1 of workgroup 0 through the loop a second time
@pytest.mark.parametrize("shape", [(1090, 481), (1024, 513)], ids=["P=2048*256+2", "1024x513"])
def test_soft_grid_stride_loop_iterates(ctx, shape):
    import sbtv
    M, N = shape
    assert M * N > 2048 * 256 and (shape != (1090, 481) or M * N == 2048 * 256 + 2)
    rng = np.random.default_rng(M)
    x = rng.standard_normal((2, M, N)) * 3.0
    T = np.array([1.5, 0.25])
    for b in range(2):                                   # specials at the start, around the loop's seam and at the very end
        flat = x[b].reshape(-1)
        flat[:len(SPECIALS)] = SPECIALS
        flat[-1] = -3.0 * T[b]
        flat[2048 * 256 - 2:2048 * 256 + 2] = [T[b], -T[b], -T[b], 2.0 * T[b]]
    got = np.asarray(sbtv.soft(x, T, ctx=ctx))
    assert_soft(got, x, T)
    for b in range(2):
        g, s = got[b].reshape(-1), 2048 * 256
        assert list(g[s - 2:s + 2]) == [0.0, 0.0, 0.0, T[b]] and list(np.signbit(g[s - 2:s + 2])) == [False, True, True, False]
        assert M * N == s + 2 or g[-1] == -2.0 * T[b]
        np.testing.assert_array_equal(np.asarray(sbtv.soft(x[b], T[b], ctx=ctx)), got[b])


@pytest.mark.parametrize("shape", [(1, 1), (5, 51), (16, 16), (257, 1), (1, 257)], ids=lambda s: "P=%d_%dx%d" % (s[0] * s[1], s[0], s[1]))
def test_soft_small_sizes_and_special_values(ctx, shape):
    import sbtv
    M, N = shape
    P = M * N
    rng = np.random.default_rng(P)
    T = np.array([0.0, 1.5, np.inf])
    x = rng.standard_normal((3, M, N)) * 3.0
    for b in range(3):
        sp = [v for v in SPECIALS if not (np.isinf(v) and np.isinf(T[b]))]        # inf - inf: nothing to pin
        flat = x[b].reshape(-1)
        n = min(P, len(sp))
        flat[P - n:] = sp[:n]                                                  # the specials sit at the END of the image
        if P > 2 * len(sp):
            flat[:len(sp)] = sp[::-1]
    if P == 1:
        for v in SPECIALS:
            x[:2, 0, 0] = v
            x[2, 0, 0] = v if np.isfinite(v) else 1.0
            assert_soft(np.asarray(sbtv.soft(x, T, ctx=ctx)), x, T)
    got = np.asarray(sbtv.soft(x, T, ctx=ctx))
    assert_soft(got, x, T)
    np.testing.assert_array_equal(got[0], x[0])                                 # T = 0 passes x through, -0.0 and inf included
    np.testing.assert_array_equal(np.signbit(got[0]), np.signbit(x[0]))
    assert np.all(got[2] == 0.0)                                                # T = inf leaves signed zeros
    np.testing.assert_array_equal(np.signbit(got[2]), np.signbit(x[2]))
    assert np.all(got[1][np.abs(x[1]) <= 1.5] == 0.0)


def test_soft_refuses_a_nan_threshold(ctx):
    import sbtv
    x = np.ones((2, 8, 8))
    for T in (np.array([0.5, np.nan]), np.array([np.nan, 0.5]), np.array([0.5, -1.0])):
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.soft(x, T, ctx=ctx)
        assert e.value.code == -1                                               # SBTV_ERR_BADARG
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.soft(x[0], np.nan, ctx=ctx)
    assert e.value.code == -1


# ---------------------------------------------------------------------------------------------------------------------
# 4. guard bands
# ---------------------------------------------------------------------------------------------------------------------
CANARY_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(%(root)r, "semi-blind-image-deblurring-problems-with-tv_amd"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import sbtv
import wavelet_geometry_cases as wg
ctx = sbtv.default_context(0)
assert ctx.canary()["enabled"], "SBTV_CANARY=1 was not picked up"
n = 0
for (M, N), K, levels, batch, marks in wg.marked("i"):
    h = sbtv.daubcqf(K)
    rng = np.random.default_rng([M, N, K])
    for B in (1, 3):
        x = rng.standard_normal((B, M, N))
        z = np.asarray(sbtv.mrdwt_TI2D(x, h, levels, ctx=ctx))
        back = np.asarray(sbtv.mirdwt_TI2D(z, h, levels, ctx=ctx)).reshape(x.shape)
        assert np.max(np.abs(back - x)) <= 1e-12 * np.max(np.abs(x))
        c = ctx.canary()
        assert c["enabled"] and c["buffers"] > 0 and c["bad_bytes"] == 0, ((M, N), K, levels, B, c)
        n += 1
print("canary ok:", c["buffers"], "guarded workspaces,", n, "round trips")
"""


def test_transforms_under_canary_guard_bands():
    """One child process with SBTV_CANARY=1 runs analysis and synthesis on the impulse subset (every K, every run regime, with
    and without the workspace images of a batch): every entry point ends by verifying the guard bands of all workspaces."""
    env = dict(os.environ)
    env["SBTV_CANARY"] = "1"
    r = subprocess.run([sys.executable, "-c", CANARY_CHILD % {"root": ROOT}], env=env, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
