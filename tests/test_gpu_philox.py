"""GPU: the device generator philox_normal_pair (csrc/sbtv_internal.h) at each of its four call sites (the wavelet step kernel
through both of its instantiations and from each of its three drivers) against the NumPy restatement
tests/philox_restatement.py, which tests/test_philox_cpu.py anchors to the known answers of Philox4x32-10.  The contract of
include/sbtv.h: pair q of chain b in step s draws counter (q, s, chain_offset + b) with key seed, and fills doubles
2q, 2q + 1 of the chain's state.

(a), (b) One step with the generator and the same step with injected zeros give the normals back:
Z = (X_philox - X_zero) / sqrt(2 gamma).  The noise term is the last addition of every step expression and 0 * sqrt(2 gamma)
adds nothing, so with eps = 2^-52 the recovery is off by at most eps max|X| / sqrt(2 gamma) + 3 eps |z| (the rounding of the
sum, of the product, of the difference and of the quotient), and NumPy's log / sin / cos differ from the device's log /
sincospi by a few ulp of r.  The bar, element by element:
    |Z - Z_ref| <= eps (2 max|X| / sqrt(2 gamma) + 64 (1 + |Z_ref|))
A wrong counter word is off by O(1) on almost every element.  Worst ratio to the bar measured on the MI355X:
    fused epilogue 1024 x 2048 and 2048 x 1024          0.161
    myula_step_kernel 64 x 32 / 100 x 90                0.179 / 0.170
    myula_plain_kernel 64 x 32                          0.103
    wav_step_kernel (csrc/wavelet_chain.hip; measured on the three kernels it replaced):
      SAPG_wavelet 34 x 30 / 512 x 256                  0.139 / 0.112
      myula_wavelet, <false> / <true> (moments)         0.139 / 0.139
      SAPG_wavelet_semiblind, all fixed / sigma2 free   0.139 / 0.141
    seed = 5 / chain_offset = 0                         0.139 / 0.141
no element over the bar in any case.

(c) Chains of several steps: the chain that draws from the generator against the SAME entry fed chain_normals(...) as injected
noise, at the entry's own bars (traces rtol 1e-9, last sample 1e-9 max|X|; TV thetas / sigmas rtol 1e-9).  That pins the step
counter over the iterations and from the warm-up into the main loop.  The two chains differ by the few ulp between the device's
and NumPy's normals; how far a chain moves under a 1e-12 RELATIVE perturbation of all its normals, measured on the CPU with
the restatements / the oracle driven by the restated normals (worst relative change of a trace | of the last sample):
    SAPG_wavelet case a, warmup 4 + 12 samples          1.0e-14 | 4.9e-14
    SAPG_wavelet_semiblind case A, sigma2 free, 4 + 12  6.8e-14 (grads; others <= 2.7e-15) | 5.4e-14
    SAPG_algorithm_Guassian 64 x 32, 3 + 6              5.3e-15 | 4.5e-14   (the Chambolle early stop does not flip)
    sbtv.myula 64 x 32, 8 samples                       last sample 4.0e-14 (9.3e-12 absolute)
    myula_wavelet 8 x 8, 2 100 samples                  gx 1.0e-14, logpi 6.4e-14
all four orders of magnitude under the bars, so none of the chains had to be shortened.  The long chain is held against the
restatement itself (tests/wavelet_myula_restatement.py): its ring of 1024 trace slots fills twice, slot 0 reads gx written by
an earlier launch, and the step counter reaches 2098.  Measured on the MI355X: generator chain against injected chain, traces
within 8.9e-16 and last samples within 5.1e-16 max|X| (sbtv.myula 2.6e-13 absolute); long chain against the restatement, gx
1.1e-15, logpi 3.8e-14 (9.5e-15 at the ring seams), last sample 8.8e-15 max|X|.

Not tested: q >= 2^32 (more than 2^33 doubles per chain) cannot be reached at a testable size."""
import functools
import math

import numpy as np
import pytest

from conftest import synth_image
from test_gpu_sapg_fista import _op_struct

import philox_restatement as pr
import wavelet_cases as wc
import wavelet_myula_restatement as wmr
import wavelet_posterior_cases as wpc
import wavelet_sapg_cases as wsc
import wavelet_sb_cases as wbc

pytestmark = pytest.mark.gpu

SEED, OFFSET, BATCH = (7 << 32) | 5, 3, 2
EPS = 2.0 ** -52


def _assert_normals(label, Xp, X0, gamma, seed=SEED, offset=OFFSET, step=0):
    """Xp, X0: (B, M, C) states after ONE step with the generator / with zero noise.  Returns the recovered normals in device
    order (B, M C)."""
    Xp, X0 = np.asarray(Xp, dtype=np.float64), np.asarray(X0, dtype=np.float64)
    assert Xp.shape == X0.shape and Xp.ndim == 3
    B, M, C = Xp.shape
    sq2g = math.sqrt(2 * gamma)
    Z = pr.device_order((Xp - X0) / sq2g)
    Zref = pr.chain_normals(M * C, [step], B, seed, offset)[0]
    xmax = max(float(np.max(np.abs(Xp))), float(np.max(np.abs(X0))))
    bound = EPS * (2 * xmax / sq2g + 64 * (1 + np.abs(Zref)))
    ratio = np.abs(Z - Zref) / bound
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{label}: {Z.size} normals, worst |Z - Z_ref| / bound = {ratio.max():.3g} at chain {worst[0]} double {worst[1]} "
          f"(max|X| = {xmax:.4g}, sqrt(2 gamma) = {sq2g:.4g}, {np.mean(ratio > 1):.3%} over)")
    assert np.all(ratio <= 1.0), label
    return Z


# ---- the TV entries ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tv_problem(M, N, offset):
    """Two images of one call: synth_image (+ offset, which keeps abs() of the step inactive) and its row flip."""
    import sbtv_oracle as o
    x = offset + synth_image(M, N, 12)
    st = o.demo_setup("gaussian", x, np.zeros((M, N)) if offset else np.random.default_rng(4).standard_normal((M, N)), evMax=0.99)
    return st, np.stack([st["y"], st["y"][::-1].copy()])


def _tv_sapg(st, y, samples, warmup, burnIn, noise=None, seed=SEED, offset=OFFSET):
    import sbtv
    op, c, _ = _op_struct("gaussian", st, samples, warmup, burnIn)
    op.update(seed=seed, chain_offset=offset)
    return sbtv.SAPG_algorithm_Guassian(y, op, c, noise=noise)[-1]


@pytest.mark.parametrize("shape", [(1024, 2048), (2048, 1024), (64, 32), (100, 90)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_step_normals_tv_sapg(ctx, shape):
    """1024 x 2048 and 2048 x 1024: the MYULA epilogue of the inverse column pass (csrc/fft_wave.inc, sides of 1024 / 2048 only;
    q = j M / 2 + e in column j, which a square image cannot tell from j N / 2 + e).  64 x 32 (a power of two off the wave
    path) and 100 x 90 (chirp-z): myula_step_kernel."""
    M, N = shape
    st, y = _tv_problem(M, N, 100.0)
    Xp = np.stack([np.asarray(r["Xlast_sample"]) for r in _tv_sapg(st, y, 2, 0, 1)])
    X0 = np.stack([np.asarray(r["Xlast_sample"]) for r in _tv_sapg(st, y, 2, 0, 1, noise=np.zeros((1, BATCH, M, N)))])
    assert Xp.min() > 50.0 and X0.min() > 50.0                    # abs() of the step is inactive
    _assert_normals(f"SAPG_algorithm_Guassian {M}x{N}", Xp, X0, st["gamma"])


@functools.lru_cache(maxsize=None)
def _plain_myula_op(samples):
    import sbtv
    st, y = _tv_problem(64, 32, 0.0)
    A = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, st["p_true"])[0])
    op = dict(y=y, samples=samples, theta_op=0.02, gamma=st["gamma"], A=A, sigma2=st["sigma"] ** 2, chambolleit=25, seed=SEED,
              chain_offset=OFFSET)
    op["lambda"] = st["lam"]
    return op


def test_one_step_normals_plain_myula(ctx):
    """myula_plain_kernel: sbtv.myula with samples = 3 makes one step (iterations 2 .. samples - 1)."""
    import sbtv
    op = _plain_myula_op(3)
    Xp = np.asarray(sbtv.myula(op))
    X0 = np.asarray(sbtv.myula(op, noise=np.zeros((1, BATCH, 64, 32))))
    _assert_normals("myula 64x32", Xp, X0, op["gamma"])


# ---- the wavelet entries ----------------------------------------------------------------------------------------------
def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", p["psf_size"], wc.PSF_PARAMS)[0])


def _two(y):
    """(1, M, N) -> two images of one call: y and its row flip."""
    return np.stack([y[0], y[0][::-1].copy()])


def _last(results):
    return np.stack([np.asarray(r["Xlast_sample"]) for r in results])


def _zeros(p, y, steps=1):
    return np.zeros((steps, y.shape[0], y.shape[1], wsc.bands(p["levels"]) * y.shape[2]))


def _sapg_wavelet(ctx, p, y, noise=None, seed=SEED, offset=OFFSET, **opkw):
    import sbtv
    op = dict(p["op"], seed=seed, chain_offset=offset, **opkw)
    return sbtv.SAPG_wavelet(y, _blur(p), p["h"], p["levels"], op, noise=noise, ctx=ctx)[1]


@pytest.mark.parametrize("name", ["34x30", "512x256"])
def test_one_step_normals_sapg_wavelet(ctx, name):
    """wav_step_kernel<false> with theta and sigma2 read from the chain block of SAPG_wavelet.  34 x 30 Haar levels 3: 7140
    coefficients per chain, the last workgroup part full.  512 x 256 Haar levels 4: 655 360 pairs per chain against 2048
    workgroups of 256 lanes, the grid-stride loop."""
    p = wsc.problem("c") if name == "34x30" else wpc.problem("e")
    assert (p["y"].shape[1:], p["levels"]) == {"34x30": ((34, 30), 3), "512x256": ((512, 256), 4)}[name]
    y = _two(p["y"])
    kw = dict(samples=2, warmup=0, burnIn=2)
    Xp = _last(_sapg_wavelet(ctx, p, y, **kw))
    X0 = _last(_sapg_wavelet(ctx, p, y, noise=_zeros(p, y), **kw))
    _assert_normals(f"SAPG_wavelet {name}", Xp, X0, p["op"]["gamma"])


def _myula_wavelet(ctx, p, y, samples, noise=None, posterior=None, theta=0.03, seed=SEED, offset=OFFSET):
    import sbtv
    op = dict(p["op"], samples=samples, seed=seed, chain_offset=offset)
    return sbtv.myula_wavelet(y, _blur(p), p["h"], p["levels"], op, theta=theta, sigma2=p["op"]["sigma2"], noise=noise,
                              posterior=posterior, ctx=ctx)


@pytest.mark.parametrize("coefficients", [False, True], ids=["fixed", "moments"])
def test_one_step_normals_myula_wavelet(ctx, coefficients):
    """wav_step_kernel<false> with theta and sigma2 read from myula_wavelet's parameter array, and wav_step_kernel<true> with
    the coefficient moments requested, 34 x 30."""
    p = wsc.problem("c")
    y = _two(p["y"])
    post = dict(coefficients=True) if coefficients else None
    Xp = _last(_myula_wavelet(ctx, p, y, 2, posterior=post))
    X0 = _last(_myula_wavelet(ctx, p, y, 2, noise=_zeros(p, y), posterior=post))
    _assert_normals(f"myula_wavelet 34x30 coefficients={coefficients}", Xp, X0, p["op"]["gamma"])


def _semiblind(ctx, p, y, noise=None, seed=SEED, offset=OFFSET, **opkw):
    import sbtv
    op = dict(p["ops"][0], seed=seed, chain_offset=offset, **opkw)
    return sbtv.SAPG_wavelet_semiblind(y, p["kind"], p["h"], p["levels"], op, noise=noise, ctx=ctx)[1]


def _sigma_free(op):
    return dict(fix_sigma=False, sigma2=(op["sigma2_min"] + op["sigma2_max"]) / 2)


@pytest.mark.parametrize("free", [False, True], ids=["all-fixed", "sigma2-free"])
def test_one_step_normals_semiblind(ctx, free):
    """wav_step_kernel<false> with theta and sigma2 read from the chain block of SAPG_wavelet_semiblind, case D (34 x 30
    Moffat): every parameter fixed, and alpha and sigma2 free (sigma2(1) the midpoint of its bounds)."""
    p = wbc.problem("D")
    op0 = p["ops"][0]
    y = _two(p["y"])
    kw = dict(samples=2, warmup=0, burnIn=2)
    kw.update(_sigma_free(op0) if free else dict(fix_p=(True, True), p_init=op0["p_true"], fix_sigma=True))
    Xp = _last(_semiblind(ctx, p, y, **kw))
    X0 = _last(_semiblind(ctx, p, y, noise=_zeros(p, y), **kw))
    _assert_normals(f"SAPG_wavelet_semiblind 34x30 sigma2 free={free}", Xp, X0, op0["gamma"])


# ---- (b) seed and chain coverage --------------------------------------------------------------------------------------
def test_seed_high_word_and_chain_offset_zero(ctx):
    """The 34 x 30 case of SAPG_wavelet at seed = 5 (the low word of (7 << 32) | 5 alone) and at chain_offset = 0: each draws
    the restatement's normals for its own key / chains, and neither draws those of the other."""
    p = wsc.problem("c")
    y = _two(p["y"])
    kw = dict(samples=2, warmup=0, burnIn=2)
    X0 = _last(_sapg_wavelet(ctx, p, y, noise=_zeros(p, y), **kw))
    g = p["op"]["gamma"]
    Z = _assert_normals("seed (7<<32)|5, offset 3", _last(_sapg_wavelet(ctx, p, y, **kw)), X0, g)
    Z5 = _assert_normals("seed 5, offset 3", _last(_sapg_wavelet(ctx, p, y, seed=5, **kw)), X0, g, seed=5)
    Z0 = _assert_normals("seed (7<<32)|5, offset 0", _last(_sapg_wavelet(ctx, p, y, offset=0, **kw)), X0, g, offset=0)
    assert np.mean(np.abs(Z5 - Z) > 1e-3) > 0.99
    assert np.mean(np.abs(Z0 - Z) > 1e-3) > 0.99
    assert np.mean(np.abs(Z0[1] - Z0[0]) > 1e-3) > 0.99             # chains 0 and 1 of one call


# ---- (c) several steps ------------------------------------------------------------------------------------------------
def _assert_same_chain(label, got, ref, traces):
    for b, (r, rr) in enumerate(zip(got, ref)):
        for k in traces:
            a, c = np.asarray(r[k], dtype=np.float64), np.asarray(rr[k], dtype=np.float64)
            assert a.shape == c.shape and a.size, (k, a.shape, c.shape)
            fin = np.isfinite(c)
            np.testing.assert_array_equal(np.isfinite(a), fin, err_msg=k)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(c[fin] != 0, np.abs(a[fin] / c[fin] - 1), np.abs(a[fin]))
            print(f"{label} chain {b} {k}: {a.size} entries, worst rel {rel.max() if rel.size else 0:.1e}")
            np.testing.assert_allclose(a[fin], c[fin], rtol=1e-9, atol=0, err_msg=f"{label} chain {b} {k}")
        xa, xc = np.asarray(r["Xlast_sample"]), np.asarray(rr["Xlast_sample"])
        ex, xs = float(np.max(np.abs(xa - xc))), float(np.max(np.abs(xc)))
        print(f"{label} chain {b}: max|X - ref| / max|X| = {ex / xs:.1e}")
        assert ex <= 1e-9 * xs, (label, b)


def _restated_noise(M, C, steps, seed=SEED, offset=OFFSET):
    """(steps, BATCH, M, C) arrays for a binding's noise= argument: the normals the generator draws in steps 0 .. steps-1."""
    return pr.as_arrays(pr.chain_normals(M * C, steps, BATCH, seed, offset), M)


def test_chain_sapg_wavelet_is_the_injected_chain_with_restated_normals(ctx):
    """SAPG_wavelet case a (64 x 64 Haar levels 4), warmup 4 + 12 samples: steps 0..2 in the warm-up, 3..13 in the main loop."""
    p = wsc.problem("a")
    y = _two(p["y"])
    kw = dict(warmup=4, samples=12, burnIn=12)
    nz = _restated_noise(y.shape[1], wsc.bands(p["levels"]) * y.shape[2], 3 + 11)
    got, ref = _sapg_wavelet(ctx, p, y, **kw), _sapg_wavelet(ctx, p, y, noise=nz, **kw)
    assert len(set(ref[0]["thetas"].tolist())) > 6                                  # theta moves
    _assert_same_chain("SAPG_wavelet", got, ref, ("thetas", "gXTrace", "logPiTraceX", "logPiTrace_WU"))


def test_chain_semiblind_is_the_injected_chain_with_restated_normals(ctx):
    """SAPG_wavelet_semiblind on case A's problem (64 x 64 Haar, Laplace, b free) with sigma2 free, warmup 4 + 12 samples."""
    p = wbc.problem("A")
    y = _two(p["y"])
    kw = dict(warmup=4, samples=12, burnIn=12, **_sigma_free(p["ops"][0]))
    nz = _restated_noise(y.shape[1], wsc.bands(p["levels"]) * y.shape[2], 3 + 11)
    got, ref = _semiblind(ctx, p, y, **kw), _semiblind(ctx, p, y, noise=nz, **kw)
    assert ref[0]["sigmas"][1] != ref[0]["sigmas"][0] and ref[0]["ps"][0, 1] != ref[0]["ps"][0, 0]   # both move
    _assert_same_chain("SAPG_wavelet_semiblind", got, ref,
                       ("thetas", "ps", "sigmas", "grads", "gXTrace", "logPiTraceX", "logPiTrace_WU"))


def test_chain_tv_sapg_is_the_injected_chain_with_restated_normals(ctx):
    """SAPG_algorithm_Guassian 64 x 32, warmup 3 + 6 samples: steps 0, 1 in the warm-up, 2..6 in the main loop."""
    st, y = _tv_problem(64, 32, 0.0)
    nz = _restated_noise(64, 32, 2 + 5)
    got, ref = _tv_sapg(st, y, 6, 3, 4), _tv_sapg(st, y, 6, 3, 4, noise=nz)
    assert len(set(ref[0]["thetas"].tolist())) > 3
    _assert_same_chain("SAPG_algorithm_Guassian", got, ref, ("thetas", "sigmas", "logPiTraceX", "logPiTrace_WU"))


def test_chain_plain_myula_is_the_injected_chain_with_restated_normals(ctx):
    """sbtv.myula 64 x 32, 8 samples: six steps; the last sample at the bar of test_plain_myula_chain_matches_oracle."""
    import sbtv
    op = _plain_myula_op(8)
    got = np.asarray(sbtv.myula(op))
    ref = np.asarray(sbtv.myula(op, noise=_restated_noise(64, 32, 6)))
    print(f"myula: max|X - ref| = {np.max(np.abs(got - ref)):.2e}, max|X| = {np.max(np.abs(ref)):.4g}")
    assert np.max(np.abs(ref[0] - ref[1])) > 1e-3
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9)


LONG_SAMPLES = 2100


@functools.lru_cache(maxsize=None)
def _long_problem():
    """8 x 8 Haar levels 3, built as tests/wavelet_posterior_cases.py builds its own cases, two images."""
    ys, sigma, H = [], None, None
    for b in range(BATCH):
        y, s, H = wsc._setup(synth_image(8, 8, 4 + 5 * b), 7, 3 + 3 * b)
        ys.append(y)
        sigma = s if sigma is None else sigma
    return dict(y=np.stack(ys), H=H, h=wc.daub(2), levels=3, op=wsc.options(sigma, LONG_SAMPLES, 0), psf_size=7)


@functools.lru_cache(maxsize=None)
def _long_reference():
    """The restatement's chains on the restated normals of steps 0 .. 2098 (computed once)."""
    p = _long_problem()
    nz = _restated_noise(8, wsc.bands(3) * 8, LONG_SAMPLES - 1)
    return [wmr.myula_wavelet_chain(p["y"][b], p["H"], p["h"], 3, p["op"], 0.03, p["op"]["sigma2"], nz[:, b])
            for b in range(BATCH)]


def test_long_myula_wavelet_chain_across_the_trace_ring(ctx):
    """myula_wavelet, 2 100 samples at theta = 0.03 with the generator against the restatement on the restated normals: gx and
    logpi of all 2 100 iterations to rtol 1e-9, the seams of the 1024-slot ring (iterations 1024..1027 and 2048..2051, indices
    1023..1026 and 2047..2050) by name, and the last sample."""
    p, ref = _long_problem(), _long_reference()
    got = _myula_wavelet(ctx, p, p["y"], LONG_SAMPLES)
    for b in range(BATCH):
        for k, kr in (("gXTrace", "gx"), ("logPiTraceX", "logpi")):
            a, c = np.asarray(got[b][k]), ref[b][kr]
            assert a.shape == c.shape == (LONG_SAMPLES,)
            rel = np.abs(a / c - 1)
            print(f"chain {b} {k}: worst rel {rel.max():.1e} at index {int(np.argmax(rel))}; at the seams "
                  f"{rel[1023:1027].max():.1e}, {rel[2047:2051].max():.1e}")
            for i in (1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050):
                assert abs(a[i] - c[i]) <= 1e-9 * abs(c[i]), (b, k, i, a[i], c[i])
            np.testing.assert_allclose(a, c, rtol=1e-9, atol=0, err_msg=f"chain {b} {k}")
        xl = ref[b]["samples"][-1]
        ex = float(np.max(np.abs(np.asarray(got[b]["Xlast_sample"]) - xl)))
        print(f"chain {b}: max|X - ref| / max|X| = {ex / np.max(np.abs(xl)):.1e}")
        assert ex <= 1e-9 * np.max(np.abs(xl))
