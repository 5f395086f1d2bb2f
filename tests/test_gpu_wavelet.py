"""GPU: the redundant wavelet frame (sbtv_mrdwt_TI2D / sbtv_mirdwt_TI2D, csrc/wavelet.hip), sbtv_soft and the wavelet-l1
SALSA driver (sbtv_SALSA_wavelet, csrc/wavelet_deconv.hip) against the NumPy restatement (tests/wavelet_restatement.py).

Transforms: atol 1e-12 max|x| (about 2 K J roundings of 1.1e-16 per output: under 1e-14 relative); adjoint and Parseval
identities on the device's own output to 1e-11 relative.  Solver: the bars of tests/test_gpu_admm.py and test_gpu_masked.py
against the LITERAL SALSA_v2 iteration: same stopping iteration, objective / mses rtol 1e-9, distance rtol 1e-7,
max |xw - ref| < 1e-7, max |x - W ref| < 1e-7, numA / numAt equal, times[0] == 0 and non-decreasing.  The length-6 filter
has instantiations of its own: two transform cases and one chain with moments (sbtv_myula_wavelet) launch them."""
import numpy as np
import pytest

import wavelet_cases as wc
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu

# (M, N), filter length, levels, batch
TRANSFORM_CASES = [
    ((13, 13), 4, 4, 1),          # reach 12 = size - 1: every tap wraps
    ((17, 9), 2, 4, 1),           # odd, rectangular
    ((24, 20), 4, 4, 1),          # rectangular
    ((64, 64), 8, 3, 1),          # the longest filter
    ((96, 160), 4, 4, 3),         # tile seams in both dimensions, non-square, a batch
    ((256, 192), 2, 5, 1),
    ((512, 512), 2, 4, 1),        # full launch geometry
    # strides beyond the run caps of csrc/wavelet.hip (16 / 8 / 4 rows, 4 / 2 columns by filter length): the tiles of the
    # deepest levels are combs of runs along both dimensions.  96 = 3 * 32 and 160 = 5 * 32 = 10 * 16 ARE multiples of the
    # deepest strides of the first two (every run has the same number of steps); only 150 and 131 leave the last step of a
    # comb partial, for filter lengths 6 and 8.  tests/test_gpu_wavelet_sweep.py has that class for every length.
    ((96, 160), 2, 7, 1),         # s = 32 > 16
    ((160, 96), 4, 6, 2),         # s = 16 > 8, reach 48, a batch
    ((150, 131), 8, 5, 1),        # s = 8 > 4, reach 56, odd sizes
    # filter length 6: its own instantiations and LDS footprint (runs capped at 4 rows / 2 columns, 84 rows per tile column)
    ((40, 44), 6, 4, 2),          # reach 20, tiles cut at both edges, a batch
    ((150, 131), 6, 5, 1),        # s = 8 above both caps, reach 40
]


@pytest.mark.parametrize("shape,K,levels,batch", TRANSFORM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_transforms_match_restatement_and_are_a_parseval_frame(ctx, shape, K, levels, batch):
    import sbtv
    h = sbtv.daubcqf(K)
    rng = np.random.default_rng(shape[0] * 7 + K)
    x = rng.standard_normal((batch,) + shape) * 100.0
    nb = 3 * (levels - 1) + 1
    arg = x[0] if batch == 1 else x
    z = np.asarray(sbtv.mrdwt_TI2D(arg, h, levels, ctx=ctx)).reshape(batch, shape[0], nb * shape[1])
    zr = np.stack([wr.mrdwt_TI2D(x[b], h, levels) for b in range(batch)])
    scale = np.max(np.abs(x))
    ea = np.max(np.abs(z - zr))
    c = rng.standard_normal(z.shape) * 100.0
    carg = c[0] if batch == 1 else c
    wc_ = np.asarray(sbtv.mirdwt_TI2D(carg, h, levels, ctx=ctx)).reshape(batch, *shape)
    wcr = np.stack([wr.mirdwt_TI2D(c[b], h, levels) for b in range(batch)])
    es = np.max(np.abs(wc_ - wcr))
    back = np.asarray(sbtv.mirdwt_TI2D(z[0] if batch == 1 else z, h, levels, ctx=ctx)).reshape(batch, *shape)
    er = np.max(np.abs(back - x))
    print(f"{shape} K={K} levels={levels} batch={batch}: analysis {ea / scale:.1e}, synthesis {es / np.max(np.abs(c)):.1e}, "
          f"W W'x - x {er / scale:.1e} (relative to max|x|)")
    assert ea <= 1e-12 * scale
    assert es <= 1e-12 * np.max(np.abs(c))
    assert er <= 1e-12 * scale
    for b in range(batch):                                    # on the device's own output
        lhs, rhs = float(np.vdot(z[b], c[b])), float(np.vdot(x[b], wc_[b]))
        adj = abs(lhs - rhs) / (np.linalg.norm(z[b]) * np.linalg.norm(c[b]))
        pars = abs(np.linalg.norm(z[b]) / np.linalg.norm(x[b]) - 1.0)
        print(f"  image {b}: adjoint {adj:.1e}, Parseval {pars:.1e}")
        assert adj <= 1e-11 and pars <= 1e-11


def test_transforms_take_device_tensors(ctx):
    import sbtv
    h = sbtv.daubcqf(4)
    x = np.random.default_rng(1).standard_normal((2, 48, 40))
    zd = sbtv.mrdwt_TI2D(sbtv.to_device(x), h, 3, ctx=ctx)
    zh = sbtv.mrdwt_TI2D(x, h, 3, ctx=ctx)
    np.testing.assert_array_equal(sbtv.to_host(zd), np.asarray(zh))
    xd = sbtv.mirdwt_TI2D(zd, h, 3, ctx=ctx)
    assert np.max(np.abs(sbtv.to_host(xd) - x)) <= 1e-12 * np.max(np.abs(x))


def test_soft(ctx):
    import sbtv
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 33, 21)) * 3.0
    x[0, 0, :4] = [0.0, -0.0, 1.5, -1.5]
    T = np.array([0.0, 1.5, 0.7])
    got = np.asarray(sbtv.soft(x, T, ctx=ctx))
    ref = np.stack([wr.soft(x[b], T[b]) for b in range(3)])
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))          # 1 ulp
    np.testing.assert_array_equal(got[0], x[0])                           # T = 0 passes x through
    assert np.all(got[1][np.abs(x[1]) <= 1.5] == 0.0)
    one = np.asarray(sbtv.soft(x[2], 0.7, ctx=ctx))
    np.testing.assert_array_equal(one, got[2])


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, p["p_true"])[0])


def test_refusals(ctx):
    """Each is refused with its error code before any launch."""
    import sbtv
    x = np.ones((32, 32))
    d4 = sbtv.daubcqf(4)
    for h, levels, arr, code in ((np.ones(3), 3, x, -1), (np.ones(10), 2, x, -1), (d4, 1, x, -1),
                                 (d4, 4, np.ones((12, 12)), -2), (d4, 4, np.ones((40, 12)), -2)):
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.mrdwt_TI2D(arr, h, levels, ctx=ctx)
        assert e.value.code == code, (h.size, levels, arr.shape, e.value.code)
        nb = max(3 * (levels - 1) + 1, 1)
        with pytest.raises(sbtv.SbtvError) as e:
            sbtv.mirdwt_TI2D(np.ones((arr.shape[0], nb * arr.shape[1])), h, levels, ctx=ctx)
        assert e.value.code == code
    sbtv.mrdwt_TI2D(np.ones((13, 13)), d4, 4, ctx=ctx)                    # reach 12 < 13 is accepted
    sbtv.mrdwt_TI2D(x, np.array([1.0, 0.25]), 3, ctx=ctx)                 # the bare transforms accept any h
    p = wc.problem("a")
    op = _blur(p)
    common = ("AT", op.T, "LEVELS", 4, "MAXITERA", 3)
    with pytest.raises(sbtv.SbtvError) as e:                              # a filter that is not orthonormal
        sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", p["mu"], "WAVELET", np.array([1.0, 0.25]), *common, ctx=ctx)
    assert e.value.code == -1
    with pytest.raises(sbtv.SbtvError) as e:                              # sum h = sqrt 2 but not of unit norm
        sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", p["mu"], "WAVELET", np.sqrt(2.0) * np.array([0.75, 0.25]), *common, ctx=ctx)
    assert e.value.code == -1
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", 0.0, "WAVELET", p["h"], *common, ctx=ctx)
    assert e.value.code == -1
    with pytest.raises(sbtv.SbtvError) as e:                              # an odd pixel count (the solver only: SBTV_ERR_SIZE)
        sbtv.SALSA_wavelet(np.ones((33, 35)), op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], *common, ctx=ctx)
    assert e.value.code == -2
    with pytest.raises(sbtv.SbtvError) as e:                              # the random start of SALSA_v2 is not offered
        sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], "INITIALIZATION", 1, *common, ctx=ctx)
    assert e.value.code == -7
    with pytest.raises(sbtv.SbtvError):                                   # levels far beyond any shift width
        sbtv.mrdwt_TI2D(x, d4, 80, ctx=ctx)
    # the checks SALSA_wavelet shares with the TV front-ends, through the bare binding (the keyword interface answers some of
    # them itself): code and message
    def bad_stop(so):
        so.stopcriterion = 4

    def array_start(so):
        so.initialization = 33333

    def no_iterations(so):
        so.maxiter = 0
    for edit, kw, code, text in ((bad_stop, {}, -6, "Unknown stopping criterion"),
                                 (array_start, {}, -7, "Initialization = array but xw_init is NULL"),
                                 (no_iterations, {}, -3, "SALSA_wavelet: maxiter must be positive"),
                                 (None, {"y": np.ones((6, 6))}, -10, "Mask does not fit inside array")):
        with pytest.raises(sbtv.SbtvError) as e:
            _raw_solve(ctx, p, op, edit, **kw)
        assert (e.value.code, e.value.msg) == (code, text)
    with pytest.raises(sbtv.SbtvError) as e:                              # MAXITERA 0 through the keyword interface too
        sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], "AT", op.T, "LEVELS", 4, "MAXITERA", 0, ctx=ctx)
    assert (e.value.code, e.value.msg) == (-3, "SALSA_wavelet: maxiter must be positive")

    # there is no TV prox in this solver: TViters = 0 (which the TV front-ends refuse) is accepted and changes nothing
    def no_tv(so):
        so.TViters = 0
    xw0, obj0 = _raw_solve(ctx, p, op, no_tv)
    xw5, obj5 = _raw_solve(ctx, p, op, None)
    assert obj0[0] > obj0[-1] > 0
    np.testing.assert_array_equal(obj0, obj5)
    np.testing.assert_array_equal(xw0, xw5)
    got = sbtv.SALSA_wavelet(p["y"], op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], "TOLERANCEA", 0.0, *common, ctx=ctx)
    np.testing.assert_array_equal(obj0, got[4])


def _raw_solve(ctx, p, op, edit, y=None):
    """sbtv_SALSA_wavelet through the bare binding on problem p (levels 4, three iterations, criterion 1 with tolerance 0):
    `edit` changes the options after their defaults.  Returns (xw as the C-ABI stores it, objective)."""
    import ctypes as C
    from sbtv import _lib as L
    y = p["y"] if y is None else y
    M, N = y.shape
    K, nbands = 3, 10
    so = L.sbtv_salsa_opts()
    ctx.lib.sbtv_salsa_opts_default(C.byref(so))
    so.stopcriterion, so.maxiter, so.tolA, so.initialization = 1, K, 0.0, 0
    if edit:
        edit(so)
    ycm = np.ascontiguousarray(y.T, dtype=np.float64)
    h = np.ascontiguousarray(p["h"], dtype=np.float64)
    taps = op._cm(1)
    tau, mu = L.dvec(p["tau"], 1), L.dvec(p["mu"], 1)
    xw = np.zeros(nbands * M * N)
    objective, distance, times = np.zeros(K + 1), np.zeros(K), np.zeros(K + 1)
    numA, numAt, nout = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    ctx.check(ctx.lib.sbtv_SALSA_wavelet(ctx.h, L.vptr(ycm), M, N, 1, L.vptr(taps), op.taille, L.vptr(h), h.size, 4, tau[1], mu[1],
                                         C.byref(so), None, None, L.vptr(xw), None, L.vptr(objective), L.vptr(distance),
                                         L.vptr(times), None, numA, numAt, nout, L.SBTV_HOST_PTRS))
    assert nout[0] == K
    return xw, objective


def _solve(ctx, p, **kw):
    import sbtv
    op = _blur(p)
    args = dict(MU=p["mu"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, STOPCRITERION=p["stop"], TOLERANCEA=p["tolA"],
                MAXITERA=p["maxiter"], TRUE_X=p["true_xw"], INITIALIZATION=p["init"], VERBOSE=0)
    args.update(kw)
    return sbtv.SALSA_wavelet(p["y"], op, p["tau"], ctx=ctx, **args)


def _check(got, ref):
    xw, x, numA, numAt, objective, distance, times, mses = got
    print(f"outer iterations {len(objective) - 1} / {ref['n_outer']}, max|xw - ref| = {np.max(np.abs(xw - ref['xw'])):.2e}, "
          f"max|x - W ref| = {np.max(np.abs(x - ref['x'])):.2e}, objective rel "
          f"{np.max(np.abs(objective[:2] - ref['objective'][:2]) / ref['objective'][:2]):.2e} (first two)")
    assert len(objective) == len(ref["objective"]) == ref["n_outer"] + 1, "different stopping iteration"
    assert (numA, numAt) == (ref["numA"], ref["numAt"])
    np.testing.assert_allclose(objective, ref["objective"], rtol=1e-9)
    np.testing.assert_allclose(mses, ref["mses"], rtol=1e-9)
    assert distance.shape == ref["distance"].shape
    np.testing.assert_allclose(distance, ref["distance"], rtol=1e-7)
    assert np.max(np.abs(xw - ref["xw"])) < 1e-7
    assert np.max(np.abs(x - ref["x"])) < 1e-7
    assert times[0] == 0 and np.all(np.diff(times) >= 0) and len(times) == len(objective)


@pytest.mark.parametrize("name", sorted(wc.SOLVER_CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(a) 64 x 64 Haar, stop rule 1 firing inside (2, 60): the rule that the host evaluates one iteration late; (b) 128 x 128
    D4, rule 2, zero start; (c) 128 x 128 Haar, levels 3, rule 3, a random coefficient start; (d) 100 x 90: the chirp-z FFT
    path; (e) 1024 x 1024: the pipelined row kernel."""
    p, ref = wc.problem(name), wc.reference(name)
    if name == "a":
        assert 2 < ref["n_outer"] < p["maxiter"], ref["n_outer"]
    else:
        assert ref["n_outer"] == p["maxiter"]
    _check(_solve(ctx, p), ref)


def test_solver_without_the_lagged_stop_rule_gives_the_same_result(ctx):
    p = wc.problem("a")
    lag, exact = _solve(ctx, p), _solve(ctx, p, SPECULATE=0)
    for a, b, name in zip(lag, exact, ("xw", "x", "numA", "numAt", "objective", "distance", "times", "mses")):
        if name != "times":
            np.testing.assert_array_equal(a, b, err_msg=name)
    _check(exact, wc.reference("a"))


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = wc.problem("a")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    op = _blur(pa)
    y = np.stack([pa["y"], st2["y"]])
    tau = np.array([pa["tau"], 0.5 * st2["sigma"] ** 2])
    mu = np.array([pa["mu"], 0.1])
    tx = np.stack([pa["true_xw"], wr.mrdwt_TI2D(x2, pa["h"], pa["levels"])])
    args = ("WAVELET", pa["h"], "LEVELS", pa["levels"], "AT", op.T, "STOPCRITERION", 1, "TOLERANCEA", 1e-4, "MAXITERA", 40,
            "INITIALIZATION", 2)
    both = sbtv.SALSA_wavelet(y, op, tau, "MU", mu, "TRUE_X", tx, *args, ctx=ctx)
    for b in range(2):
        one = sbtv.SALSA_wavelet(y[b], op, tau[b], "MU", mu[b], "TRUE_X", tx[b], *args, ctx=ctx)
        np.testing.assert_array_equal(both[0][b], one[0])
        np.testing.assert_array_equal(both[1][b], one[1])
        assert (both[2][b], both[3][b]) == (one[2], one[3])
        for q in (4, 5, 7):
            np.testing.assert_array_equal(both[q][b], one[q])


def test_solver_takes_device_tensors(ctx):
    import sbtv
    p = wc.problem("d")
    op = _blur(p)
    host = _solve(ctx, p)
    dev = sbtv.SALSA_wavelet(sbtv.to_device(p["y"]), op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], "LEVELS", p["levels"],
                             "AT", op.T, "STOPCRITERION", p["stop"], "TOLERANCEA", p["tolA"], "MAXITERA", p["maxiter"],
                             "TRUE_X", sbtv.to_device(p["true_xw"]), "INITIALIZATION", 2, ctx=ctx)
    np.testing.assert_array_equal(sbtv.to_host(dev[0]), np.asarray(host[0]))
    np.testing.assert_array_equal(sbtv.to_host(dev[1]), np.asarray(host[1]))
    np.testing.assert_array_equal(dev[4], host[4])


def test_filter_length_6_chain_and_moments_match_the_restatement(ctx):
    """sbtv.myula_wavelet with the length-6 filter at 40 x 44, levels 4, four samples with the image and coefficient moments:
    wav_synthesis_moments_kernel<6> next to the plain length-6 kernels, against tests/wavelet_myula_restatement.py at the bars
    of tests/test_gpu_wavelet_posterior.py (traces rtol 1e-9, last sample 1e-9 max|X|, _assert_moments)."""
    import sbtv
    import wavelet_myula_restatement as wmr
    import wavelet_sapg_cases as wsc
    from test_gpu_posterior import _assert_moments
    M, N, levels, S, theta = 40, 44, 4, 4, 0.03
    h = sbtv.daubcqf(6)
    y, sigma, H = wsc._setup(wc.synth_image(M, N, 4), 7, 3)
    op = wsc.options(sigma, S, 0)
    nz = np.random.default_rng(26).standard_normal((S - 1, M, wsc.bands(levels) * N))
    ref = wmr.myula_wavelet_chain(y, H, h, levels, op, theta, op["sigma2"], nz)
    A = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, wc.PSF_PARAMS)[0])
    r = sbtv.myula_wavelet(y, A, h, levels, op, theta=theta, sigma2=op["sigma2"], noise=nz,
                           posterior=dict(coefficients=True), ctx=ctx)
    for k, c in (("gXTrace", ref["gx"]), ("logPiTraceX", ref["logpi"])):
        a = np.asarray(r[k])
        assert a.shape == c.shape == (S,)
        print(f"{k}: worst rel {np.max(np.abs(a / c - 1)):.1e}")
        np.testing.assert_allclose(a, c, rtol=1e-9, atol=0, err_msg=k)
    xs = float(np.max(np.abs(ref["samples"][-1])))
    ex = float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - ref["samples"][-1])))
    print(f"max|X - ref| / max|X| = {ex / xs:.1e}, n = {r['posteriorcount']}")
    assert ex <= 1e-9 * xs
    assert r["posteriorcount"] == S
    _assert_moments(r["posteriormean"], r["posteriorvar"], *wmr.two_pass(ref["images"]))
    _assert_moments(r["coefmean"], r["coefvar"], *wmr.two_pass(ref["samples"]))
