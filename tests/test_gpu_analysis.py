"""GPU: the analysis-prior wavelet SALSA driver (sbtv_SALSA_analysis, csrc/wavelet_deconv.hip; sbtv.SALSA_analysis) against SALSA_v2.m
restated line for line in NumPy with P = W, PT = W' (tests/analysis_restatement.py, salsa_analysis_literal) on the cases of
tests/analysis_cases.py.

The bars are those tests/test_gpu_wavelet.py and tests/test_gpu_fista_l1.py use for this frame and operator: the same stopping
iteration, objective / distance / mses rtol 1e-9, max|x - ref| < 1e-7, times[0] == 0 and non-decreasing, traces n_outer + 1
long (distance n_outer), numA == 1 + n_outer, numAt == 1.  The cases whose rule fires inside the loop do so with a margin of
at least 1 % on both sides (tests/test_analysis_cpu.py), far above those bars."""
import ctypes as C

import numpy as np
import pytest

import analysis_cases as ac
import wavelet_cases as wc
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu

NAMES = ("x", "numA", "numAt", "objective", "distance", "times", "mses")


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, p["p_true"])[0])


def _solve(ctx, p, **kw):
    import sbtv
    op = _blur(p)
    args = dict(MU=p["mu"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, STOPCRITERION=p["stop"], TOLERANCEA=p["tolA"],
                MAXITERA=p["maxiter"], TRUE_X=p["x"], INITIALIZATION=p["init"], VERBOSE=0)
    args.update(kw)
    args = {k: v for k, v in args.items() if v is not None}
    return sbtv.SALSA_analysis(p["y"], op, p["tau"], ctx=ctx, **args)


def _check(got, ref):
    x, numA, numAt, objective, distance, times, mses = got
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1))) if len(a) == len(b) and len(a) else float("nan")
    print(f"outer iterations {len(objective) - 1} / {ref['n_outer']}, max|x - ref| = {np.max(np.abs(x - ref['x'])):.2e}, worst rel: "
          f"objective {rel(objective, ref['objective']):.2e}, distance {rel(distance, ref['distance']):.2e}, "
          f"mses {rel(mses, ref['mses']):.2e}")
    n = ref["n_outer"]
    assert len(objective) == len(ref["objective"]) == n + 1, "different stopping iteration"
    assert len(times) == len(mses) == n + 1 and len(distance) == n
    assert (numA, numAt) == (ref["numA"], ref["numAt"]) == (1 + n, 1)
    np.testing.assert_allclose(objective, ref["objective"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(distance, ref["distance"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(mses, ref["mses"], rtol=1e-9, atol=0)
    assert np.max(np.abs(x - ref["x"])) < 1e-7
    assert times[0] == 0 and np.all(np.diff(times) >= 0)


def _same_bits(a, b, skip=("times",)):
    for u, v, name in zip(a, b, NAMES):
        if name not in skip:
            np.testing.assert_array_equal(u, v, err_msg=name)


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(a) rule 1 fires at 36 of 60: the lagged stop; (b) D4, rule 2 on the image, zero start; (c) rule 3 from a random start
    image, met at outer 1 already but not evaluated before outer 2; (d) 100 x 90, the chirp-z FFT path, to MAXITERA; (e) 512 x
    512: 2 621 440 coefficients, the grid-stride loop of the step kernel; (f) 16 x 18: a partly filled last workgroup; (g) D4,
    rectangular, rule 2."""
    p, ref = ac.problem(name), ac.reference(name)
    assert ref["n_outer"] == p["stops_at"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    calls = ctx.calls
    _check(got, ref)
    assert calls == ac.calls(p, ref["n_outer"])


def test_solver_without_the_lagged_stop_rule_gives_the_same_result(ctx):
    for name in ("a", "g"):
        p = ac.problem(name)
        lag, exact = _solve(ctx, p), _solve(ctx, p, SPECULATE=0)
        _same_bits(lag, exact)
        _check(exact, ac.reference(name))


def test_without_true_x_no_mses_and_the_same_iterates(ctx):
    """No pixel pass under rule 1, the pixel pass without its first sum under rule 2."""
    for name in ("f", "g"):
        p = ac.problem(name)
        with_true, got = _solve(ctx, p), _solve(ctx, p, TRUE_X=None)
        assert len(got[6]) == 0
        _same_bits(got, with_true, skip=("times", "mses"))


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = ac.problem("a")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    taps = np.stack([sbtv.psf_family("gaussian", 7, pa["p_true"])[0], sbtv.psf_family("gaussian", 7, (0.5, 0.35))[0]])
    y = np.stack([pa["y"], st2["y"]])
    tau = np.array([pa["tau"], 0.5 * st2["sigma"] ** 2])
    mu = np.array([pa["mu"], 0.1])
    tx = np.stack([pa["x"], x2])
    args = dict(WAVELET=pa["h"], LEVELS=pa["levels"], STOPCRITERION=1, TOLERANCEA=1e-4, MAXITERA=60, INITIALIZATION=2)
    opb = sbtv.BlurOperator(taps)
    both = sbtv.SALSA_analysis(y, opb, tau, MU=mu, TRUE_X=tx, AT=opb.T, ctx=ctx, **args)
    lens = []
    for b in range(2):
        op1 = sbtv.BlurOperator(taps[b])
        one = sbtv.SALSA_analysis(y[b], op1, tau[b], MU=mu[b], TRUE_X=tx[b], AT=op1.T, ctx=ctx, **args)
        np.testing.assert_array_equal(both[0][b], one[0])
        assert (both[1][b], both[2][b]) == (one[1], one[2])
        for q in (3, 4, 6):
            np.testing.assert_array_equal(both[q][b], one[q])
        assert len(both[5][b]) == len(one[5])
        lens.append(len(one[3]) - 1)
    assert lens[0] == ac.reference("a")["n_outer"]
    print("outer iterations of the two images:", lens)


def test_solver_takes_device_tensors(ctx):
    import sbtv
    for name in ("d", "c"):                                   # (c): the start image is a device tensor too
        p = ac.problem(name)
        host = _solve(ctx, p)
        dev_init = sbtv.to_device(p["init"]) if isinstance(p["init"], np.ndarray) else p["init"]
        op = _blur(p)
        dev = sbtv.SALSA_analysis(sbtv.to_device(p["y"]), op, p["tau"], "MU", p["mu"], "WAVELET", p["h"], "LEVELS", p["levels"],
                                  "AT", op.T, "STOPCRITERION", p["stop"], "TOLERANCEA", p["tolA"], "MAXITERA", p["maxiter"],
                                  "TRUE_X", sbtv.to_device(p["x"]), "INITIALIZATION", dev_init, ctx=ctx)
        _same_bits((sbtv.to_host(dev[0]),) + tuple(dev[1:]), (np.asarray(host[0]),) + tuple(host[1:]))


def test_a_threshold_above_every_coefficient_keeps_u_at_zero(ctx):
    """tau / mu above every soft argument of the run (analysis_cases.huge_tau): u is zero throughout, so every distance is
    ||W'x|| / ||W'x|| = 1 and the objective is the data term of the returned x alone."""
    p = ac.problem("f")
    tau = ac.huge_tau(p)
    got = _solve(ctx, dict(p, tau=tau), STOPCRITERION=2, TOLERANCEA=0.0, MAXITERA=6, INITIALIZATION=0)
    x, numA, numAt, objective, distance, times, mses = got
    assert len(objective) == 7 and len(distance) == 6
    print("distance - 1:", np.asarray(distance) - 1.0)
    np.testing.assert_allclose(distance, 1.0, rtol=1e-12, atol=0)
    Bx = np.real(np.fft.ifft2(p["H"] * np.fft.fft2(np.asarray(x))))
    np.testing.assert_allclose(objective[-1], 0.5 * wr._sq(p["y"] - Bx), rtol=1e-9, atol=0)
    assert objective[0] == pytest.approx(0.5 * wr._sq(p["y"]), rel=1e-12)      # the zero start


def _raw(ctx, p, **kw):
    """sbtv_SALSA_analysis through the bare binding on problem p (three iterations, criterion 1 with tolerance 0, zero start);
    keywords replace arguments, `edit` changes the options after their defaults.  Returns (code, message)."""
    from sbtv import _lib as L
    a = dict(y=p["y"], taps=_blur(p)._cm(1), taille=7, h=np.ascontiguousarray(p["h"]), levels=p["levels"], tau=np.array([p["tau"]]),
             mu=np.array([p["mu"]]), batch=1, x_out=True, handle=ctx.h, edit=None)
    a.update(kw)
    M, N = p["y"].shape if a["y"] is None else a["y"].shape
    K = 3
    so = L.sbtv_salsa_opts()
    ctx.lib.sbtv_salsa_opts_default(C.byref(so))
    so.stopcriterion, so.maxiter, so.tolA, so.initialization = 1, K, 0.0, 0
    if a["edit"]:
        a["edit"](so)
    ycm = None if a["y"] is None else np.ascontiguousarray(a["y"].T, dtype=np.float64)
    x = np.zeros(M * N)
    objective, distance, times = np.zeros(max(so.maxiter, K) + 1), np.zeros(max(so.maxiter, K)), np.zeros(max(so.maxiter, K) + 1)
    numA, numAt, nout = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    vp = lambda v: None if v is None else L.vptr(v)
    ctx.reset_calls()
    rc = ctx.lib.sbtv_SALSA_analysis(a["handle"], vp(ycm), M, N, a["batch"], vp(a["taps"]), a["taille"], vp(a["h"]),
                                     0 if a["h"] is None else a["h"].size, a["levels"], vp(a["tau"]), vp(a["mu"]), C.byref(so),
                                     None, None, vp(x) if a["x_out"] else None, vp(objective), vp(distance), vp(times), None,
                                     numA, numAt, nout, L.SBTV_HOST_PTRS)
    if rc != 0:
        assert ctx.calls == 0, "an operator ran before the refusal"
    try:
        ctx.check(rc)
    except L.SbtvError as e:
        return e.code, e.msg
    return rc, ""


def _set(**fields):
    def edit(so):
        for k, v in fields.items():
            setattr(so, k, v)
    return edit


def test_refusals(ctx):
    """Each is refused with the code and message sbtv_SALSA_wavelet gives for the same fault, before any launch."""
    p = ac.problem("f")                                                               # 16 x 18, Haar, levels 3
    BADARG, SIZE, MAXITER, STOP, INIT, MISSING_AT, PSF = -1, -2, -3, -6, -7, -8, -10
    assert _raw(ctx, p)[0] == 0
    assert _raw(ctx, p, handle=None)[0] == BADARG
    for kw in (dict(y=None), dict(h=None), dict(tau=None), dict(mu=None), dict(x_out=False), dict(batch=0),
               dict(mu=np.array([0.0])), dict(mu=np.array([-1.0])),
               dict(h=np.array([1.0, 0.25])),                                          # not orthonormal
               dict(h=np.sqrt(2.0) * np.array([0.75, 0.25])),                          # sum sqrt 2 but not of unit norm
               dict(levels=1)):
        assert _raw(ctx, p, **kw)[0] == BADARG, kw
    assert _raw(ctx, p, taps=None) == (MISSING_AT, "The function handle for transpose of A is missing")
    assert _raw(ctx, p, x_out=False) == (BADARG, "SALSA_analysis: missing required argument")
    assert _raw(ctx, p, mu=np.array([0.0])) == (BADARG, "SALSA_analysis: mu must be > 0")
    assert _raw(ctx, p, levels=5, h=wc.daub(4))[0] == SIZE                             # D4: reach 3 * 8 >= min(16, 18)
    assert _raw(ctx, p, levels=5)[0] == 0                                              # Haar: reach 8 fits
    assert _raw(ctx, p, y=np.ones((33, 35)))[0] == SIZE                                # an odd pixel count
    for stop in (0, 4):
        assert _raw(ctx, p, edit=_set(stopcriterion=stop)) == (STOP, "Unknown stopping criterion")
    assert _raw(ctx, p, edit=_set(initialization=1)) == (INIT, "Unknown 'Initialization' option")
    assert _raw(ctx, p, edit=_set(initialization=33333)) == (INIT, "Initialization = array but x_init is NULL")
    for m in (0, -1):
        assert _raw(ctx, p, edit=_set(maxiter=m)) == (MAXITER, "SALSA_analysis: maxiter must be positive")
    assert _raw(ctx, p, y=np.ones((6, 6)), levels=2) == (PSF, "Mask does not fit inside array")
    assert _raw(ctx, p, edit=_set(TViters=0))[0] == 0                                  # no TV prox here: accepted


def test_keyword_interface_refusals(ctx):
    import sbtv
    p = ac.problem("f")
    op = _blur(p)
    common = dict(MU=p["mu"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, MAXITERA=3, ctx=ctx)
    with pytest.raises(sbtv.SbtvError) as e:                              # the random start of SALSA_v2 is not offered
        sbtv.SALSA_analysis(p["y"], op, p["tau"], INITIALIZATION=1, **common)
    assert e.value.code == -7
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.SALSA_analysis(p["y"], op, p["tau"], **dict(common, MAXITERA=0))
    assert (e.value.code, e.value.msg) == (-3, "SALSA_analysis: maxiter must be positive")
    with pytest.raises(ValueError):                                       # TRUE_X is an image here, not coefficients
        sbtv.SALSA_analysis(p["y"], op, p["tau"], TRUE_X=wr.mrdwt_TI2D(p["x"], p["h"], p["levels"]), **common)
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.SALSA_analysis(p["y"], op, p["tau"], **{k: v for k, v in common.items() if k != "MU"})
    assert e.value.code == -1
