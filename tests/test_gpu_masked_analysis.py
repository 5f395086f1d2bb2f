"""GPU: the masked-observation wavelet SALSA driver (sbtv_SALSA_masked_analysis, csrc/masked_wavelet.hip;
sbtv.SALSA_masked_analysis) against its iteration restated line for line in NumPy (tests/masked_analysis_restatement.py,
salsa_masked_analysis_literal) on the cases of tests/masked_analysis_cases.py.

The bars are those of tests/test_gpu_analysis.py and tests/test_gpu_masked.py: the same stopping iteration, objective / mses
rtol 1e-9, distance (both columns) rtol 1e-7, max|x - ref| < 1e-7, times[0] == 0 and non-decreasing, traces n_outer + 1 long
(distance (n_outer, 2)), numA, numAt and the call counter those of the restatement.  The cases whose rule fires inside the loop
do so with a margin of at least 1 % on both sides (tests/test_masked_analysis_cpu.py), far above those bars."""
import ctypes as C

import numpy as np
import pytest

import masked_analysis_cases as mc
import wavelet_cases as wc
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu

NAMES = ("x", "numA", "numAt", "objective", "distance", "times", "mses")


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(p["taps"] if p["taps"] is not None else sbtv.psf_family("gaussian", 7, p["p_true"])[0])


def _solve(ctx, p, **kw):
    import sbtv
    op = _blur(p)
    args = dict(MU1=p["mu1"], MU2=p["mu2"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, STOPCRITERION=p["stop"],
                TOLERANCEA=p["tolA"], MAXITERA=p["maxiter"], TRUE_X=p["x"], INITIALIZATION=p["init"], VERBOSE=0)
    args.update(kw)
    args = {k: v for k, v in args.items() if v is not None}
    return sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], ctx=ctx, **args)


def _check(got, ref):
    x, numA, numAt, objective, distance, times, mses = got
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1))) if np.shape(a) == np.shape(b) and len(a) else float("nan")
    print(f"outer iterations {len(objective) - 1} / {ref['n_outer']}, max|x - ref| = {np.max(np.abs(x - ref['x'])):.2e}, worst rel: "
          f"objective {rel(objective, ref['objective']):.2e}, distance {rel(distance, ref['distance']):.2e}, "
          f"mses {rel(mses, ref['mses']):.2e}")
    n = ref["n_outer"]
    assert len(objective) == len(ref["objective"]) == n + 1, "different stopping iteration"
    assert len(times) == len(mses) == n + 1 and distance.shape == ref["distance"].shape == (n, 2)
    assert (numA, numAt) == (ref["numA"], ref["numAt"])
    np.testing.assert_allclose(objective, ref["objective"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(distance, ref["distance"], rtol=1e-7, atol=0)
    np.testing.assert_allclose(mses, ref["mses"], rtol=1e-9, atol=0)
    assert np.max(np.abs(x - ref["x"])) < 1e-7
    assert times[0] == 0 and np.all(np.diff(times) >= 0)


def _same_bits(a, b, skip=("times",)):
    for u, v, name in zip(a, b, NAMES):
        if name not in skip:
            np.testing.assert_array_equal(u, v, err_msg=name)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(a) frame mask, rule 1 fires at 18 of 60: the lagged stop; (b) D4, frame mask with 30 % holes, rule 2 on the image, zero
    start; (c) weights in [0, 2], rule 3 from a random start image; (d) 100 x 90, the chirp-z FFT path, to MAXITERA; (e) 1024 x
    1024: 1 048 576 pixels, the grid-stride loop of the pixel pass; (f) 16 x 18: a partly filled last workgroup; (g) D4,
    rectangular, a single unit tap (B = identity: inpainting with 30 % missing), rule 2."""
    p, ref = mc.problem(name), mc.reference(name)
    assert ref["n_outer"] == p["stops_at"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    calls = ctx.calls
    _check(got, ref)
    assert calls == mc.calls(p, ref["n_outer"])
    if name == "g":
        assert got[6][-1] < got[6][0]                        # the mean squared error fell


def test_solver_without_the_lagged_stop_rule_gives_the_same_result(ctx):
    for name in ("a", "g"):
        p = mc.problem(name)
        lag, exact = _solve(ctx, p), _solve(ctx, p, SPECULATE=0)
        _same_bits(lag, exact)
        _check(exact, mc.reference(name))


def test_without_true_x_no_mses_and_the_same_iterates(ctx):
    """The pixel pass without x under rule 1 (f), with x and xprev but without the true image under rule 2 (g)."""
    for name in ("f", "g"):
        p = mc.problem(name)
        with_true, got = _solve(ctx, p), _solve(ctx, p, TRUE_X=None)
        assert len(got[6]) == 0
        _same_bits(got, with_true, skip=("times", "mses"))


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = mc.problem("a")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    m2 = mc.frame_mask(x2.shape) * (np.random.default_rng(31).random(x2.shape) > 0.2)
    taps = np.stack([sbtv.psf_family("gaussian", 7, pa["p_true"])[0], sbtv.psf_family("gaussian", 7, (0.5, 0.35))[0]])
    y = np.stack([pa["y"], st2["y"] * m2])
    m = np.stack([pa["m"], m2])
    tau = np.array([pa["tau"], 0.5 * st2["sigma"] ** 2])
    mu1, mu2 = np.array([pa["mu1"], 0.1]), np.array([pa["mu2"], 1.0])
    tx = np.stack([pa["x"], x2])
    args = dict(WAVELET=pa["h"], LEVELS=pa["levels"], STOPCRITERION=1, TOLERANCEA=1e-4, MAXITERA=60, INITIALIZATION=2)
    opb = sbtv.BlurOperator(taps)
    both = sbtv.SALSA_masked_analysis(y, opb, m, tau, MU1=mu1, MU2=mu2, TRUE_X=tx, AT=opb.T, ctx=ctx, **args)
    lens = []
    for b in range(2):
        op1 = sbtv.BlurOperator(taps[b])
        one = sbtv.SALSA_masked_analysis(y[b], op1, m[b], tau[b], MU1=mu1[b], MU2=mu2[b], TRUE_X=tx[b], AT=op1.T, ctx=ctx, **args)
        np.testing.assert_array_equal(both[0][b], one[0])
        assert (both[1][b], both[2][b]) == (one[1], one[2])
        for q in (3, 4, 6):
            np.testing.assert_array_equal(both[q][b], one[q])
        assert len(both[5][b]) == len(one[5])
        lens.append(len(one[3]) - 1)
    assert lens[0] == mc.reference("a")["n_outer"]
    print("outer iterations of the two images:", lens)


def test_solver_takes_device_tensors(ctx):
    import sbtv
    for name in ("d", "c"):                                   # (c): the start image is a device tensor too
        p = mc.problem(name)
        host = _solve(ctx, p)
        dev_init = sbtv.to_device(p["init"]) if isinstance(p["init"], np.ndarray) else p["init"]
        op = _blur(p)
        dev = sbtv.SALSA_masked_analysis(sbtv.to_device(p["y"]), op, sbtv.to_device(p["m"]), p["tau"], "MU1", p["mu1"], "MU2",
                                         p["mu2"], "WAVELET", p["h"], "LEVELS", p["levels"], "AT", op.T, "STOPCRITERION",
                                         p["stop"], "TOLERANCEA", p["tolA"], "MAXITERA", p["maxiter"], "TRUE_X",
                                         sbtv.to_device(p["x"]), "INITIALIZATION", dev_init, ctx=ctx)
        _same_bits((sbtv.to_host(dev[0]),) + tuple(dev[1:]), (np.asarray(host[0]),) + tuple(host[1:]))


def test_what_lies_under_a_zero_of_the_mask_does_not_matter(ctx):
    """y enters only as m .* y: other finite values under m = 0 leave every output bit-identical."""
    p = mc.problem("b")
    y2 = np.where(p["m"] == 0, 1e3, p["y"])
    assert np.any(y2 != p["y"])
    _same_bits(_solve(ctx, dict(p, y=y2)), _solve(ctx, p))


def test_masked_beats_the_periodic_solver_on_an_observation_without_wrapped_pixels(ctx):
    """The property the entry exists for (masked_analysis_cases.property_problem): PSNR over the observed pixels, SALSA_masked_analysis
    on embed_observation(y_obs, 7) against SALSA_analysis on y_obs.  The NumPy restatements score 25.06 against 21.02 dB in 87 and
    81 iterations (tests/test_masked_analysis_cpu.py asserts the same bar on them); the bar is +2 dB."""
    import sbtv
    q = mc.property_problem()
    t = mc.TAILLE
    op = sbtv.BlurOperator(sbtv.psf_family("gaussian", t, q["p_true"])[0])
    common = dict(WAVELET=q["h"], LEVELS=q["levels"], AT=op.T, STOPCRITERION=q["stop"], TOLERANCEA=q["tolA"], MAXITERA=q["maxiter"],
                  INITIALIZATION=0, VERBOSE=0, ctx=ctx)
    xp, _, _, objp, *_ = sbtv.SALSA_analysis(q["y_obs"], op, q["tau"], MU=q["mu1"], **common)
    y, m = sbtv.embed_observation(q["y_obs"], t)
    np.testing.assert_array_equal(y, q["y"])
    np.testing.assert_array_equal(m, q["m"])
    xm, _, _, objm, *_ = sbtv.SALSA_masked_analysis(y, op, m, q["tau"], MU1=q["mu1"], MU2=q["mu2"], **common)
    obs = q["scene"][t - 1:, t - 1:]
    p_per = mc.psnr_over(np.ones_like(obs), obs, xp)
    p_msk = mc.psnr_over(m, q["scene"], xm)
    print(f"periodic {p_per:.2f} dB ({len(objp) - 1} outer iterations), masked {p_msk:.2f} dB ({len(objm) - 1} outer iterations)")
    assert p_msk >= p_per + 2.0


def _raw(ctx, p, **kw):
    """sbtv_SALSA_masked_analysis through the bare binding on problem p (three iterations, criterion 1 with tolerance 0, zero
    start); keywords replace arguments, `edit` changes the options after their defaults.  Returns (code, message)."""
    from sbtv import _lib as L
    a = dict(y=p["y"], mask=p["m"], taps=_blur(p)._cm(1), taille=7, h=np.ascontiguousarray(p["h"]), levels=p["levels"],
             tau=np.array([p["tau"]]), mu1=np.array([p["mu1"]]), mu2=np.array([p["mu2"]]), batch=1, x_out=True, handle=ctx.h,
             edit=None)
    a.update(kw)
    M, N = p["y"].shape if a["y"] is None else a["y"].shape
    if a["mask"] is not None and a["mask"].shape != (M, N):
        a["mask"] = np.ones((M, N))
    K = 3
    so = L.sbtv_salsa_opts()
    ctx.lib.sbtv_salsa_opts_default(C.byref(so))
    so.stopcriterion, so.maxiter, so.tolA, so.initialization = 1, K, 0.0, 0
    if a["edit"]:
        a["edit"](so)
    cm = lambda v: None if v is None else np.ascontiguousarray(v.T, dtype=np.float64)
    ycm, mcm = cm(a["y"]), cm(a["mask"])
    x = np.zeros(M * N)
    objective, distance, times = np.zeros(max(so.maxiter, K) + 1), np.zeros(2 * max(so.maxiter, K)), np.zeros(max(so.maxiter, K) + 1)
    numA, numAt, nout = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    vp = lambda v: None if v is None else L.vptr(v)
    ctx.reset_calls()
    rc = ctx.lib.sbtv_SALSA_masked_analysis(a["handle"], vp(ycm), vp(mcm), M, N, a["batch"], vp(a["taps"]), a["taille"], vp(a["h"]),
                                            0 if a["h"] is None else a["h"].size, a["levels"], vp(a["tau"]), vp(a["mu1"]),
                                            vp(a["mu2"]), C.byref(so), None, None, vp(x) if a["x_out"] else None, vp(objective),
                                            vp(distance), vp(times), None, numA, numAt, nout, L.SBTV_HOST_PTRS)
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
    """Each is refused with the code (and message) its parent gives for the same fault, before any launch."""
    p = mc.problem("f")                                                               # 16 x 18, Haar, levels 3
    BADARG, SIZE, MAXITER, STOP, INIT, MISSING_AT, PSF = -1, -2, -3, -6, -7, -8, -10
    assert _raw(ctx, p)[0] == 0
    assert _raw(ctx, p, handle=None)[0] == BADARG
    bad = p["m"].copy()
    bad[3, 4] = -0.5
    nan, inf = bad.copy(), bad.copy()
    nan[3, 4], inf[3, 4] = np.nan, np.inf
    for kw in (dict(y=None), dict(mask=None), dict(h=None), dict(tau=None), dict(mu1=None), dict(mu2=None), dict(x_out=False),
               dict(batch=0), dict(mu1=np.array([0.0])), dict(mu1=np.array([-1.0])), dict(mu2=np.array([0.0])),
               dict(mu2=np.array([-1.0])),
               dict(h=np.array([1.0, 0.25])),                                          # not orthonormal
               dict(h=np.sqrt(2.0) * np.array([0.75, 0.25])),                          # sum sqrt 2 but not of unit norm
               dict(levels=1), dict(mask=bad), dict(mask=nan), dict(mask=inf)):
        assert _raw(ctx, p, **kw)[0] == BADARG, kw
    assert _raw(ctx, p, taps=None) == (MISSING_AT, "The function handle for transpose of A is missing")
    assert _raw(ctx, p, mask=None) == (BADARG, "SALSA_masked_analysis: the mask is missing")
    assert _raw(ctx, p, x_out=False) == (BADARG, "SALSA_masked_analysis: missing required argument")
    assert _raw(ctx, p, mu2=np.array([0.0])) == (BADARG, "SALSA_masked_analysis: mu1, mu2 must be > 0")
    assert _raw(ctx, p, mask=bad) == (BADARG, "SALSA_masked_analysis: the mask must be finite and non-negative")
    assert _raw(ctx, p, levels=5, h=wc.daub(4))[0] == SIZE                             # D4: reach 3 * 8 >= min(16, 18)
    assert _raw(ctx, p, levels=5)[0] == 0                                              # Haar: reach 8 fits
    assert _raw(ctx, p, y=np.ones((33, 35)))[0] == SIZE                                # an odd pixel count
    for stop in (0, 4):
        assert _raw(ctx, p, edit=_set(stopcriterion=stop)) == (STOP, "Unknown stopping criterion")
    assert _raw(ctx, p, edit=_set(initialization=1)) == (INIT, "Unknown 'Initialization' option")
    assert _raw(ctx, p, edit=_set(initialization=33333)) == (INIT, "Initialization = array but x_init is NULL")
    for m in (0, -1):
        assert _raw(ctx, p, edit=_set(maxiter=m)) == (MAXITER, "SALSA_masked_analysis: maxiter must be positive")
    assert _raw(ctx, p, y=np.ones((6, 6)), levels=2) == (PSF, "Mask does not fit inside array")
    assert _raw(ctx, p, edit=_set(TViters=0))[0] == 0                                  # no TV prox here: accepted


def test_keyword_interface_refusals(ctx):
    import sbtv
    p = mc.problem("f")
    op = _blur(p)
    common = dict(MU1=p["mu1"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, MAXITERA=3, ctx=ctx)
    calls0 = ctx.calls
    with pytest.raises(sbtv.SbtvError) as e:                              # no random start
        sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], INITIALIZATION=1, **common)
    assert e.value.code == -7
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], **dict(common, MAXITERA=0))
    assert (e.value.code, e.value.msg) == (-3, "SALSA_masked_analysis: maxiter must be positive")
    with pytest.raises(ValueError):                                       # TRUE_X is an image here, not coefficients
        sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], TRUE_X=wr.mrdwt_TI2D(p["x"], p["h"], p["levels"]), **common)
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], **{k: v for k, v in common.items() if k != "MU1"})
    assert e.value.code == -1
    with pytest.raises(sbtv.SbtvError, match="mask is missing") as e:
        sbtv.SALSA_masked_analysis(p["y"], op, None, p["tau"], **common)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="shape of y"):
        sbtv.SALSA_masked_analysis(p["y"], op, np.ones((16, 16)), p["tau"], **common)
    assert ctx.calls == calls0                                            # no operator was applied by any of the refused calls
    got = sbtv.SALSA_masked_analysis(p["y"], op, p["m"], p["tau"], **common)          # 'MU2' defaults to 0.1
    assert np.all(np.isfinite(got[0])) and len(got[3]) == 4
