"""GPU: CoRAL with the TV + wavelet-l1 regulariser (sbtv_CoRAL_wavelet, csrc/coral_wavelet.hip; sbtv.CoRAL_wavelet) against CoRAL_v2.m
restated line for line in NumPy with P1 = identity / TV and P2 = W, P2' = W' / soft (tests/coral_wavelet_restatement.py,
coral_literal) on the cases of tests/coral_wavelet_cases.py.

The bars are those of test_coral_matches_oracle (tests/test_gpu_admm.py): the same stopping iteration, objective / mses rtol 1e-9,
distance rtol 1e-7, max|x - ref| < 1e-7; times[0] == 0 and non-decreasing, traces n_outer + 1 long (distance (n_outer, 2)),
numA == 1 + n_outer, numAt == 2.  The cases whose rule fires inside the loop do so with a margin of at least 1 % on both sides,
and every Chambolle step is at least 1 % away from the inner tolerance (tests/test_coral_wavelet_cpu.py), far above those bars."""
import ctypes as C

import numpy as np
import pytest

import coral_wavelet_cases as cc
import coral_wavelet_restatement as cr
import wavelet_cases as wc
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu

NAMES = ("x", "numA", "numAt", "objective", "distance", "times", "mses")


def _taps(p):
    import sbtv
    return p.get("gain", 1.0) * sbtv.psf_family("gaussian", 7, p["p_true"])[0]


def _solve(ctx, p, **kw):
    import sbtv
    op = sbtv.BlurOperator(_taps(p))
    args = dict(MU1=p["mu1"], MU2=p["mu2"], WAVELET=p["h"], LEVELS=p["levels"], TVITERS=p["TViters"], AT=op.T,
                LS=op.LS(p["mu1"] + p["mu2"]), STOPCRITERION=p["stop"], TOLERANCEA=p["tolA"], MAXITERA=p["maxiter"], TRUE_X=p["x"],
                INITIALIZATION=p["init"], VERBOSE=0)
    args.update(kw)
    args = {k: v for k, v in args.items() if v is not None}
    return sbtv.CoRAL_wavelet(p["y"], op, p["tau1"], p["tau2"], ctx=ctx, **args)


def _check(got, ref):
    x, numA, numAt, objective, distance, times, mses = got
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1))) if np.shape(a) == np.shape(b) and len(a) else float("nan")
    print(f"outer iterations {len(objective) - 1} / {ref['n_outer']}, max|x - ref| = {np.max(np.abs(x - ref['x'])):.2e}, worst rel: "
          f"objective {rel(objective, ref['objective']):.2e}, distance {rel(distance, ref['distance']):.2e}, "
          f"mses {rel(mses, ref['mses']):.2e}")
    n = ref["n_outer"]
    assert len(objective) == len(ref["objective"]) == n + 1, "different stopping iteration"
    assert len(times) == len(mses) == n + 1 and np.shape(distance) == (n, 2)
    assert (numA, numAt) == (ref["numA"], ref["numAt"]) == (1 + n, 2)
    np.testing.assert_allclose(objective, ref["objective"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(mses, ref["mses"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(distance, ref["distance"], rtol=1e-7, atol=0)
    assert np.max(np.abs(x - ref["x"])) < 1e-7
    assert times[0] == 0 and np.all(np.diff(times) >= 0)


def _same_bits(a, b, skip=("times",)):
    for u, v, name in zip(a, b, NAMES):
        if name not in skip:
            np.testing.assert_array_equal(u, v, err_msg=name)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(1) rule 1 fires at 27 of 60: the lagged stop; (2) 16 x 18: a partly filled last workgroup; (3) D4, rectangular, zero start,
    three Chambolle iterations, mu1 != mu2; (4) 100 x 90, the chirp-z FFT path, to MAXITERA; (5) 15 x 16, odd M: TV(u) by the
    stand-alone reduction; (6) D4, rule 2 on the image, ten Chambolle iterations in two launches per prox; (7) 512 x 512: the
    grid-stride loops of both pixel passes; (8) rule 3 from a random start image."""
    p, ref = cc.problem(name), cc.reference(name)
    assert ref["n_outer"] == p["stops_at"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    calls = ctx.calls
    _check(got, ref)
    assert calls == cc.calls(p, ref["n_outer"])


def test_speculation_modes_give_the_same_bits(ctx):
    """SPECULATE 1 (default: optimistic prox launches, the host one iteration late), 0 (optimistic, no lag), 3 (exact launches)."""
    for name in ("1", "3"):
        p = cc.problem(name)
        lag, nolag, exact = _solve(ctx, p, SPECULATE=1), _solve(ctx, p, SPECULATE=0), _solve(ctx, p, SPECULATE=3)
        _same_bits(lag, nolag)
        _same_bits(lag, exact)
        _check(exact, cc.reference(name))


def test_without_true_x_no_mses_and_the_same_iterates(ctx):
    """The post pass without its first sum under rule 1 (case 2), and with the sum over x - xprev under rule 2 (case 6)."""
    for name in ("2", "6"):
        p = cc.problem(name)
        with_true, got = _solve(ctx, p), _solve(ctx, p, TRUE_X=None)
        assert len(got[6]) == 0
        _same_bits(got, with_true, skip=("times", "mses"))


def test_a_flat_observation_takes_one_exact_restart(ctx):
    """Every prox of the restatement stops at k = 1 (tests/test_coral_wavelet_cpu.py), so the optimistic launches of outer 2 are
    caught by the host's check of the step sums and the solve is repeated with exact launches, once."""
    p, ref = cc.flat_problem(), cc.flat_reference()
    assert [k for k, _ in ref["prox1"]] == [1] * 6
    s0 = ctx.solve_stats()["exact_restarts"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    assert ctx.calls == cc.calls(p, 6)                        # the repeat rewinds the counter
    assert ctx.solve_stats()["exact_restarts"] == s0 + 1
    _check(got, ref)


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = cc.problem("1")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    taps = np.stack([_taps(pa), sbtv.psf_family("gaussian", 7, (0.5, 0.35))[0]])
    y = np.stack([pa["y"], st2["y"]])
    tau1 = np.array([pa["tau1"], 0.4 * st2["sigma"] ** 2])
    tau2 = np.array([pa["tau2"], 0.6 * st2["sigma"] ** 2])
    mu1, mu2 = np.array([pa["mu1"], 0.1]), np.array([pa["mu2"], 0.03])
    tx = np.stack([pa["x"], x2])
    args = dict(WAVELET=pa["h"], LEVELS=pa["levels"], TVITERS=5, STOPCRITERION=1, TOLERANCEA=1e-4, MAXITERA=60, INITIALIZATION=2)
    opb = sbtv.BlurOperator(taps)
    both = sbtv.CoRAL_wavelet(y, opb, tau1, tau2, MU1=mu1, MU2=mu2, TRUE_X=tx, AT=opb.T, LS=opb.LS(mu1 + mu2), ctx=ctx, **args)
    lens = []
    for b in range(2):
        op1 = sbtv.BlurOperator(taps[b])
        one = sbtv.CoRAL_wavelet(y[b], op1, tau1[b], tau2[b], MU1=mu1[b], MU2=mu2[b], TRUE_X=tx[b], AT=op1.T,
                                 LS=op1.LS(mu1[b] + mu2[b]), ctx=ctx, **args)
        np.testing.assert_array_equal(both[0][b], one[0])
        assert (both[1][b], both[2][b]) == (one[1], one[2])
        for q in (3, 4, 6):
            np.testing.assert_array_equal(both[q][b], one[q])
        assert len(both[5][b]) == len(one[5])
        lens.append(len(one[3]) - 1)
    assert lens[0] == cc.reference("1")["n_outer"]
    print("outer iterations of the two images:", lens)


def test_solver_takes_device_tensors(ctx):
    import sbtv
    for name in ("4", "8"):                                   # (8): the start image is a device tensor too
        p = cc.problem(name)
        host = _solve(ctx, p)
        dev_init = sbtv.to_device(p["init"]) if isinstance(p["init"], np.ndarray) else p["init"]
        dev = _solve(ctx, dict(p, y=sbtv.to_device(p["y"]), x=sbtv.to_device(p["x"]), init=dev_init))
        _same_bits((sbtv.to_host(dev[0]),) + tuple(dev[1:]), (np.asarray(host[0]),) + tuple(host[1:]))


def test_a_threshold_above_every_coefficient_keeps_v_at_zero(ctx):
    """tau2 / mu2 above every soft argument of the run (coral_wavelet_cases.huge_tau2): v is zero throughout, so the second
    distance is ||W'x|| / ||W'x|| = 1, the l1 term of every objective entry is zero (parity at 1e-9 with the restatement, whose v
    is zero, under a tau2 this large: a coefficient of rounding size would already show), and the last entry is the data term
    of the returned x plus tau1 TV(u) alone."""
    p = cc.problem("2")
    n = 6
    q = dict(p, tau2=cc.huge_tau2(p, n), stop=2, tolA=0.0, maxiter=n, init=0)
    ref = cc.run(cr.coral_wavelet, q)
    assert not np.any(ref["v"])
    got = _solve(ctx, q)
    _check(got, ref)
    x, numA, numAt, objective, distance, times, mses = got
    np.testing.assert_allclose(distance[:, 1], 1.0, rtol=1e-12, atol=0)
    Bx = np.real(np.fft.ifft2(p["H"] * np.fft.fft2(np.asarray(x))))
    import sbtv_oracle as o
    assert objective[-1] - 0.5 * wr._sq(p["y"] - Bx) == pytest.approx(q["tau1"] * o.TVnorm(ref["u"]), rel=1e-6)   # no l1 term
    assert objective[0] == pytest.approx(0.5 * wr._sq(p["y"]), rel=1e-12)      # the zero start


def _raw(ctx, p, **kw):
    """sbtv_CoRAL_wavelet through the bare binding on problem p (three iterations, criterion 1 with tolerance 0, zero start);
    keywords replace arguments, `edit` changes the options after their defaults.  Returns (code, message)."""
    import sbtv
    from sbtv import _lib as L
    a = dict(y=p["y"], taps=sbtv.BlurOperator(_taps(p))._cm(1), taille=7, h=np.ascontiguousarray(p["h"]), levels=p["levels"],
             tau1=np.array([p["tau1"]]), tau2=np.array([p["tau2"]]), mu1=np.array([p["mu1"]]), mu2=np.array([p["mu2"]]), batch=1,
             x_out=True, handle=ctx.h, edit=None)
    a.update(kw)
    M, N = p["y"].shape if a["y"] is None else a["y"].shape
    K = 3
    so = L.sbtv_salsa_opts()
    ctx.lib.sbtv_salsa_opts_default(C.byref(so))
    so.stopcriterion, so.maxiter, so.tolA, so.initialization, so.TViters = 1, K, 0.0, 0, 5
    if a["edit"]:
        a["edit"](so)
    ycm = None if a["y"] is None else np.ascontiguousarray(a["y"].T, dtype=np.float64)
    x = np.zeros(M * N)
    mi = max(so.maxiter, K)
    objective, distance, times = np.zeros(mi + 1), np.zeros(2 * mi), np.zeros(mi + 1)
    numA, numAt, nout = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    vp = lambda v: None if v is None else L.vptr(v)
    ctx.reset_calls()
    rc = ctx.lib.sbtv_CoRAL_wavelet(a["handle"], vp(ycm), M, N, a["batch"], vp(a["taps"]), a["taille"], vp(a["h"]),
                                    0 if a["h"] is None else a["h"].size, a["levels"], vp(a["tau1"]), vp(a["tau2"]), vp(a["mu1"]),
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
    """Each is refused with the code sbtv_SALSA_analysis (frame, pointers, sizes) or sbtv_CoRAL_v2 (mu1, mu2, TViters) gives for
    the same fault, before any launch."""
    p = cc.problem("2")                                                               # 16 x 18, Haar, levels 3
    BADARG, SIZE, MAXITER, STOP, INIT, MISSING_AT, MISSING_LS, PSF = -1, -2, -3, -6, -7, -8, -9, -10
    assert _raw(ctx, p)[0] == 0
    assert _raw(ctx, p, handle=None)[0] == BADARG
    for kw in (dict(y=None), dict(h=None), dict(tau1=None), dict(tau2=None), dict(mu1=None), dict(mu2=None), dict(x_out=False),
               dict(batch=0),
               dict(h=np.array([1.0, 0.25])),                                          # not orthonormal
               dict(h=np.sqrt(2.0) * np.array([0.75, 0.25])),                          # sum sqrt 2 but not of unit norm
               dict(levels=1)):
        assert _raw(ctx, p, **kw)[0] == BADARG, kw
    assert _raw(ctx, p, taps=None) == (MISSING_AT, "The function handle for transpose of A is missing")
    assert _raw(ctx, p, x_out=False) == (BADARG, "CoRAL_wavelet: missing required argument")
    for kw in (dict(mu1=np.array([0.0])), dict(mu1=np.array([-1.0])), dict(mu2=np.array([0.0])), dict(mu2=np.array([-1.0]))):
        assert _raw(ctx, p, **kw)[0] == MISSING_LS, kw
    assert _raw(ctx, p, levels=5, h=wc.daub(4))[0] == SIZE                             # D4: reach 3 * 8 >= min(16, 18)
    assert _raw(ctx, p, levels=5)[0] == 0                                              # Haar: reach 8 fits
    assert _raw(ctx, p, y=np.ones((33, 35)))[0] == SIZE                                # an odd pixel count
    for stop in (0, 4):
        assert _raw(ctx, p, edit=_set(stopcriterion=stop)) == (STOP, "Unknown stopping criterion")
    assert _raw(ctx, p, edit=_set(initialization=1)) == (INIT, "Unknown 'Initialization' option")
    assert _raw(ctx, p, edit=_set(initialization=33333)) == (INIT, "Initialization = array but x_init is NULL")
    for m in (0, -1):
        assert _raw(ctx, p, edit=_set(maxiter=m)) == (MAXITER, "CoRAL_wavelet: maxiter must be positive")
        assert _raw(ctx, p, edit=_set(TViters=m)) == (MAXITER, "CoRAL_wavelet: TViters must be positive")
    assert _raw(ctx, p, y=np.ones((6, 6)), levels=2) == (PSF, "Mask does not fit inside array")


def test_keyword_interface_refusals(ctx):
    import sbtv
    p = cc.problem("2")
    op = sbtv.BlurOperator(_taps(p))
    mu = p["mu1"] + p["mu2"]
    common = dict(MU1=p["mu1"], MU2=p["mu2"], WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, LS=op.LS(mu), MAXITERA=3, ctx=ctx)
    run = lambda **kw: sbtv.CoRAL_wavelet(p["y"], op, p["tau1"], p["tau2"], **kw)
    assert len(run(**common)[3]) == 4
    with pytest.raises(sbtv.SbtvError) as e:                              # the random start of CoRAL_v2 is not offered
        run(INITIALIZATION=1, **common)
    assert e.value.code == -7
    with pytest.raises(sbtv.SbtvError) as e:
        run(**dict(common, MAXITERA=0))
    assert (e.value.code, e.value.msg) == (-3, "CoRAL_wavelet: maxiter must be positive")
    for bad_ls in (op.LS(p["mu1"]), None, sbtv.BlurOperator(_taps(p)).LS(mu)):   # another mu, none, another operator's
        with pytest.raises(sbtv.SbtvError) as e:
            run(**dict(common, LS=bad_ls))
        assert e.value.code == -9
    for missing in ("MU1", "MU2"):
        with pytest.raises(sbtv.SbtvError) as e:
            run(**{k: v for k, v in common.items() if k != missing})
        assert e.value.code == -1
    with pytest.raises(ValueError):                                       # TRUE_X is an image here, not coefficients
        run(TRUE_X=wr.mrdwt_TI2D(p["x"], p["h"], p["levels"]), **common)
    with pytest.raises(NotImplementedError):                              # the TV/TV front-end points here and keeps its type
        sbtv.CoRAL(p["y"], op, p["tau1"], p["tau2"], AT=op.T, LS=op.LS(mu), TVINITIALIZATION1=1, ctx=ctx)
