"""GPU: the wavelet-l1 FISTA driver (sbtv_fista_l1, csrc/wavelet_deconv.hip; sbtv.my_fista_l1) against my_fista_l1.m restated line for
line in NumPy (tests/fista_l1_restatement.py, fista_l1_literal) on the cases of tests/fista_l1_cases.py.

The bars are those tests/test_gpu_wavelet.py uses for this frame and operator: the same stopping iteration, objective / mses
rtol 1e-9, max|xw - ref| < 1e-7, max|x - W ref| < 1e-7, times[0] == 0 and non-decreasing, every trace n_iter long.  The cases
whose rule fires inside the loop do so with a margin far above those bars (tests/test_fista_l1_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import fista_l1_cases as fc
import wavelet_cases as wc
import wavelet_restatement as wr

pytestmark = pytest.mark.gpu


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, p["p_true"])[0])


def _solve(ctx, p, **kw):
    import sbtv
    args = dict(L=p["L"], xw_init=p["init"], return_xw=True, ctx=ctx)
    args.update(kw)
    return sbtv.my_fista_l1(p["y"], _blur(p), p["tau"], p["h"], p["levels"], p["stop"], p["tol"], p["maxiters"], p["true_xw"],
                            **args)


def _check(got, ref):
    Wx, objective, times, mses, xw = got
    print(f"iterations {len(objective)} / {ref['n_iter']}, max|xw - ref| = {np.max(np.abs(xw - ref['xw'])):.2e}, "
          f"max|x - W ref| = {np.max(np.abs(Wx - ref['x'])):.2e}, objective rel "
          f"{np.max(np.abs(objective[:2] / ref['objective'][:2] - 1)):.2e} (first two)")
    assert len(objective) == ref["n_iter"], "different stopping iteration"
    np.testing.assert_allclose(objective, ref["objective"], rtol=1e-9)
    np.testing.assert_allclose(mses, ref["mses"], rtol=1e-9)
    assert np.max(np.abs(xw - ref["xw"])) < 1e-7
    assert np.max(np.abs(Wx - ref["x"])) < 1e-7
    assert times[0] == 0 and np.all(np.diff(times) >= 0)
    assert len(times) == len(mses) == len(objective)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(a) rule 1 fires at k = 55 of 80: the lagged stop; (b) rule 2; (c) rule 3 with L = 2; (d) 100 x 90, the chirp-z FFT
    path, to maxiters; (e) 512 x 512: 2 621 440 coefficients, the grid-stride loop of the step kernel; (f) 16 x 18: a partly
    filled last workgroup; (g) a random coefficient start."""
    p, ref = fc.problem(name), fc.reference(name)
    if name in "abcf":
        assert 2 < ref["n_iter"] < p["maxiters"], ref["n_iter"]
    else:
        assert ref["n_iter"] == p["maxiters"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    calls = ctx.calls
    _check(got, ref)
    assert calls == ref["calls"] == 2 + 3 * (ref["n_iter"] - 1)


def test_without_true_no_mses_and_the_same_iterates(ctx):
    """The step kernel without the fourth sum."""
    import sbtv
    p = fc.problem("f")
    with_true = _solve(ctx, p)
    got = sbtv.my_fista_l1(p["y"], _blur(p), p["tau"], p["h"], p["levels"], p["stop"], p["tol"], p["maxiters"], None,
                           return_xw=True, ctx=ctx)
    assert len(got[3]) == 0
    np.testing.assert_array_equal(got[1], with_true[1])
    np.testing.assert_array_equal(got[4], with_true[4])
    np.testing.assert_array_equal(got[0], with_true[0])


def test_solver_without_the_lag_gives_the_same_result(ctx):
    p = fc.problem("a")
    lag, nolag = _solve(ctx, p), _solve(ctx, p, lag=False)
    for a, b, name in zip(lag, nolag, ("Wx", "objective", "times", "mses", "xw")):
        if name != "times":
            np.testing.assert_array_equal(a, b, err_msg=name)
    _check(nolag, fc.reference("a"))


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = fc.problem("a")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    taps = np.stack([sbtv.psf_family("gaussian", 7, pa["p_true"])[0], sbtv.psf_family("gaussian", 7, (0.5, 0.35))[0]])
    y = np.stack([pa["y"], st2["y"]])
    tau = np.array([pa["tau"], 0.5 * st2["sigma"] ** 2])
    tx = np.stack([pa["true_xw"], wr.mrdwt_TI2D(x2, pa["h"], pa["levels"])])
    args = (pa["h"], pa["levels"], 1, 1e-4, 80)
    both = sbtv.my_fista_l1(y, sbtv.BlurOperator(taps), tau, *args, tx, return_xw=True, ctx=ctx)
    lens = []
    for b in range(2):
        one = sbtv.my_fista_l1(y[b], sbtv.BlurOperator(taps[b]), tau[b], *args, tx[b], return_xw=True, ctx=ctx)
        np.testing.assert_array_equal(both[0][b], one[0])
        np.testing.assert_array_equal(both[4][b], one[4])
        for q in (1, 3):
            np.testing.assert_array_equal(both[q][b], one[q])
        assert len(both[2][b]) == len(one[1])
        lens.append(len(one[1]))
    assert lens[0] == fc.reference("a")["n_iter"]
    print("iterations of the two images:", lens)


def test_solver_takes_device_tensors(ctx):
    import sbtv
    p = fc.problem("d")
    host = _solve(ctx, p)
    dev = sbtv.my_fista_l1(sbtv.to_device(p["y"]), _blur(p), p["tau"], p["h"], p["levels"], p["stop"], p["tol"], p["maxiters"],
                           sbtv.to_device(p["true_xw"]), L=p["L"], return_xw=True, ctx=ctx)
    np.testing.assert_array_equal(sbtv.to_host(dev[0]), np.asarray(host[0]))
    np.testing.assert_array_equal(sbtv.to_host(dev[4]), np.asarray(host[4]))
    np.testing.assert_array_equal(dev[1], host[1])
    np.testing.assert_array_equal(dev[3], host[3])


def test_full_size_kernel_image_is_the_blur_operator(ctx):
    """h as the reference passes it: the full-size image with the taps in its top-left corner."""
    import sbtv
    p = fc.problem("f")
    hk = np.zeros(p["y"].shape)
    hk[:7, :7] = sbtv.psf_family("gaussian", 7, p["p_true"])[0]
    got = sbtv.my_fista_l1(p["y"], hk, p["tau"], p["h"], p["levels"], p["stop"], p["tol"], p["maxiters"], p["true_xw"],
                           return_xw=True, ctx=ctx)
    for a, b, name in zip(got, _solve(ctx, p), ("Wx", "objective", "times", "mses", "xw")):
        if name != "times":
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_a_threshold_above_every_coefficient_keeps_x_at_zero(ctx):
    import sbtv
    p = fc.problem("f")
    tau = fc.huge_tau(p)
    r2 = sbtv.my_fista_l1(p["y"], _blur(p), tau, p["h"], p["levels"], 2, 1e300, 6, p["true_xw"], return_xw=True, ctx=ctx)
    assert len(r2[1]) == 6 and not np.any(r2[4]) and not np.any(r2[0])          # rule 2 is NaN: never fires
    assert np.all(r2[1] == r2[1][0])
    np.testing.assert_allclose(r2[1][0], 0.5 * wr._sq(p["y"]), rtol=1e-12)
    r1 = sbtv.my_fista_l1(p["y"], _blur(p), tau, p["h"], p["levels"], 1, 1e-6, 6, p["true_xw"], return_xw=True, ctx=ctx)
    assert len(r1[1]) == 2 and not np.any(r1[4])
    one = sbtv.my_fista_l1(p["y"], _blur(p), p["tau"], p["h"], p["levels"], 1, 0.0, 1, p["true_xw"], return_xw=True, ctx=ctx)
    assert len(one[1]) == len(one[2]) == len(one[3]) == 1 and not np.any(one[4])   # maxiters = 1: the start state
    assert one[3][0] == pytest.approx(wr._sq(p["true_xw"]) / p["true_xw"].size, rel=1e-12)


def _raw(ctx, p, **kw):
    """sbtv_fista_l1 through the bare binding on problem p; keywords replace arguments.  Returns (code, message)."""
    from sbtv import _lib as L
    a = dict(b=p["y"], taps=_blur(p)._cm(1), taille=7, h=np.ascontiguousarray(p["h"]), levels=p["levels"], tau=np.array([p["tau"]]),
             L=1.0, stop=1, tol=0.0, maxiters=3, batch=1, xw_out=True, handle=ctx.h)
    a.update(kw)
    M, N = p["y"].shape if a["b"] is None else a["b"].shape
    bcm = None if a["b"] is None else np.ascontiguousarray(a["b"].T, dtype=np.float64)
    xw = np.zeros((3 * (p["levels"] - 1) + 1) * M * N)
    vp = lambda v: None if v is None else L.vptr(v)
    n = (C.c_int * 1)()
    rc = ctx.lib.sbtv_fista_l1(a["handle"], vp(bcm), M, N, a["batch"], vp(a["taps"]), a["taille"], vp(a["h"]),
                               0 if a["h"] is None else a["h"].size, a["levels"], vp(a["tau"]), a["L"], a["stop"], a["tol"],
                               a["maxiters"], None, None, vp(xw) if a["xw_out"] else None, None, None, None, None, n,
                               L.SBTV_HOST_PTRS)
    try:
        ctx.check(rc)
    except L.SbtvError as e:
        return e.code, e.msg
    return rc, ""


def test_refusals(ctx):
    """Each is refused with its code before any launch."""
    p = fc.problem("f")
    BADARG, SIZE, MAXITER, STOP, PSF = -1, -2, -3, -6, -10
    assert _raw(ctx, p)[0] == 0
    assert _raw(ctx, p, handle=None)[0] == BADARG
    for kw in (dict(b=None), dict(taps=None), dict(h=None), dict(tau=None), dict(xw_out=False), dict(batch=0),
               dict(L=0.0), dict(L=-1.0), dict(L=float("inf")), dict(L=float("nan")), dict(tol=float("nan")),
               dict(tau=np.array([-1.0])), dict(tau=np.array([float("inf")])), dict(tau=np.array([float("nan")])),
               dict(h=np.array([1.0, 0.25])),                                          # not orthonormal
               dict(h=np.sqrt(2.0) * np.array([0.75, 0.25])),                          # sum sqrt 2 but not of unit norm
               dict(levels=1)):
        assert _raw(ctx, p, **kw)[0] == BADARG, kw
    for stop in (0, 4):
        assert _raw(ctx, p, stop=stop) == (STOP, "Invalid stopping criterion!")
    assert _raw(ctx, p, maxiters=0)[0] == MAXITER
    assert _raw(ctx, p, levels=5)[0] == SIZE                                           # reach 3 * 8 >= min(16, 18)
    assert _raw(ctx, p, b=np.ones((33, 35)))[0] == SIZE                                # an odd pixel count
    assert _raw(ctx, p, b=np.ones((6, 6)), levels=2) == (PSF, "Mask does not fit inside array")
    assert _raw(ctx, p, taille=16)[0] == PSF
