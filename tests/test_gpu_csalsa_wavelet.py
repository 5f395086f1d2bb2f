"""GPU: C-SALSA with the wavelet analysis prior (sbtv_CSALSA_wavelet, csrc/csalsa_wavelet.hip; sbtv.csalsa_wavelet) against
CSALSA_v2.m restated line for line in NumPy with P = W, PT = W', psi = soft and phi = ||W' .||_1
(tests/csalsa_wavelet_restatement.py, csalsa_wavelet_literal) on the cases of tests/csalsa_wavelet_cases.py.

The bars are the project's own for these operators: the same stopping iteration; objective rtol 1e-9, criterion 1e-8 and
distance1 rtol 1e-6 with atol 1e-9 (tests/test_gpu_admm.py); distance2 and mses rtol 1e-9 and max|x - ref| < 1e-7
(tests/test_gpu_analysis.py); times[0] == 0 and non-decreasing; every trace n_outer long; numA, numAt and the call counter as
csalsa_one counts them.  The cases that stop inside the loop do so with the margins tests/test_csalsa_wavelet_cpu.py asserts
(1 % in the rule, 1e-3 in criterion / epsilon and in ||ve|| / epsilon), far above those bars."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import csalsa_wavelet_cases as cc
import wavelet_cases as wc

pytestmark = pytest.mark.gpu

NAMES = ("x", "numA", "numAt", "objective", "distance1", "distance2", "criterion", "times", "mses")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, p["p_true"])[0])


def _solve(ctx, p, **kw):
    import sbtv
    op = _blur(p)
    args = dict(WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, STOPCRITERION=p["stop"], TOLERANCEA=p["tolA"], MAXITERA=p["maxiter"],
                TRUE_X=p["x"], INITIALIZATION=p["init"], CONTINUATIONFACTOR=p["delta"], EPSILON=p["epsilon"], VERBOSE=0)
    args.update(kw)
    args = {k: v for k, v in args.items() if v is not None}
    return sbtv.csalsa_wavelet(p["y"], op, p["mu1"], p["mu2"], p["sigma"], ctx=ctx, **args)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not a.size:
        return float("nan")
    nz = b != 0
    return float(np.max(np.abs(a[nz] / b[nz] - 1))) if np.any(nz) else 0.0


def _within_bars(got, ref, tag=""):
    """got, ref: dicts of x, objective, distance1, distance2, criterion, mses."""
    print(f"{tag}max|x - ref| = {np.max(np.abs(got['x'] - ref['x'])):.2e}, worst rel: " +
          ", ".join(f"{k} {_rel(got[k], ref[k]):.2e}" for k in ("objective", "criterion", "distance1", "distance2", "mses")))
    np.testing.assert_allclose(got["objective"], ref["objective"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["criterion"], ref["criterion"], rtol=1e-8, atol=0)
    np.testing.assert_allclose(got["distance1"], ref["distance1"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got["distance2"], ref["distance2"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["mses"], ref["mses"], rtol=1e-9, atol=0)
    assert np.max(np.abs(got["x"] - ref["x"])) < 1e-7


def _check(got, ref):
    g = dict(zip(NAMES, got))
    n = ref["n_outer"]
    print(f"outer iterations {len(g['objective'])} / {n}")
    assert len(g["objective"]) == len(ref["objective"]) == n, "different stopping iteration"
    for k in ("distance1", "distance2", "criterion", "times", "mses"):
        assert len(g[k]) == n, k
    assert (g["numA"], g["numAt"]) == (ref["numA"], ref["numAt"])
    _within_bars(g, ref)
    assert g["times"][0] == 0 and np.all(np.diff(g["times"]) >= 0)


def _same_bits(a, b, skip=("times",)):
    for u, v, name in zip(a, b, NAMES):
        if name not in skip:
            np.testing.assert_array_equal(u, v, err_msg=name)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_solver_matches_the_literal_restatement(ctx, name):
    """(a) rule 3 and the constraint met at 23 of 60: the lagged stop; (b) D4, rule 1 on the objective ||W'x||_1; (c) rule 2 on the
    image from a given start; (d) 100 x 90, the chirp-z plan: the image form; (e) 512 x 512, 2 621 440 coefficients: the
    grid-stride loop of the step kernel; (f) 16 x 18: a partly filled last workgroup; (g) the constraint decides the stop; (h)
    mu2 != 1; (i) a wide ball: both branches of the projection; (j) a continuation factor: the image form, a new threshold per
    iteration."""
    p, ref = cc.problem(name), cc.reference(name)
    assert ref["n_outer"] == p["stops_at"]
    ctx.reset_calls()
    got = _solve(ctx, p)
    calls = ctx.calls
    _check(got, ref)
    assert calls == cc.calls(p, ref["n_outer"])
    if name in cc.INSIDE:
        f = cc.feasible(p, np.asarray(got[0]))
        print(f"||B x - y|| / epsilon of the returned x: {f:.5f}")
        assert f <= 1


def test_solver_without_the_lagged_stop_rule_gives_the_same_result(ctx):
    for name in ("a", "g"):
        p = cc.problem(name)
        lag, exact = _solve(ctx, p), _solve(ctx, p, SPECULATE=0)
        _same_bits(lag, exact)
        _check(exact, cc.reference(name))


def test_without_true_x_no_mses_and_the_same_iterates(ctx):
    """No pixel pass under rule 3 (f), the pixel pass without its first sum under rule 2 (g)."""
    for name in ("f", "g"):
        p = cc.problem(name)
        with_true, got = _solve(ctx, p), _solve(ctx, p, TRUE_X=None)
        assert len(got[8]) == 0
        _same_bits(got, with_true, skip=("times", "mses"))


def test_batch_of_two_equals_the_single_calls_bit_for_bit(ctx):
    import sbtv
    pa = cc.problem("a")
    x2 = wc.synth_image(64, 64, 9)
    st2 = wc.setup(x2, seed=6)
    taps = np.stack([sbtv.psf_family("gaussian", 7, pa["p_true"])[0], sbtv.psf_family("gaussian", 7, (0.5, 0.35))[0]])
    y = np.stack([pa["y"], st2["y"]])
    mu1, mu2, sigma = np.array([pa["mu1"], 1.5]), np.array([pa["mu2"], 0.8]), np.array([pa["sigma"], st2["sigma"]])
    tx = np.stack([pa["x"], x2])
    args = dict(WAVELET=pa["h"], LEVELS=pa["levels"], STOPCRITERION=3, TOLERANCEA=1e-3, MAXITERA=60, INITIALIZATION=0)
    opb = sbtv.BlurOperator(taps)
    both = sbtv.csalsa_wavelet(y, opb, mu1, mu2, sigma, TRUE_X=tx, AT=opb.T, ctx=ctx, **args)
    lens = []
    for b in range(2):
        op1 = sbtv.BlurOperator(taps[b])
        one = sbtv.csalsa_wavelet(y[b], op1, mu1[b], mu2[b], sigma[b], TRUE_X=tx[b], AT=op1.T, ctx=ctx, **args)
        np.testing.assert_array_equal(both[0][b], one[0])
        assert (both[1][b], both[2][b]) == (one[1], one[2])
        for q in (3, 4, 5, 6, 8):
            np.testing.assert_array_equal(both[q][b], one[q])
        assert len(both[7][b]) == len(one[7])
        lens.append(len(one[3]))
    assert lens[0] == cc.reference("a")["n_outer"]
    print("outer iterations of the two images:", lens)


def test_solver_takes_device_tensors(ctx):
    import sbtv
    for name in ("d", "c"):                                   # (c): the start image is a device tensor too
        p = cc.problem(name)
        host = _solve(ctx, p)
        dev_init = sbtv.to_device(p["init"]) if isinstance(p["init"], np.ndarray) else p["init"]
        op = _blur(p)
        dev = sbtv.csalsa_wavelet(sbtv.to_device(p["y"]), op, p["mu1"], p["mu2"], p["sigma"], "WAVELET", p["h"], "LEVELS",
                                  p["levels"], "AT", op.T, "STOPCRITERION", p["stop"], "TOLERANCEA", p["tolA"], "MAXITERA",
                                  p["maxiter"], "TRUE_X", sbtv.to_device(p["x"]), "INITIALIZATION", dev_init, ctx=ctx)
        _same_bits((sbtv.to_host(dev[0]),) + tuple(dev[1:]), (np.asarray(host[0]),) + tuple(host[1:]))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%(root)r, "semi-blind-image-deblurring-problems-with-tv_amd"))
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import sbtv
import csalsa_wavelet_cases as cc
import wavelet_cases as wc
res = {}
pa = cc.problem("a")
runs = {"a": (pa["y"], pa["x"], pa["sigma"], pa["p_true"], dict(STOPCRITERION=pa["stop"], TOLERANCEA=pa["tolA"], MAXITERA=pa["maxiter"]))}
for tag, shape in (("b", (256, 192)), ("c", (256, 128))):
    x = wc.synth_image(shape[0], shape[1], 8)
    st = wc.setup(x, seed=2)
    runs[tag] = (st["y"], x, st["sigma"], st["p_true"], dict(STOPCRITERION=2, TOLERANCEA=1e-9, MAXITERA=15, INITIALIZATION=2))
for tag, (y, tx, sigma, pt, kw) in runs.items():
    op = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, pt)[0])
    got = sbtv.csalsa_wavelet(y, op, 1.0, 1.0, sigma, WAVELET=pa["h"], LEVELS=4, AT=op.T, TRUE_X=tx, VERBOSE=0, **kw)
    for nm, v in zip(("x", "objective", "distance1", "distance2", "criterion", "mses"), (got[0], got[3], got[4], got[5], got[6], got[8])):
        res[tag + "_" + nm] = np.asarray(v)
np.savez(sys.argv[1], **res)
"""


def test_spectral_and_image_forms_agree(tmp_path):
    """The default (the constraint split as one spectrum and a scalar) against SBTV_CSALSA_SPECTRAL=0 (v and bv as images), each in
    a fresh child process: case a (the stop inside the loop), a 256 x 192 problem (its FFT plan has no OP_CSALSA row pass: both
    runs take the image form, as the third size of test_csalsa_spectral_and_image_forms_agree does) and a 256 x 128 one, 15
    iterations each."""
    def run(name, env):
        out = str(tmp_path / (name + ".npz"))
        e = dict(os.environ)
        e.update(env)
        subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], check=True, env=e, timeout=600)
        return np.load(out)
    a, b = run("spectral", {}), run("images", {"SBTV_CSALSA_SPECTRAL": "0"})
    keys = ("x", "objective", "distance1", "distance2", "criterion", "mses")
    for tag in ("a", "b", "c"):
        sp, im = ({k: r[tag + "_" + k] for k in keys} for r in (a, b))
        assert len(sp["objective"]) == len(im["objective"]), "different stopping iteration"
        _within_bars(im, sp, tag + ": ")
        if tag != "b":
            assert np.any(im["x"] != sp["x"]), "the two runs took the same form"
    ref = cc.reference("a")
    assert len(a["a_objective"]) == ref["n_outer"]
    _within_bars({k: b["a_" + k] for k in keys}, ref, "a, image form against the literal restatement: ")
    assert len(a["b_objective"]) == len(a["c_objective"]) == 15


def _raw(ctx, p, **kw):
    """sbtv_CSALSA_wavelet through the bare binding on problem p (three iterations, rule 3 with tolerance 0, zero start); keywords
    replace arguments, `edit` changes the options after their defaults.  Returns (code, message)."""
    from sbtv import _lib as L
    one = lambda v: np.array([float(v)])
    a = dict(y=p["y"], taps=_blur(p)._cm(1), taille=7, h=np.ascontiguousarray(p["h"]), levels=p["levels"], mu1=one(p["mu1"]),
             mu2=one(p["mu2"]), sigma=one(p["sigma"]), batch=1, x_out=True, handle=ctx.h, edit=None)
    a.update(kw)
    M, N = p["y"].shape if a["y"] is None else a["y"].shape
    K = 3
    so = L.sbtv_salsa_opts()
    ctx.lib.sbtv_salsa_opts_default(C.byref(so))
    so.stopcriterion, so.maxiter, so.tolA, so.initialization = 3, K, 0.0, 0
    if a["edit"]:
        a["edit"](so)
    ycm = None if a["y"] is None else np.ascontiguousarray(a["y"].T, dtype=np.float64)
    x = np.zeros(M * N)
    tr = [np.zeros(max(so.maxiter, K)) for _ in range(5)]
    numA, numAt, nout = (C.c_int * 1)(), (C.c_int * 1)(), (C.c_int * 1)()
    vp = lambda v: None if v is None else L.vptr(v)
    ctx.reset_calls()
    rc = ctx.lib.sbtv_CSALSA_wavelet(a["handle"], vp(ycm), M, N, a["batch"], vp(a["taps"]), a["taille"], vp(a["h"]),
                                     0 if a["h"] is None else a["h"].size, a["levels"], vp(a["mu1"]), vp(a["mu2"]), vp(a["sigma"]),
                                     None, 1.0, C.byref(so), None, None, vp(x) if a["x_out"] else None, vp(tr[0]), vp(tr[1]),
                                     vp(tr[2]), vp(tr[3]), vp(tr[4]), None, numA, numAt, nout, L.SBTV_HOST_PTRS)
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
    """Each is refused with the code sbtv_SALSA_analysis or sbtv_CSALSA_v2 gives for the same fault, before any launch."""
    p = cc.problem("f")                                                               # 16 x 18, Haar, levels 3
    BADARG, SIZE, MAXITER, STOP, INIT, MISSING_AT, MISSING_LS, PSF = -1, -2, -3, -6, -7, -8, -9, -10
    assert _raw(ctx, p)[0] == 0
    assert _raw(ctx, p, handle=None)[0] == BADARG
    for kw in (dict(y=None), dict(h=None), dict(mu1=None), dict(mu2=None), dict(sigma=None), dict(x_out=False), dict(batch=0),
               dict(h=np.array([1.0, 0.25])),                                          # not orthonormal
               dict(h=np.sqrt(2.0) * np.array([0.75, 0.25])),                          # sum sqrt 2 but not of unit norm
               dict(levels=1)):
        assert _raw(ctx, p, **kw)[0] == BADARG, kw
    assert _raw(ctx, p, x_out=False) == (BADARG, "CSALSA_wavelet: missing required argument")
    for kw in (dict(mu1=np.array([0.0])), dict(mu1=np.array([-1.0])), dict(mu2=np.array([0.0])), dict(mu2=np.array([-2.0]))):
        assert _raw(ctx, p, **kw) == (MISSING_LS, "(A^T A + \\mu I)^(-1) must be specified: mu1, mu2 must be > 0"), kw
    assert _raw(ctx, p, taps=None) == (MISSING_AT, "The function handle for transpose of A is missing")
    assert _raw(ctx, p, levels=5, h=wc.daub(4))[0] == SIZE                             # D4: reach 3 * 8 >= min(16, 18)
    assert _raw(ctx, p, levels=5)[0] == 0                                              # Haar: reach 8 fits
    assert _raw(ctx, p, y=np.ones((33, 35)))[0] == SIZE                                # an odd pixel count
    for stop in (0, 4):
        assert _raw(ctx, p, edit=_set(stopcriterion=stop)) == (STOP, "Unknown stopping criterion")
    assert _raw(ctx, p, edit=_set(initialization=1)) == (INIT, "Unknown 'Initialization' option")
    assert _raw(ctx, p, edit=_set(initialization=33333)) == (INIT, "Initialization = array but x_init is NULL")
    for m in (0, -1):
        assert _raw(ctx, p, edit=_set(maxiter=m)) == (MAXITER, "CSALSA_wavelet: maxiter must be positive")
    assert _raw(ctx, p, y=np.ones((6, 6)), levels=2) == (PSF, "Mask does not fit inside array")
    assert _raw(ctx, p, edit=_set(TViters=0))[0] == 0                                  # no TV prox here: accepted


def test_keyword_interface_refusals(ctx):
    import sbtv
    p = cc.problem("f")
    op = _blur(p)
    common = dict(WAVELET=p["h"], LEVELS=p["levels"], AT=op.T, MAXITERA=3, ctx=ctx)
    with pytest.raises(sbtv.SbtvError) as e:                              # the random start of CSALSA_v2 is not offered
        sbtv.csalsa_wavelet(p["y"], op, 1.0, 1.0, p["sigma"], INITIALIZATION=1, **common)
    assert e.value.code == -7
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.csalsa_wavelet(p["y"], op, 1.0, 1.0, p["sigma"], **dict(common, MAXITERA=0))
    assert (e.value.code, e.value.msg) == (-3, "CSALSA_wavelet: maxiter must be positive")
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.csalsa_wavelet(p["y"], op, 1.0, 1.0, p["sigma"], **{k: v for k, v in common.items() if k != "AT"})
    assert e.value.code == -8
    with pytest.raises(ValueError):                                       # TRUE_X is an image here, not coefficients
        sbtv.csalsa_wavelet(p["y"], op, 1.0, 1.0, p["sigma"], TRUE_X=np.zeros((16, 18 * 7)), **common)
