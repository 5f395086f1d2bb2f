"""GPU: the SK-ROCK chain on the TV posterior at fixed parameters (sbtv_skrock, csrc/skrock.hip) against
the NumPy restatement (tests/skrock_tv_restatement.py) on the cases of tests/skrock_tv_cases.py: delta = 0.8 of the stability
bound, chambolleit = 25, theta = 0.02.

Parity with injected noise: the last sample at rtol = atol = 1e-9, gx and logpi at rtol 1e-9: the bar
test_plain_myula_chain_matches_oracle holds for the same prox and operator.  tests/test_skrock_tv_cpu.py shows that no prox call
of a case sits on the edge of the stop rule and that the chain amplifies prox rounding by less than 1e3, which is what makes
the bar meaningful.  Moments: the tolerance of tests/test_gpu_posterior.py.  Every test prints its figures.

Measured on an MI355X: gx off by at most 6.7e-16 relative, logpi by 2.7e-15 (3.3e-15 from a start state x0), the last sample by
2.1e-12 absolute = 8.8e-15 max|X| (32 x 32, s = 10; <= 3.5e-15 max|X| elsewhere); the Philox chain 4.4e-16 / 1.4e-15 / 1.9e-15;
the normals of step 0 recovered from sbtv.myula differ from the restated ones by 1.4e-14; means off by <= 7.4e-13 and
variances by <= 3.9e-11 absolute.  The whole file takes 3 s."""
import ctypes as C

import numpy as np
import pytest

import philox_restatement as phr
import skrock_tv_cases as skc
import wavelet_myula_restatement as wmr

pytestmark = pytest.mark.gpu

KEYS = ("x", "gx", "logpi")


def _blur(q):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, q["p"])[0])


def _op(name, **kw):
    q = skc.problem(name)
    return dict(dict(q["op"], y=q["y"], A=_blur(q), theta_op=q["theta"], sigma2=q["sigma2"]), **kw)


def _run(ctx, name, noise=None, x0=None, posterior=None, **kw):
    import sbtv
    return sbtv.skrock(_op(name, **kw), noise=noise, x0=x0, posterior=posterior, ctx=ctx)


def _same(a, b, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def _assert_chain(tag, r, rr):
    ref = rr["samples"][-1]
    xs, ex = float(np.max(np.abs(ref))), float(np.max(np.abs(np.asarray(r["x"]) - ref)))
    for k in ("gx", "logpi"):
        a = np.asarray(r[k])
        assert a.shape == rr[k].shape, (k, a.shape)
        print(f"{tag} {k}: worst rel {np.max(np.abs(a / rr[k] - 1)):.1e}")
    print(f"{tag}: max|X - ref| = {ex:.1e}, / max|X| = {ex / xs:.1e}")
    for k in ("gx", "logpi"):
        np.testing.assert_allclose(np.asarray(r[k]), rr[k], rtol=1e-9, atol=0, err_msg=k)
    np.testing.assert_allclose(np.asarray(r["x"]), ref, rtol=1e-9, atol=1e-9)


# ---- 1. parity with injected noise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", skc.NAMES)
def test_chain_and_traces_match_the_restatement(ctx, name):
    """32 x 32 at s = 2 (first and last stage in consecutive launches), 3 (odd: the buffers swap) and 10; 24 x 40 at s = 5:
    the chirp-z transform and tvnorm_partials for the trace."""
    q = skc.problem(name)
    _assert_chain(name, _run(ctx, name, q["noise"]), skc.reference(name))


def test_start_state_x0(ctx):
    """X(1) = x0: sample 1 of the traces is that of x0, and the chain is the restatement started there."""
    q = skc.problem("sq-s3")
    x0 = 0.5 * q["y"] + 20.0
    _assert_chain("x0", _run(ctx, "sq-s3", q["noise"], x0=x0), skc.chain("sq-s3", x0=x0))


# ---- 2. the generator -----------------------------------------------------------------------------------------------
def test_philox_chain_is_the_restatement_fed_with_the_restated_normals(ctx):
    """noise = NULL: pair q of chain b at sample ii draws (q, ii - 2, chain_offset + b), the counters of sbtv_myula."""
    import sbtv
    name, seed, off = "sq-s3", 11, 2
    q = skc.problem(name)
    M, N = q["y"].shape
    steps = q["op"]["samples"] - 1
    nz = phr.as_arrays(phr.chain_normals(M * N, steps, 1, seed, off), M)[:, 0]
    ref = skc.chain(name, noise=nz)
    a = _run(ctx, name, seed=seed, chain_offset=off)
    _assert_chain("Philox", a, ref)
    _same(a, _run(ctx, name, seed=seed, chain_offset=off))                          # same seed, same bits
    c = _run(ctx, name, seed=seed + 1, chain_offset=off)
    assert np.max(np.abs(np.asarray(c["x"]) - np.asarray(a["x"]))) > 1e-3
    assert c["gx"][0] == a["gx"][0] and c["gx"][1] != a["gx"][1]                    # the start state draws nothing
    # the normals of the first step are those of sbtv_myula with that seed: one MYULA step with the generator minus the same
    # step with zero noise is sqrt(2 gamma) Z; SK-ROCK fed with that Z makes the generator's first step
    gamma = 0.5
    mop = dict(y=q["y"], samples=3, theta_op=q["theta"], gamma=gamma, A=_blur(q), sigma2=q["sigma2"], chambolleit=25, seed=seed,
               chain_offset=off, **{"lambda": q["lambda"]})
    z = (np.asarray(sbtv.myula(mop, ctx=ctx)) - np.asarray(sbtv.myula(mop, noise=np.zeros((1, M, N)), ctx=ctx))) / np.sqrt(2 * gamma)
    print(f"normals of step 0 from sbtv.myula against the restated ones: max |d| = {np.max(np.abs(z - nz[0])):.1e}")
    np.testing.assert_allclose(z, nz[0], rtol=0, atol=1e-9)
    one = _run(ctx, name, seed=seed, chain_offset=off, samples=2)
    inj = _run(ctx, name, noise=z[None], samples=2)
    np.testing.assert_allclose(np.asarray(inj["x"]), np.asarray(one["x"]), rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(one["gx"], a["gx"][:2])


# ---- 3. independence ------------------------------------------------------------------------------------------------
def test_chains_of_a_batch_are_computed_as_alone(ctx):
    """Three chains with their own theta, sigma2 and stream in one call are the three single calls, bit for bit, with the
    generator and with injected noise, moments included."""
    name = "sq-s3"
    q = skc.problem(name)
    y3 = np.stack([q["y"], q["y"][::-1].copy(), q["y"].T.copy()])
    th, s2 = np.array([0.02, 0.03, 0.015]), q["sigma2"] * np.array([1.0, 1.3, 0.8])
    rng = np.random.default_rng(3)
    nz = rng.standard_normal((q["op"]["samples"] - 1, 3) + q["y"].shape)
    post = dict(first=2)
    for noise in (None, nz):
        both = _run(ctx, name, noise, y=y3, theta_op=th, sigma2=s2, seed=5, chain_offset=2, posterior=post)
        assert both["x"].shape == (3,) + q["y"].shape and both["gx"].shape == (3, q["op"]["samples"])
        for b in range(3):
            alone = _run(ctx, name, None if noise is None else noise[:, b], y=y3[b], theta_op=th[b], sigma2=s2[b], seed=5,
                         chain_offset=2 + b, posterior=post)
            for k in KEYS + ("mean", "var"):
                np.testing.assert_array_equal(np.asarray(both[k])[b], np.asarray(alone[k]), err_msg=f"{k} chain {b}")
            assert both["count"][b] == alone["count"]
        assert both["gx"][0, 1] != both["gx"][1, 1]


# ---- 4. moments -----------------------------------------------------------------------------------------------------
def _assert_moments(mean, var, ref_mean, ref_var):
    """the tolerance of tests/test_gpu_posterior.py"""
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(var, ref_var, rtol=1e-6, atol=1e-8 * np.max(ref_var))


@pytest.mark.parametrize("name", ["sq-s3", "rect-s5"])
def test_moments_are_the_welford_recursion_of_the_restated_samples(ctx, name):
    q, ref = skc.problem(name), skc.reference(name)
    S = q["op"]["samples"]
    plain = _run(ctx, name, q["noise"])
    for first, thin in ((1, 1), (2, 2), (S, 1), (0, 3)):
        got = _run(ctx, name, q["noise"], posterior=dict(first=first, thin=thin))
        f = first or 1
        n = (S - f) // thin + 1
        m, v = wmr.welford(list(ref["samples"][f - 1::thin]))
        assert got["count"] == n
        print(f"{name} ({first}, {thin}): n = {n}, mean off by {np.max(np.abs(got['mean'] - m)):.1e}, "
              f"var by {np.max(np.abs(got['var'] - v)):.1e} (max var {np.max(v):.3g})")
        _assert_moments(got["mean"], got["var"], m, v)
        _same(got, plain)                                                # moments change no bit of the chain
        if n == 1:
            assert not np.any(got["var"])


def test_pooled_moments_are_the_chan_combination_of_the_chains(ctx):
    import sbtv
    q = skc.problem("sq-s3")
    kw = dict(y=np.stack([q["y"]] * 3), seed=3)
    per = _run(ctx, "sq-s3", posterior=dict(first=2), **kw)
    pooled = _run(ctx, "sq-s3", posterior=dict(first=2, pooled=True), **kw)
    n, m, v = sbtv.combine_moments([(per["count"][b], per["mean"][b], per["var"][b]) for b in range(3)])
    assert pooled["count"] == n == 3 * (q["op"]["samples"] - 1)
    np.testing.assert_allclose(pooled["mean"], m, rtol=1e-12)
    np.testing.assert_allclose(pooled["var"], v, rtol=1e-12)
    _same(per, pooled)
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, "sq-s3", posterior=dict(pooled=True), **dict(kw, theta_op=np.array([0.02, 0.02, 0.03])))
    assert e.value.code == -1


# ---- 5. the C ABI: optional outputs, refusals ------------------------------------------------------------------------
def _raw_call(ctx, name, opt=None, **over):
    """sbtv_skrock through ctypes with every argument valid unless overridden: (return code, outputs)."""
    from sbtv import _lib as L
    q = skc.problem(name)
    y = L.Images(q["y"])
    M, N = y.M, y.N
    ko = dict(q["op"], seed=1, chain_offset=0)
    ko.update(opt or {})
    o = L.sbtv_skrock_opts(ko["samples"], ko["stages"], ko["chambolleit"], ko["lambda"], ko["delta"], ko["eta"], ko["seed"],
                           ko["chain_offset"])
    S = max(ko["samples"], 1)
    taps = _blur(q)._cm(1)
    th, s2 = np.array([q["theta"]]), np.array([q["sigma2"]])
    mo = L.sbtv_moments_opts(0, 1, 0)
    bufs = dict(gx=np.zeros(S), logpi=np.zeros(S), x_last=np.zeros(M * N), post_mean=np.zeros(M * N), post_var=np.zeros(M * N),
                post_count=np.zeros(1, dtype=np.int64))
    a = dict(y=y.ptr, M=M, N=N, taps=L.vptr(taps), taille=7, op=C.byref(o), theta=L.vptr(th), sigma2=L.vptr(s2), mo=C.byref(mo),
             **{k: L.vptr(v) for k, v in bufs.items()})
    a.update(over)
    rc = ctx.lib.sbtv_skrock(ctx.h, a["y"], a["M"], a["N"], 1, a["taps"], a["taille"], a["op"], a["theta"], a["sigma2"], None, None,
                             a["gx"], a["logpi"], a["x_last"], a["mo"], a["post_mean"], a["post_var"], a["post_count"], 0)
    return rc, bufs


def test_chain_and_traces_do_not_depend_on_what_is_requested(ctx):
    """With and without moments, with both traces, one or none: the same bits in what is returned."""
    name = "sq-s2"
    rc, full = _raw_call(ctx, name)
    assert rc == 0 and full["post_count"][0] == skc.problem(name)["op"]["samples"]
    nomom = dict(mo=None, post_mean=None, post_var=None, post_count=None)
    for over in (nomom, dict(gx=None), dict(logpi=None), dict(gx=None, logpi=None), dict(nomom, gx=None, logpi=None),
                 dict(post_var=None, post_count=None)):
        rc, got = _raw_call(ctx, name, **over)
        assert rc == 0, over
        for k, v in got.items():
            if k not in over:
                np.testing.assert_array_equal(v, full[k], err_msg=f"{k} with {sorted(over)}")
    r = _run(ctx, name, seed=1, posterior=True)
    np.testing.assert_array_equal(np.asarray(r["x"]).ravel(order="F"), full["x_last"])
    np.testing.assert_array_equal(r["gx"], full["gx"])
    np.testing.assert_array_equal(np.asarray(r["mean"]).ravel(order="F"), full["post_mean"])


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, through the C ABI and through the Python mirror, and a valid call
    succeeds afterwards."""
    import sbtv
    name = "sq-s2"
    S = skc.problem(name)["op"]["samples"]
    nan, inf = float("nan"), float("inf")
    bad = [dict(samples=1), dict(samples=0), dict(stages=1), dict(stages=0), dict(stages=-3), dict(chain_offset=-1)]
    for f in ("lambda", "delta", "eta"):
        bad += [{f: 0.0}, {f: -1.0}, {f: nan}, {f: inf}]
    ctx.reset_calls()
    for kw in bad:
        rc, _ = _raw_call(ctx, name, opt=kw)
        assert rc == -1, (kw, rc)
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(theta_op=0.0), dict(theta_op=-1.0), dict(theta_op=nan), dict(sigma2=0.0), dict(sigma2=inf),
               dict(posterior=dict(thin=0)), dict(posterior=dict(first=S + 1)), dict(posterior=dict(first=-1))):
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, **kw)
        assert e.value.code == -1, kw
    for kw in (dict(chambolleit=0), dict(chambolleit=-2)):
        rc, _ = _raw_call(ctx, name, opt=kw)
        assert rc == -3, (kw, rc)                                                     # SBTV_ERR_MAXITER, as sbtv_myula
        with pytest.raises(sbtv.SbtvError) as e:
            _run(ctx, name, **kw)
        assert e.value.code == -3, kw
    with pytest.raises(sbtv.SbtvError) as e:
        sbtv.skrock(dict(_op(name), y=np.ones((33, 35))), ctx=ctx)                    # an odd pixel count
    assert e.value.code == -2
    for over, code in ((dict(y=None), -1), (dict(taps=None), -1), (dict(op=None), -1), (dict(theta=None), -1),
                       (dict(sigma2=None), -1), (dict(taille=16), -10), (dict(taille=0), -10), (dict(post_mean=None), -1),
                       (dict(mo=None), -1), (dict(mo=None, post_mean=None, post_var=None), -1)):
        rc, _ = _raw_call(ctx, name, **over)
        assert rc == code, (over, rc)
    assert ctx.calls == 0
    rc, bufs = _raw_call(ctx, name)
    assert rc == 0 and bufs["post_count"][0] == S and np.all(np.isfinite(bufs["logpi"]))
    assert ctx.calls == 0                                                 # the operator layer counts nothing (include/sbtv.h)


# ---- 6. device pointers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sq-s2", "sq-s3"])
def test_device_tensors_give_the_same_bits(ctx, name):
    """Both parities of the stage count: the last sample ends in the caller's buffer or in the second one."""
    import sbtv
    q = skc.problem(name)
    post = dict(first=2, thin=2)
    x0 = 0.5 * q["y"] + 20.0
    host = _run(ctx, name, q["noise"], x0=x0, posterior=post)
    dev = _run(ctx, name, sbtv.to_device(q["noise"]), x0=sbtv.to_device(x0), posterior=post, y=sbtv.to_device(q["y"]))
    for k in ("gx", "logpi"):
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)
    assert dev["count"] == host["count"]
    for k in ("x", "mean", "var"):
        assert dev[k].is_cuda
        np.testing.assert_array_equal(sbtv.to_host(dev[k]), np.asarray(host[k]), err_msg=k)
