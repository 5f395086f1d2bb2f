"""GPU: the MYULA chain of the wavelet-l1 model at a fixed theta with the posterior moments of its samples in the image and
in the coefficient domain (sbtv_myula_wavelet, csrc/wavelet_myula.hip) against the NumPy restatement
(tests/wavelet_myula_restatement.py) on the cases of tests/wavelet_posterior_cases.py.

Parity with injected noise: traces to rtol 1e-9 and the last sample to 1e-9 max|X|, the figures of
tests/test_gpu_wavelet_sapg.py (the chain is not chaotic: a 1e-12 perturbation of case a's start is 2e-14 after 24 samples on
the CPU); moments with _assert_moments of tests/test_gpu_posterior.py.  The accumulators themselves are checked to the bit
against a NumPy Welford of the device's own samples.  Statistics: 8 Philox chains against 8 restatement chains with NumPy
normals, |difference of the group means| <= 3 pooled standard errors, the criterion of tests/test_gpu_sapg_long.py (two NumPy
groups, seeds 100.. and 200.., differ by 1.28 SE on the CPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_posterior import _assert_moments

import wavelet_myula_restatement as wmr
import wavelet_posterior_cases as wpc
import wavelet_sapg_cases as wsc

pytestmark = pytest.mark.gpu

TRACES = ("gXTrace", "logPiTraceX")


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", p["psf_size"], wsc.wc.PSF_PARAMS)[0])


def _run(ctx, p, nz=None, y=None, theta=None, sigma2=None, posterior=None, **opkw):
    """sbtv.myula_wavelet on problem p (all its images in one call), as a list of result dicts per chain."""
    import sbtv
    op = dict(p["op"], **opkw)
    y = p["y"] if y is None else y
    theta = p["theta"] if theta is None else theta
    sigma2 = p["sigma2"] if sigma2 is None else sigma2
    if y.shape[0] == 1:
        return [sbtv.myula_wavelet(y[0], _blur(p), p["h"], p["levels"], op, theta=theta, sigma2=sigma2,
                                   noise=None if nz is None else nz[:, 0], posterior=posterior, ctx=ctx)]
    return sbtv.myula_wavelet(y, _blur(p), p["h"], p["levels"], op, theta=theta, sigma2=sigma2, noise=nz, posterior=posterior,
                              ctx=ctx)


def _same_chain(a, b):
    for k in TRACES:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(np.asarray(a["Xlast_sample"]), np.asarray(b["Xlast_sample"]))


# ---- 1. parity with injected noise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,first,thin", [("a", 1, 1), ("a", 3, 2), ("a", 24, 1), ("b", 1, 1), ("c", 2, 3), ("d", 1, 1),
                                             ("e", 1, 1)])
def test_chain_traces_and_moments_match_the_restatement(ctx, name, first, thin):
    """(a) 64 x 64 Haar levels 4 at three selections, the last one a single sample; (b) 100 x 90 D4, two chains with their own
    theta, sigma2 and noise: chirp-z, tiles cut at both image edges; (c) 66 x 18 levels 2: level 1 is the only level, second
    tiles of two rows / two columns; (d) 2 x 2; (e) 512 x 256: the grid-stride loop of the step kernel."""
    p, ref = wpc.problem(name), wpc.reference(name)
    S = p["op"]["samples"]
    got = _run(ctx, p, wpc.noise(name), posterior=dict(first=first, thin=thin, coefficients=True))
    n = (S - first) // thin + 1
    for b, (r, rr) in enumerate(zip(got, ref)):
        xs = float(np.max(np.abs(rr["samples"][-1])))
        ex = float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - rr["samples"][-1])))
        for k, c in (("gXTrace", rr["gx"]), ("logPiTraceX", rr["logpi"])):
            a = np.asarray(r[k])
            assert a.shape == c.shape == (S,), (k, a.shape)
            print(f"{name} chain {b} {k}: worst rel {np.max(np.abs(a / c - 1)):.1e}")
            np.testing.assert_allclose(a, c, rtol=1e-9, atol=0, err_msg=k)
        print(f"{name} chain {b}: max|X - ref| / max|X| = {ex / xs:.1e}, n = {r['posteriorcount']}")
        assert ex <= 1e-9 * xs
        assert r["posteriorcount"] == n
        m, v = wmr.two_pass(rr["images"][first - 1::thin])
        _assert_moments(r["posteriormean"], r["posteriorvar"], m, v)
        m, v = wmr.two_pass(rr["samples"][first - 1::thin])
        _assert_moments(r["coefmean"], r["coefvar"], m, v)
        if n == 1:
            assert not np.any(r["posteriorvar"]) and not np.any(r["coefvar"])


# ---- 2. the accumulators to the bit: Welford of the device's own samples -------------------------------------------
def test_moments_are_the_welford_of_the_devices_own_samples_bit_for_bit(ctx):
    """With injected noise the chain is deterministic, so xw_last of calls with samples = 2..12 gives every sample; sample 1
    is W'y.  NumPy Welford (the device's arithmetic, one rounding per operation) over sbtv.mirdwt_TI2D of those samples, and
    over the samples themselves, must give the bits of the fused accumulators."""
    import sbtv
    p, S = wpc.problem("a"), 12
    nz = wpc.noise("a", S)
    Xs = [np.array(sbtv.mrdwt_TI2D(p["y"][0], p["h"], p["levels"], ctx=ctx))]
    Xs += [np.array(_run(ctx, p, nz[:s - 1], samples=s)[0]["Xlast_sample"]) for s in range(2, S + 1)]
    imgs = [np.array(sbtv.mirdwt_TI2D(X, p["h"], p["levels"], ctx=ctx)) for X in Xs]
    for first, thin in ((1, 1), (2, 3)):
        r = _run(ctx, p, nz, samples=S, posterior=dict(first=first, thin=thin, coefficients=True))[0]
        np.testing.assert_array_equal(np.asarray(r["Xlast_sample"]), Xs[-1])
        assert r["posteriorcount"] == len(imgs[first - 1::thin])
        for dom, xs in (("posterior", imgs), ("coef", Xs)):
            m, v = wmr.welford(xs[first - 1::thin])
            np.testing.assert_array_equal(r[dom + "mean"], m, err_msg=f"{dom}mean {first} {thin}")
            np.testing.assert_array_equal(r[dom + "var"], v, err_msg=f"{dom}var {first} {thin}")


# ---- 3. anchor to sbtv_SAPG_wavelet: its warm-up is this chain ------------------------------------------------------
@pytest.mark.parametrize("injected", [True, False])
def test_warmup_of_sapg_wavelet_is_this_chain(ctx, injected):
    import sbtv
    p, S, theta = wpc.problem("a"), 9, 0.03
    B, M, N = p["y"].shape
    nz = np.random.default_rng(41).standard_normal((S, M, wsc.bands(p["levels"]) * N)) if injected else None
    sop = dict(wsc.problem("a")["op"], warmup=S, samples=2, burnIn=2, th_init=theta, seed=9)
    _, sap = sbtv.SAPG_wavelet(p["y"][0], _blur(p), p["h"], p["levels"], sop, noise=nz, ctx=ctx)
    r = _run(ctx, p, None if nz is None else nz[:, None], theta=theta, sigma2=sop["sigma2"], samples=S + 1, seed=9)[0]
    np.testing.assert_allclose(r["logPiTraceX"][1:S], sap["logPiTrace_WU"][1:], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(np.asarray(r["Xlast_sample"]), np.asarray(sap["Xlast_sample"]))


# ---- 4. moments change no bit of the chain; Philox streams ----------------------------------------------------------
def test_moments_change_no_bit_and_philox_streams_follow_chain_offset(ctx):
    p = wpc.problem("b")
    plain = _run(ctx, p, seed=5)
    for post in (True, dict(first=2, thin=2, coefficients=True), None):
        for a, b in zip(_run(ctx, p, seed=5, posterior=post), plain):
            _same_chain(a, b)
    assert plain[0]["gXTrace"][1] != plain[1]["gXTrace"][1]                          # two streams
    # chain 1 of the batch at chain_offset 0 = a call of its own at chain_offset 1
    alone = _run(ctx, p, y=p["y"][1:], theta=p["theta"][1:], sigma2=p["sigma2"][1:], seed=5, chain_offset=1,
                 posterior=dict(coefficients=True))[0]
    both = _run(ctx, p, seed=5, posterior=dict(coefficients=True))[1]
    _same_chain(alone, both)
    for k in ("posteriormean", "posteriorvar", "coefmean", "coefvar"):
        np.testing.assert_array_equal(alone[k], both[k], err_msg=k)
    other = _run(ctx, p, seed=6)
    assert other[0]["gXTrace"][1] != plain[0]["gXTrace"][1]
    assert other[0]["gXTrace"][0] == plain[0]["gXTrace"][0]                          # the start state draws nothing


# ---- 5. pooled ------------------------------------------------------------------------------------------------------
def test_pooled_moments_are_the_chan_combination_of_the_chains(ctx):
    import sbtv
    p = wpc.problem("a")
    y3, th, s2 = np.repeat(p["y"], 3, axis=0), np.repeat(p["theta"], 3), np.repeat(p["sigma2"], 3)
    kw = dict(y=y3, theta=th, sigma2=s2, samples=8, seed=3)
    per = _run(ctx, p, posterior=dict(first=2, coefficients=True), **kw)
    pooled = _run(ctx, p, posterior=dict(first=2, pooled=True, coefficients=True), **kw)
    for dom in ("posterior", "coef"):
        n, m, v = sbtv.combine_moments([(r["posteriorcount"], r[dom + "mean"], r[dom + "var"]) for r in per])
        assert n == 21 == pooled[0]["posteriorcount"]
        for r in pooled:
            np.testing.assert_allclose(r[dom + "mean"], m, rtol=1e-12, atol=0)
            np.testing.assert_allclose(r[dom + "var"], v, rtol=1e-12, atol=0)
    for a, b in zip(per, pooled):
        _same_chain(a, b)
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, p, posterior=dict(pooled=True), **dict(kw, theta=np.array([0.03, 0.03, 0.04])))
    assert e.value.code == -1
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, p, posterior=dict(pooled=True), **dict(kw, sigma2=s2 * np.array([1.0, 1.0, 2.0])))
    assert e.value.code == -1


# ---- 6. device tensors ----------------------------------------------------------------------------------------------
def test_device_tensors_give_the_same_bits(ctx):
    import sbtv
    p, nz = wpc.problem("b"), wpc.noise("b")
    post = dict(first=2, thin=3, coefficients=True)
    host = _run(ctx, p, nz, posterior=post)
    nzd = sbtv.to_device(nz.reshape((-1,) + nz.shape[2:]))         # step-major, column-major coefficient arrays
    res = sbtv.myula_wavelet(sbtv.to_device(p["y"]), _blur(p), p["h"], p["levels"], p["op"], theta=p["theta"],
                             sigma2=p["sigma2"], noise=nzd, posterior=post, ctx=ctx)
    for b in range(2):
        for k in TRACES:
            np.testing.assert_array_equal(res[b][k], host[b][k], err_msg=k)
        assert res[b]["posteriorcount"] == host[b]["posteriorcount"]
        for k in ("Xlast_sample", "posteriormean", "posteriorvar", "coefmean", "coefvar"):
            assert res[b][k].is_cuda
            np.testing.assert_array_equal(sbtv.to_host(res[b][k]), np.asarray(host[b][k]), err_msg=k)


def test_device_noise_that_is_not_the_expected_dense_float64_array_is_refused(ctx):
    """The step kernel reads (samples-1) * B * dimX doubles from a device noise pointer, so the host mirror refuses a tensor
    that is too short, too long, float32 or strided before anything is launched; the right one still runs."""
    import sbtv
    p, nz = wpc.problem("c"), wpc.noise("c")
    yd, A = sbtv.to_device(p["y"][0]), _blur(p)
    good = sbtv.to_device(nz[:, 0])
    call = lambda t: sbtv.myula_wavelet(yd, A, p["h"], p["levels"], p["op"], theta=0.03, sigma2=p["sigma2"][0], noise=t, ctx=ctx)
    flat = good.permute(0, 2, 1).contiguous().reshape(-1)
    for bad in (flat[:-2], flat.repeat(2), flat.float(), flat.repeat(2)[::2]):
        with pytest.raises(ValueError, match="noise"):
            call(bad)
    np.testing.assert_array_equal(call(good)["gXTrace"], call(flat)["gXTrace"])
    np.testing.assert_array_equal(call(flat)["gXTrace"], _run(ctx, p, nz)[0]["gXTrace"])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def _raw_call(ctx, p, **over):
    """sbtv_myula_wavelet through ctypes with every argument valid unless overridden: (return code, outputs kept alive)."""
    from sbtv import _lib as L
    y = L.Images(p["y"][0])
    M, N, nb = y.M, y.N, wsc.bands(p["levels"])
    S = p["op"]["samples"]
    taps = _blur(p)._cm(1)
    h = np.ascontiguousarray(p["h"], dtype=np.float64)
    o = L.sbtv_myula_wavelet_opts(S, p["op"]["lambda"], p["op"]["gamma"], 1, 0)
    th, s2 = np.array([0.03]), np.array([float(p["sigma2"][0])])
    mo = L.sbtv_moments_opts(0, 1, 0)
    bufs = dict(gx=np.zeros(S), logpi=np.zeros(S), xw_last=np.zeros(nb * M * N), post_mean=np.zeros(M * N),
                post_var=np.zeros(M * N), post_count=np.zeros(1, dtype=np.int64), coef_mean=np.zeros(nb * M * N),
                coef_var=np.zeros(nb * M * N))
    a = dict(taps=L.vptr(taps), taille=7, theta=L.vptr(th), sigma2=L.vptr(s2), mo=C.byref(mo),
             **{k: L.vptr(v) for k, v in bufs.items()})
    a.update(over)
    rc = ctx.lib.sbtv_myula_wavelet(ctx.h, y.ptr, M, N, 1, a["taps"], a["taille"], L.vptr(h), h.size, p["levels"], C.byref(o),
                                    a["theta"], a["sigma2"], None, None, a["gx"], a["logpi"], a["xw_last"], a["mo"],
                                    a["post_mean"], a["post_var"], a["post_count"], a["coef_mean"], a["coef_var"], 0)
    return rc, bufs


def test_refusals(ctx):
    """Each is refused with its code before any GPU work, and a valid call succeeds afterwards."""
    import sbtv
    p = wpc.problem("c")
    A, y, h = _blur(p), p["y"][0], p["h"]
    S = p["op"]["samples"]
    call = lambda arr=y, hh=h, levels=p["levels"], theta=0.03, sigma2=float(p["sigma2"][0]), posterior=None, **kw: \
        sbtv.myula_wavelet(arr, A, hh, levels, dict(p["op"], **kw), theta=theta, sigma2=sigma2, posterior=posterior, ctx=ctx)
    nan, inf = float("nan"), float("inf")
    bad = [dict(samples=1), dict(gamma=0.0), dict(gamma=nan), dict(gamma=inf), {"lambda": -1.0}, {"lambda": inf},
           dict(chain_offset=-1), dict(theta=0.0), dict(theta=-0.1), dict(theta=nan), dict(theta=inf), dict(sigma2=0.0),
           dict(sigma2=nan), dict(sigma2=inf), dict(posterior=dict(thin=0)), dict(posterior=dict(first=-1)),
           dict(posterior=dict(first=S + 1))]
    for kw in bad:
        with pytest.raises(sbtv.SbtvError) as e:
            call(**kw)
        assert e.value.code == -1, (kw, e.value.code)
    d4 = sbtv.daubcqf(4)
    for hh, levels, arr, code in ((np.array([1.0, 0.25]), 3, y, -1),                # not orthonormal
                                  (np.sqrt(2.0) * np.array([0.75, 0.25]), 3, y, -1),
                                  (np.ones(3), 3, y, -1), (h, 1, y, -1),
                                  (d4, 4, np.ones((12, 12)), -2),                   # too small for the depth
                                  (h, 3, np.ones((33, 35)), -2)):                   # an odd pixel count
        with pytest.raises(sbtv.SbtvError) as e:
            call(arr=arr, hh=hh, levels=levels)
        assert e.value.code == code, (hh.size, levels, arr.shape, e.value.code)
    # what the Python mirror cannot express: missing pointers and the moment-pointer rules
    for over, code in ((dict(taps=None), -8), (dict(taille=16), -10), (dict(theta=None), -1), (dict(sigma2=None), -1),
                       (dict(post_mean=None, post_var=None, coef_mean=None, coef_var=None), -1),   # neither mean
                       (dict(post_mean=None, coef_var=None), -1),                                  # post_var alone
                       (dict(coef_mean=None, post_var=None), -1),                                  # coef_var alone
                       (dict(mo=None), -1)):                                                       # outputs without options
        rc, _ = _raw_call(ctx, p, **over)
        assert rc == code, (over, rc)
    rc, bufs = _raw_call(ctx, p)
    assert rc == 0 and bufs["post_count"][0] == S
    r = call(posterior=True)
    np.testing.assert_array_equal(np.asarray(r["posteriormean"]).ravel(order="F"), bufs["post_mean"])
    np.testing.assert_array_equal(r["gXTrace"], bufs["gx"])
    # only the image moments / only the coefficient moments are legal requests
    for over in (dict(coef_mean=None, coef_var=None), dict(post_mean=None, post_var=None), dict(post_var=None, post_count=None)):
        assert _raw_call(ctx, p, **over)[0] == 0, over


# ---- 8. statistics --------------------------------------------------------------------------------------------------
STAT_CHAINS, STAT_SAMPLES, STAT_FROM = 8, 150, 50


def _stat(gx):
    return float(np.mean(gx[STAT_FROM - 1:STAT_SAMPLES]))                           # iterations 50..150


@functools.lru_cache(maxsize=None)
def _stat_reference():
    """mean gx over iterations 50..150 of 8 restatement chains on case a, NumPy normals (computed once)."""
    p = wpc.problem("a")
    shape = (STAT_SAMPLES - 1, p["y"].shape[1], wsc.bands(p["levels"]) * p["y"].shape[2])
    return np.array([_stat(wpc.chain(p, 0, np.random.default_rng(100 + c).standard_normal(shape), samples=STAT_SAMPLES)["gx"])
                     for c in range(STAT_CHAINS)])


def test_gx_of_philox_chains_within_the_restatement_chains_spread(ctx):
    p = wpc.problem("a")
    y8 = np.repeat(p["y"], STAT_CHAINS, axis=0)
    res = _run(ctx, p, y=y8, theta=np.repeat(p["theta"], STAT_CHAINS), sigma2=np.repeat(p["sigma2"], STAT_CHAINS),
               samples=STAT_SAMPLES, seed=7)
    gpu = np.array([_stat(r["gXTrace"]) for r in res])
    ref = _stat_reference()
    assert len(set(gpu.tolist())) == STAT_CHAINS                                    # all different streams
    n = STAT_CHAINS
    se = np.sqrt(gpu.var(ddof=1) / n + ref.var(ddof=1) / n)
    diff = abs(gpu.mean() - ref.mean())
    print(f"mean gx: device {gpu.mean():.8g} (spread {gpu.std(ddof=1) / gpu.mean():.2e}), restatement {ref.mean():.8g} "
          f"(spread {ref.std(ddof=1) / ref.mean():.2e}), |d| = {diff:.3g}, z = {diff / se:.2f} SE")
    assert diff <= 3.0 * se
