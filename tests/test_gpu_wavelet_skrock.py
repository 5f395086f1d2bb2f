"""GPU: the SK-ROCK chain of the wavelet-l1 model at a fixed theta (sbtv_skrock_wavelet, csrc/wavelet_skrock.hip and the stage
kernels of csrc/wavelet_chain.hip) against the NumPy restatement (tests/wavelet_skrock_restatement.py)
on the runs of tests/wavelet_skrock_cases.py.  Every run uses delta = 0.8 l_s / (1 / sigma2 + 1 / lambda).

Parity with injected noise: traces to rtol 1e-9 and the last sample to 1e-9 max|X|, the bars of
tests/test_gpu_wavelet_posterior.py.  Moments: rtol 1e-9 against the restatement's Welford recursion of the restated samples,
with the absolute floor that the sample bar itself implies (a sample may be off by e = 1e-9 max|X|, so may a mean; a variance
by 2 sd e).  Statistics: 8 Philox chains against 8 restatement chains with NumPy normals, |difference of the group means| <= 3
pooled standard errors, the rule of test_gx_of_philox_chains_within_the_restatement_chains_spread.

Measured on an MI355X (each test prints its figures): traces off by at most 1.0e-14 relative (logpi of case a at s = 10; <= 1.3e-15
at s = 2, 3 on every case), last sample by at most 1.6e-14 max|X| (case a, s = 10; <= 2.3e-15 elsewhere); the Philox chain
4.9e-15 / 2.0e-15; means off by <= 5.7e-13 and variances by <= 1.9e-11 absolute (floors 2.3e-07 and 7.0e-06 or more); the
statistic: device 1677370 against restatement 1680147, 2.00 SE apart.  The whole file takes 6 s."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_image

import philox_restatement as phr
import wavelet_myula_restatement as wmr
import wavelet_posterior_cases as wpc
import wavelet_sapg_cases as wsc
import wavelet_skrock_cases as wkc
import wavelet_skrock_restatement as wkr

pytestmark = pytest.mark.gpu

TRACES = ("gXTrace", "logPiTraceX")
MOMENTS = ("posteriormean", "posteriorvar", "coefmean", "coefvar")


def _blur(p):
    import sbtv
    return sbtv.BlurOperator(sbtv.psf_family("gaussian", p["psf_size"], wsc.wc.PSF_PARAMS)[0])


def _run(ctx, name, stages, samples, nz=None, y=None, theta=None, sigma2=None, posterior=None, **opkw):
    """sbtv.skrock_wavelet on a case (all its images in one call), as a list of result dicts per chain."""
    import sbtv
    p = wpc.problem(name)
    op = dict(wkc.options(name, stages, samples), **opkw)
    y = p["y"] if y is None else y
    theta = p["theta"] if theta is None else theta
    sigma2 = p["sigma2"] if sigma2 is None else sigma2
    if y.shape[0] == 1:
        return [sbtv.skrock_wavelet(y[0], _blur(p), p["h"], p["levels"], op, theta=theta, sigma2=sigma2,
                                    noise=None if nz is None else nz[:, 0], posterior=posterior, ctx=ctx)]
    return sbtv.skrock_wavelet(y, _blur(p), p["h"], p["levels"], op, theta=theta, sigma2=sigma2, noise=nz, posterior=posterior,
                               ctx=ctx)


def _same_chain(a, b):
    for k in TRACES:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(np.asarray(a["Xlast_sample"]), np.asarray(b["Xlast_sample"]))


def _assert_chain(tag, r, rr, S):
    xs = float(np.max(np.abs(rr["samples"][-1])))
    ex = float(np.max(np.abs(np.asarray(r["Xlast_sample"]) - rr["samples"][-1])))
    for k, c in (("gXTrace", rr["gx"]), ("logPiTraceX", rr["logpi"])):
        a = np.asarray(r[k])
        assert a.shape == c.shape == (S,), (k, a.shape)
        print(f"{tag} {k}: worst rel {np.max(np.abs(a / c - 1)):.1e}")
        np.testing.assert_allclose(a, c, rtol=1e-9, atol=0, err_msg=k)
    print(f"{tag}: max|X - ref| / max|X| = {ex / xs:.1e}")
    assert ex <= 1e-9 * xs


# ---- 1. parity with injected noise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,stages,samples", wkc.RUNS, ids=[f"{n}-s{s}-S{S}" for n, s, S in wkc.RUNS])
def test_chain_and_traces_match_the_restatement(ctx, name, stages, samples):
    """(a) 64 x 64 Haar at s = 2 (first and last stage in consecutive launches), 3 (one middle stage) and 10; (b) 100 x 90 D4,
    chirp-z, two chains with their own theta, sigma2 and noise; (c) 66 x 18; (d) 2 x 2; (e) 512 x 256: the grid-stride loop;
    (a, s = 2, two samples): perturbation, first and last stage, no fused perturbation of a next step."""
    ref = wkc.reference(name, stages, samples)
    got = _run(ctx, name, stages, samples, wkc.noise(name, samples))
    assert len(got) == len(ref)
    for b, (r, rr) in enumerate(zip(got, ref)):
        _assert_chain(f"{name} s = {stages} chain {b}", r, rr, samples)


# ---- 2. moments -----------------------------------------------------------------------------------------------------
def _assert_moments(tag, r, rr, first, thin):
    """rtol 1e-9 against the Welford recursion of the restated samples; the floor is what the sample bar allows."""
    for dom, xs in (("posterior", rr["images"]), ("coef", rr["samples"])):
        m, v = wmr.welford(list(xs[first - 1::thin]))
        e = 1e-9 * float(np.max(np.abs(xs)))
        gm, gv = np.asarray(r[dom + "mean"]), np.asarray(r[dom + "var"])
        print(f"{tag} {dom}: mean off by {np.max(np.abs(gm - m)):.1e} (floor {e:.1e}), var by {np.max(np.abs(gv - v)):.1e} "
              f"(floor {2 * np.sqrt(np.max(v)) * e:.1e})")
        np.testing.assert_allclose(gm, m, rtol=1e-9, atol=e, err_msg=dom + "mean")
        np.testing.assert_allclose(gv, v, rtol=1e-9, atol=2 * float(np.sqrt(np.max(v))) * e, err_msg=dom + "var")


@pytest.mark.parametrize("name,stages,samples", [("a", 3, 5), ("b", 3, 4)])
def test_moments_are_the_welford_recursion_of_the_restated_samples(ctx, name, stages, samples):
    ref, nz = wkc.reference(name, stages, samples), wkc.noise(name, samples)
    plain = _run(ctx, name, stages, samples, nz)
    for first, thin in ((1, 1), (2, 2), (samples, 1)):
        got = _run(ctx, name, stages, samples, nz, posterior=dict(first=first, thin=thin, coefficients=True))
        n = (samples - first) // thin + 1
        for b, (r, rr) in enumerate(zip(got, ref)):
            assert r["posteriorcount"] == n
            _assert_moments(f"{name} ({first}, {thin}) chain {b}", r, rr, first, thin)
            _same_chain(r, plain[b])                                     # moments change no bit of the chain
            if n == 1:
                assert not np.any(r["posteriorvar"]) and not np.any(r["coefvar"])
    for r, q in zip(_run(ctx, name, stages, samples, nz, posterior=True), plain):          # image moments alone
        _same_chain(r, q)
        assert "coefmean" not in r


def test_pooled_moments_are_the_chan_combination_of_the_chains(ctx):
    import sbtv
    p = wpc.problem("a")
    y3, th, s2 = np.repeat(p["y"], 3, axis=0), np.repeat(p["theta"], 3), np.repeat(p["sigma2"], 3)
    kw = dict(y=y3, theta=th, sigma2=s2, seed=3)
    per = _run(ctx, "a", 3, 6, posterior=dict(first=2, coefficients=True), **kw)
    pooled = _run(ctx, "a", 3, 6, posterior=dict(first=2, pooled=True, coefficients=True), **kw)
    for dom in ("posterior", "coef"):
        n, m, v = sbtv.combine_moments([(r["posteriorcount"], r[dom + "mean"], r[dom + "var"]) for r in per])
        assert n == 15 == pooled[0]["posteriorcount"]
        for r in pooled:
            np.testing.assert_allclose(r[dom + "mean"], m, rtol=1e-12, atol=0)
            np.testing.assert_allclose(r[dom + "var"], v, rtol=1e-12, atol=0)
    for a, b in zip(per, pooled):
        _same_chain(a, b)
    with pytest.raises(sbtv.SbtvError) as e:
        _run(ctx, "a", 3, 6, posterior=dict(pooled=True), **dict(kw, theta=np.array([0.03, 0.03, 0.04])))
    assert e.value.code == -1


# ---- 3. the generator -----------------------------------------------------------------------------------------------
def test_philox_chain_is_the_restatement_fed_with_the_restated_normals(ctx):
    """noise = None: sample ii draws Philox step ii - 2, pair q of chain b the counters (q, step, chain_offset + b): the MYULA
    counters.  8 x 8, s = 3, 6 samples, chain_offset 2."""
    import sbtv
    M = N = 8
    levels, S, s, seed, off = 3, 6, 3, 11, 2
    y, sigma, H = wsc._setup(synth_image(M, N, 4), 7, 3)
    h = wsc.wc.daub(2)
    lam = wsc.options(sigma, S, 0)["lambda"]
    op = dict(samples=S, stages=s, eta=0.05, delta=0.8 * wkr.max_step(s, 0.05, sigma ** 2, lam), seed=seed, chain_offset=off,
              **{"lambda": lam})
    nz = phr.as_arrays(phr.chain_normals(M * N * wsc.bands(levels), S - 1, 1, seed, off), M)[:, 0]      # (steps, M, (3J+1) N)
    ref = wkr.skrock_wavelet_chain(y, H, h, levels, op, 0.03, sigma ** 2, nz)
    A = sbtv.BlurOperator(sbtv.psf_family("gaussian", 7, wsc.wc.PSF_PARAMS)[0])
    r = sbtv.skrock_wavelet(y, A, h, levels, op, theta=0.03, sigma2=sigma ** 2, ctx=ctx)
    _assert_chain("8 x 8 Philox", r, ref, S)
    inj = sbtv.skrock_wavelet(y, A, h, levels, op, theta=0.03, sigma2=sigma ** 2, noise=nz, ctx=ctx)
    _assert_chain("8 x 8 restated normals injected", inj, ref, S)


# ---- 4. independence ------------------------------------------------------------------------------------------------
def test_chains_of_a_batch_are_computed_as_alone_and_chain_offset_shifts_the_streams(ctx):
    p = wpc.problem("b")
    plain = _run(ctx, "b", 3, 4, seed=5)
    assert plain[0]["gXTrace"][1] != plain[1]["gXTrace"][1]                          # two streams
    # chain 1 of the batch at chain_offset 0 = a call of its own at chain_offset 1 (delta is the batch's)
    alone = _run(ctx, "b", 3, 4, y=p["y"][1:], theta=p["theta"][1:], sigma2=p["sigma2"][1:], seed=5, chain_offset=1,
                 posterior=dict(coefficients=True))[0]
    both = _run(ctx, "b", 3, 4, seed=5, posterior=dict(coefficients=True))[1]
    _same_chain(alone, both)
    _same_chain(both, plain[1])
    for k in MOMENTS:
        np.testing.assert_array_equal(alone[k], both[k], err_msg=k)
    # injected noise: chain 1 alone, with its own slice of the normals
    nz = wkc.noise("b", 4)
    inj = _run(ctx, "b", 3, 4, nz)
    inj1 = _run(ctx, "b", 3, 4, nz[:, 1:], y=p["y"][1:], theta=p["theta"][1:], sigma2=p["sigma2"][1:])[0]
    _same_chain(inj1, inj[1])
    other = _run(ctx, "b", 3, 4, seed=6)
    assert other[0]["gXTrace"][1] != plain[0]["gXTrace"][1]
    assert other[0]["gXTrace"][0] == plain[0]["gXTrace"][0]                          # the start state draws nothing
    shifted = _run(ctx, "b", 3, 4, seed=5, chain_offset=1)
    for b in range(2):
        assert shifted[b]["gXTrace"][0] == plain[b]["gXTrace"][0] and shifted[b]["gXTrace"][1] != plain[b]["gXTrace"][1]


def test_chain_offset_names_the_stream_of_the_same_chain_elsewhere(ctx):
    """Chain 0 at chain_offset 1 on image 1's data is chain 1 at chain_offset 0."""
    p = wpc.problem("b")
    y = np.stack([p["y"][1], p["y"][1]])
    th, s2 = np.repeat(p["theta"][1:], 2), np.repeat(p["sigma2"][1:], 2)
    d = wkc.options("b", 3, 4)["delta"]
    two = _run(ctx, "b", 3, 4, y=y, theta=th, sigma2=s2, seed=5, delta=d)
    one = _run(ctx, "b", 3, 4, y=y[1:], theta=th[1:], sigma2=s2[1:], seed=5, chain_offset=1, delta=d)[0]
    _same_chain(one, two[1])
    assert two[0]["gXTrace"][1] != two[1]["gXTrace"][1]


@pytest.mark.parametrize("stages", [2, 3])
def test_device_tensors_give_the_same_bits(ctx, stages):
    """Both parities of the stage count: the last sample ends in the caller's buffer or in the second one."""
    import sbtv
    p, nz = wpc.problem("b"), wkc.noise("b", 4)
    post = dict(first=2, thin=2, coefficients=True)
    host = _run(ctx, "b", stages, 4, nz, posterior=post)
    nzd = sbtv.to_device(nz.reshape((-1,) + nz.shape[2:]))         # step-major, column-major coefficient arrays
    res = sbtv.skrock_wavelet(sbtv.to_device(p["y"]), _blur(p), p["h"], p["levels"], wkc.options("b", stages, 4),
                              theta=p["theta"], sigma2=p["sigma2"], noise=nzd, posterior=post, ctx=ctx)
    for b in range(2):
        for k in TRACES:
            np.testing.assert_array_equal(res[b][k], host[b][k], err_msg=k)
        assert res[b]["posteriorcount"] == host[b]["posteriorcount"]
        for k in ("Xlast_sample",) + MOMENTS:
            assert res[b][k].is_cuda
            np.testing.assert_array_equal(sbtv.to_host(res[b][k]), np.asarray(host[b][k]), err_msg=k)


# ---- 5. statistics --------------------------------------------------------------------------------------------------
STAT_CHAINS, STAT_SAMPLES, STAT_FROM, STAT_STAGES = 8, 60, 30, 10


def _stat(gx):
    return float(np.mean(gx[STAT_FROM - 1:STAT_SAMPLES]))                           # samples 30..60


@functools.lru_cache(maxsize=None)
def _stat_reference():
    """mean gx over samples 30..60 of 8 restatement chains on case a, NumPy normals (computed once)."""
    p = wpc.problem("a")
    shape = (STAT_SAMPLES - 1, p["y"].shape[1], wsc.bands(p["levels"]) * p["y"].shape[2])
    return np.array([_stat(wkc.chain("a", 0, STAT_STAGES, STAT_SAMPLES, np.random.default_rng(100 + c).standard_normal(shape))["gx"])
                     for c in range(STAT_CHAINS)])


def test_gx_of_philox_chains_within_the_restatement_chains_spread(ctx):
    p = wpc.problem("a")
    y8 = np.repeat(p["y"], STAT_CHAINS, axis=0)
    res = _run(ctx, "a", STAT_STAGES, STAT_SAMPLES, y=y8, theta=np.repeat(p["theta"], STAT_CHAINS),
               sigma2=np.repeat(p["sigma2"], STAT_CHAINS), seed=7)
    gpu = np.array([_stat(r["gXTrace"]) for r in res])
    ref = _stat_reference()
    assert len(set(gpu.tolist())) == STAT_CHAINS                                    # all different streams
    n = STAT_CHAINS
    se = np.sqrt(gpu.var(ddof=1) / n + ref.var(ddof=1) / n)
    diff = abs(gpu.mean() - ref.mean())
    print(f"mean gx: device {gpu.mean():.8g} (spread {gpu.std(ddof=1) / gpu.mean():.2e}), restatement {ref.mean():.8g} "
          f"(spread {ref.std(ddof=1) / ref.mean():.2e}), |d| = {diff:.3g}, z = {diff / se:.2f} SE")
    assert diff <= 3.0 * se


# ---- 6. refusals and the call counter -------------------------------------------------------------------------------
def _raw_call(ctx, name, stages, samples, opt=None, **over):
    """sbtv_skrock_wavelet through ctypes with every argument valid unless overridden: (return code, outputs kept alive)."""
    from sbtv import _lib as L
    p = wpc.problem(name)
    y = L.Images(p["y"][0])
    M, N, nb = y.M, y.N, wsc.bands(p["levels"])
    S = samples
    taps = _blur(p)._cm(1)
    h = np.ascontiguousarray(p["h"], dtype=np.float64)
    ko = dict(wkc.options(name, stages, samples), seed=1, chain_offset=0)
    ko.update(opt or {})
    o = L.sbtv_skrock_wavelet_opts(ko["samples"], ko["stages"], ko["lambda"], ko["delta"], ko["eta"], ko["seed"], ko["chain_offset"])
    th, s2 = np.array([0.03]), np.array([float(p["sigma2"][0])])
    mo = L.sbtv_moments_opts(0, 1, 0)
    bufs = dict(gx=np.zeros(S), logpi=np.zeros(S), xw_last=np.zeros(nb * M * N), post_mean=np.zeros(M * N),
                post_var=np.zeros(M * N), post_count=np.zeros(1, dtype=np.int64), coef_mean=np.zeros(nb * M * N),
                coef_var=np.zeros(nb * M * N))
    a = dict(taps=L.vptr(taps), taille=7, theta=L.vptr(th), sigma2=L.vptr(s2), mo=C.byref(mo),
             **{k: L.vptr(v) for k, v in bufs.items()})
    a.update(over)
    rc = ctx.lib.sbtv_skrock_wavelet(ctx.h, y.ptr, M, N, 1, a["taps"], a["taille"], L.vptr(h), h.size, p["levels"], C.byref(o),
                                     a["theta"], a["sigma2"], None, None, a["gx"], a["logpi"], a["xw_last"], a["mo"],
                                     a["post_mean"], a["post_var"], a["post_count"], a["coef_mean"], a["coef_var"], 0)
    return rc, bufs


def test_refusals(ctx):
    """Each is refused with its code before any GPU work (the call counter stands still), through the C-ABI and through the
    Python mirror, and a valid call succeeds afterwards."""
    import sbtv
    p = wpc.problem("c")
    A, y, h = _blur(p), p["y"][0], p["h"]
    S, s = 4, 2
    base = wkc.options("c", s, S)
    call = lambda arr=y, levels=p["levels"], theta=0.03, sigma2=float(p["sigma2"][0]), posterior=None, **kw: \
        sbtv.skrock_wavelet(arr, A, h, levels, dict(base, **kw), theta=theta, sigma2=sigma2, posterior=posterior, ctx=ctx)
    nan, inf = float("nan"), float("inf")
    new = [dict(stages=1), dict(stages=0), dict(stages=-3), dict(delta=0.0), dict(delta=-1.0), dict(delta=nan), dict(delta=inf),
           dict(eta=0.0), dict(eta=-0.05), dict(eta=nan), dict(eta=inf)]
    inherited = [dict(samples=1), {"lambda": -1.0}, {"lambda": inf}, dict(chain_offset=-1), dict(theta=0.0), dict(theta=nan),
                 dict(sigma2=0.0), dict(sigma2=inf), dict(posterior=dict(thin=0)), dict(posterior=dict(first=S + 1))]
    ctx.reset_calls()
    for kw in new + inherited:
        with pytest.raises(sbtv.SbtvError) as e:
            call(**kw)
        assert e.value.code == -1, (kw, e.value.code)
    for kw in new + [dict(samples=1), {"lambda": nan}, dict(chain_offset=-1)]:
        rc, _ = _raw_call(ctx, "c", s, S, opt=kw)
        assert rc == -1, (kw, rc)
    with pytest.raises(sbtv.SbtvError) as e:
        call(arr=np.ones((33, 35)), levels=3)                                       # an odd pixel count
    assert e.value.code == -2
    for over, code in ((dict(taps=None), -8), (dict(taille=16), -10), (dict(theta=None), -1), (dict(sigma2=None), -1),
                       (dict(post_mean=None, post_var=None, coef_mean=None, coef_var=None), -1),
                       (dict(post_mean=None, coef_var=None), -1), (dict(mo=None), -1)):
        rc, _ = _raw_call(ctx, "c", s, S, **over)
        assert rc == code, (over, rc)
    assert ctx.calls == 0
    rc, bufs = _raw_call(ctx, "c", s, S)
    assert rc == 0 and bufs["post_count"][0] == S
    r = call(posterior=True, seed=1)
    np.testing.assert_array_equal(np.asarray(r["posteriormean"]).ravel(order="F"), bufs["post_mean"])
    np.testing.assert_array_equal(r["gXTrace"], bufs["gx"])


def test_default_step_is_four_fifths_of_the_bound(ctx):
    """delta = None: 0.8 skrock_max_step at ||B||^2 = 1, the step every case here passes explicitly."""
    nz = wkc.noise("c", 4)
    want = _run(ctx, "c", 2, 4, nz)[0]
    got = _run(ctx, "c", 2, 4, nz, delta=None)[0]
    _same_chain(got, want)


@pytest.mark.parametrize("name,stages,samples", [("b", 3, 4), ("a", 2, 2), ("c", 10, 3)])
def test_call_counter(ctx, name, stages, samples):
    batch = wpc.problem(name)["batch"]
    ctx.reset_calls()
    _run(ctx, name, stages, samples, seed=2)
    assert ctx.calls == (2 * stages + 1) * batch * (samples - 1) + batch
